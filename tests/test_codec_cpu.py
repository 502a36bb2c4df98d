"""Compact proof blobs ("HBPC" version 1), the parts that need no GPU:

* tests/golden/codec_kat.json (written by tests/golden/make_codec.py from the Python restatement) pins
  version 1: the restatement still gives its digests, and so does the library's host encoder;
* hipbp_proofs_encode_host equals the restatement byte for byte, hipbp_proofs_decode_host returns
  every limb, the parser accepts what the encoder wrote, the error paths write nothing and leave
  zeroed structs;
* the layout, the lane bodies' round trips over forced edge proofs and every malformed blob, run on the
  CPU by tests/codec_check.hip, a stand-alone host program, at -O2 and under ASan + UBSan;
* the host codec runs in a process that sees no device."""
import ctypes
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import codec_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "codec_check.hip")
KAT = json.load(open(os.path.join(cr.GOLDEN, "codec_kat.json"))) if os.path.exists(os.path.join(cr.GOLDEN, "codec_kat.json")) else {}
SETS = ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64")


@pytest.fixture(scope="module")
def m():
    import cudabulletproof_amd as mod
    mod.build()
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def blobs(oracle):
    """name -> (n, arrs, with_blinding, the restatement's blob), computed once."""
    out = {}
    for name in SETS:
        n, arrs, _ = cr.golden_set(name)
        f = bool(KAT[name]["with_blinding"])
        out[name] = (n, arrs, f, cr.encode(oracle, arrs, n, f))
    return out


def test_kat_fixture():
    assert sorted(KAT) == sorted(SETS)
    assert [KAT[k]["count"] for k in SETS] == [6, 6, 28, 16]
    assert [KAT[k]["with_blinding"] for k in SETS] == [False, False, True, True]
    # every reference proof of proofs_n16 / proofs_n64 is compact; rpverify's `rand` cases are raw
    assert KAT["proofs_n16"]["raw_count"] == 0 and KAT["proofs_n64"]["raw_count"] == 0
    assert KAT["proofs_n16"]["bytes"] == cr.blob_bytes(6, 1, 4, 0, 0) and KAT["proofs_n64"]["bytes"] == cr.blob_bytes(6, 1, 6, 0, 0)
    d = np.load(os.path.join(cr.GOLDEN, "rpverify.npz"))
    for n in (16, 64):
        rand = int(np.sum(d[f"n{n}_kind"] == "rand"))
        assert 0 < rand <= KAT[f"rpverify_n{n}"]["raw_count"] < KAT[f"rpverify_n{n}"]["count"]


@pytest.mark.parametrize("name", SETS)
def test_restatement_gives_the_kat(blobs, oracle, name):
    n, arrs, f, blob = blobs[name]
    assert len(blob) == KAT[name]["bytes"] and hashlib.sha256(blob).hexdigest() == KAT[name]["sha256"]
    m, back = cr.decode(oracle, blob)
    assert m == n and cr.same(arrs, back, list(back))
    if name.startswith("rpverify"):   # the kinds: exactly the cases that are not as the prover leaves them
        kinds = np.frombuffer(blob[32:32 + len(arrs["V"])], np.uint8)
        d = np.load(os.path.join(cr.GOLDEN, "rpverify.npz"))
        assert all(kinds[d[f"n{n}_kind"] == "rand"] == 1) and int(kinds.sum()) == KAT[name]["raw_count"]


@pytest.mark.parametrize("name", SETS)
def test_host_encoder_equals_restatement_and_kat(m, blobs, name):
    n, arrs, f, ref = blobs[name]
    got = m.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=f)
    assert got == ref
    assert hashlib.sha256(got).hexdigest() == KAT[name]["sha256"] and len(got) == KAT[name]["bytes"]
    info = m.proof_blob_info(got)
    assert info == dict(count=len(arrs["V"]), n=n, ab_len=1, L_len=arrs["L"].shape[1], flags=int(f),
                        raw_count=KAT[name]["raw_count"], bytes=len(got))
    assert m.lib().hipbp_proof_blob_bound(len(arrs["V"]), 1, arrs["L"].shape[1], int(f)) == \
        cr.blob_bytes(len(arrs["V"]), 1, arrs["L"].shape[1], int(f), len(arrs["V"]))


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("blinding", [False, True])
def test_host_decoder_returns_every_limb(m, blobs, oracle, name, blinding):
    n, arrs, _, _ = blobs[name]
    blob = m.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=blinding)
    assert blob == cr.encode(oracle, arrs, n, blinding)
    back = m.proofs_from_bytes(blob)
    assert all(p["n"] == n and p["L_len"] == arrs["L"].shape[1] for p in back)
    got = cr.from_dicts(back, True)
    keys = [k for k in arrs if blinding or k not in ("taux", "mu")]
    assert cr.same(arrs, got, keys)
    if not blinding:   # not stored: zero
        assert not got["taux"].any() and not got["mu"].any()


def test_ab_len_two_and_empty(m, oracle):
    """ab_len = 2 has no compact slots (every proof raw); count = 0 is the header alone."""
    n, arrs, _ = cr.golden_set("proofs_n16")
    two = dict(arrs)
    two["a"] = np.concatenate([arrs["a"], arrs["a"] + np.uint64(1)], axis=1)
    two["b"] = np.concatenate([arrs["b"], arrs["b"] + np.uint64(2)], axis=1)
    blob = m.proofs_to_bytes(cr.to_dicts(two), n, with_blinding=True)
    assert blob == cr.encode(oracle, two, n, True) and m.proof_blob_info(blob)["raw_count"] == 6
    assert cr.same(two, cr.from_dicts(m.proofs_from_bytes(blob), True), list(two))
    empty = m.proofs_to_bytes([], 64)
    assert len(empty) == 32 and m.proof_blob_info(empty)["count"] == 0 and m.proofs_from_bytes(empty) == []
    assert empty == b"HBPC" + struct.pack("<HHIIIIQ", 1, 0, 64, 1, 0, 0, 0)


def _structs(m, proofs, n, keep):
    arr = (m.RangeProofC * len(proofs))()
    for i, pr in enumerate(proofs):
        arr[i] = m._range_proof_struct(pr, n, keep)
    return arr


def test_error_paths(m, blobs):
    n, arrs, f, blob = blobs["rpverify_n16"]
    L = m.lib()
    proofs = cr.to_dicts(arrs)
    keep = []
    arr = _structs(m, proofs, n, keep)
    cap = L.hipbp_proof_blob_bound(len(proofs), 1, 4, 1)
    out = np.full(cap, 0xEE, np.uint8)
    nb = ctypes.c_size_t(7)
    enc = lambda a, c: L.hipbp_proofs_encode_host(a, ctypes.c_size_t(len(proofs)), ctypes.c_size_t(n), 1, m._p(out),
                                                  ctypes.c_size_t(c), ctypes.byref(nb))
    # a cap below the bound: HIPBP_ERR_ARG, nothing written
    assert enc(arr, cap - 1) == 1 and b"cap" in L.hipbp_last_error() and (out == 0xEE).all() and nb.value == 7
    # a proof of another shape / with inconsistent lengths: its index, nothing written
    arr[5].ip_proof.L_len = 3
    assert enc(arr, cap) == 1 and b"proof 5" in L.hipbp_last_error() and (out == 0xEE).all()
    arr[5].ip_proof.L_len = 4
    arr[9].ip_proof.b.length = 2
    assert enc(arr, cap) == 1 and b"proof 9" in L.hipbp_last_error() and (out == 0xEE).all()
    arr[9].ip_proof.b.length = 1
    assert enc(arr, cap) == 0 and bytes(out[:nb.value]) == blob
    # the decoder: a malformed blob leaves nothing allocated and zeroed structs
    back = (m.RangeProofC * len(proofs))()
    good = np.frombuffer(blob, np.uint8)
    for bad in (good[:-1], np.concatenate([good, good[:1]])):
        assert L.hipbp_proofs_decode_host(m._p(np.ascontiguousarray(bad)), ctypes.c_size_t(len(bad)), back) == 1
        assert bytes(back) == bytes(ctypes.sizeof(back))
    flip = good.copy()
    flip[32 + 3] = 2
    assert L.hipbp_proofs_decode_host(m._p(flip), ctypes.c_size_t(len(flip)), back) == 1
    assert b"kind" in L.hipbp_last_error() and bytes(back) == bytes(ctypes.sizeof(back))
    with pytest.raises(m.BulletproofError):
        m.proof_blob_info(b"HBPD" + blob[4:])
    # the header check alone, for a blob that lives in device memory
    ic = m.ProofBlobInfoC()
    assert L.hipbp_proof_blob_header(m._p(good[:32].copy()), ctypes.c_size_t(len(good)), ctypes.byref(ic)) == 0
    assert (ic.count, ic.raw_count, ic.bytes) == (28, KAT["rpverify_n16"]["raw_count"], len(good))
    assert L.hipbp_proof_blob_header(m._p(good[:32].copy()), ctypes.c_size_t(len(good) + 8), ctypes.byref(ic)) == 1


def test_host_codec_needs_no_gpu(blobs):
    """One child process with every device hidden: encode, parse and decode on the CPU."""
    n, arrs, f, blob = blobs["proofs_n64"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    py = ("import sys, hashlib\n"
          "sys.path.insert(0, 'tests')\n"
          "import codec_ref as cr, cudabulletproof_amd as bp\n"
          "n, arrs, _ = cr.golden_set('proofs_n64')\n"
          "assert bp.lib().hipbp_device_count() == 0\n"
          "blob = bp.proofs_to_bytes(cr.to_dicts(arrs), n)\n"
          "back = cr.from_dicts(bp.proofs_from_bytes(blob), False)\n"
          "assert cr.same(arrs, back, list(back))\n"
          "print('DIGEST', bp.proof_blob_info(blob)['count'], hashlib.sha256(blob).hexdigest())\n")
    r = subprocess.run([sys.executable, "-c", py], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert f"DIGEST 6 {KAT['proofs_n64']['sha256']}" in r.stdout, (r.stdout, r.stderr)


# ---------------------------------------------------------------- layout, lane bodies, malformed blobs
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


def _build(exe, opt, extra=()):
    subprocess.run(["hipcc", opt, "-std=c++17", "--cuda-host-only", "-x", "hip", SRC, "-o", str(exe)] + list(extra),
                   check=True, capture_output=True)
    return str(exe)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checks, fails = (int(x) for x in r.stdout.split("\n")[-2].split())
    # 60 shapes x ~10 layout checks, 42 round trips with a check per kind byte and per slice, 2 x 27 malformed blobs
    assert fails == 0 and checks >= 6000, r.stdout[-3000:]
    return r


@needs_hipcc
def test_codec_check(tmp_path):
    _run(_build(tmp_path / "cc", "-O2"))


@needs_hipcc
def test_codec_check_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "cc_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]

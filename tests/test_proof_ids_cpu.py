"""Proof ids and the batch Merkle root, the parts that need no GPU:

* tests/golden/proof_id_kat.json: the contract's published answers (ids of a compact and of a raw
  proof, with and without taux and mu; roots for six counts) and the golden sets' digests, against the
  Python restatement (tests/proof_id_ref.py) and the library's host entry points;
* hipbp_proof_ids_host against the restatement on the four golden sets (mixes of compact and raw),
  f = 0 and 1, an ab_len = 2 batch and an empty one; ids from a host blob equal ids from the structs;
* the root against RFC 6962's recursive form for every count 0..70 and 257; for every count 1..33 and
  every index the audit path and its check, and what the check must reject;
* the error paths; the host calls in a process that sees no device;
* every lane body of bp_ids.h on the CPU against a byte-at-a-time SHA-256 (tests/ids_check.hip, a
  stand-alone host program), at -O2 and under ASan + UBSan."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import codec_ref as cr
import proof_id_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ids_check.hip")
KAT = json.load(open(os.path.join(cr.GOLDEN, "proof_id_kat.json")))
SETS = ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64")
P1 = np.array([0xFFFFFFFFFFFFFFEE, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF], np.uint64)   # p + 1


@pytest.fixture(scope="module")
def m():
    import cudabulletproof_amd as mod
    mod.build()
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def refs(oracle):
    """(name, f) -> (n, arrs, the restatement's ids, its kinds), computed once."""
    out = {}
    for name in SETS:
        n, arrs, _ = cr.golden_set(name)
        for f in (0, 1):
            out[name, f] = (n, arrs) + pr.proof_ids(oracle, arrs, n, bool(f))
    return out


def _given_inputs():
    n, arrs, _ = cr.golden_set("proofs_n16")
    bad = cr.take(arrs, np.arange(1))
    bad["L"][0, 0, 8:12] = P1
    return {"untouched": (n, cr.take(arrs, np.arange(1))), "tampered": (n, bad)}


# ---------------------------------------------------------------- known answers
def test_kat_fixture_is_the_published_one():
    g = KAT["given"]
    assert [(e["input"], e["f"], e["kind"], e["message_bytes"]) for e in g["ids"]] == \
        [("tampered", 0, 1, 1856), ("tampered", 1, 1, 1920), ("untouched", 0, 0, 928), ("untouched", 1, 0, 992)]
    assert g["ids"][0]["id"] == "0f3dcc00ccb2c199ec18cf51c5aa37fc6de2c033011333ccfea34b081c620cc5"
    assert g["ids"][1]["id"] == "6d8e66387263c1519f5d90aed74b9d949b42d45794e2c452c275222e450b6b48"
    assert g["ids"][2]["id"] == "9d501615fe5ff36e1631f9996c64495d8504c749102da447723ded4c74870029"
    assert g["ids"][3]["id"] == "8e78a6bf2ef9cf0fa3d514614a7325f42898ca395b560865e1f20912d35148ea"
    assert sorted(g["roots"], key=int) == ["0", "1", "2", "3", "7", "257"]
    assert g["roots"]["0"] == hashlib.sha256(b"").hexdigest()
    assert g["roots"]["257"] == "feadb4c7b1a3395932e3231e618af5d0552ce76f321fd1f78c149efb8cec1053"
    assert sorted(KAT["sets"]) == sorted(f"{s}_f{f}" for s in SETS for f in (0, 1))


def test_restatement_gives_the_published_ids(oracle):
    inputs = _given_inputs()
    for e in KAT["given"]["ids"]:
        n, arrs = inputs[e["input"]]
        kind, msg = pr.message(oracle, arrs, n, 0, bool(e["f"]))
        assert (kind, len(msg)) == (e["kind"], e["message_bytes"])
        assert hashlib.sha256(msg).hexdigest() == e["id"]


def test_library_gives_the_published_ids(m):
    inputs = _given_inputs()
    for e in KAT["given"]["ids"]:
        n, arrs = inputs[e["input"]]
        assert m.proof_ids_host(cr.to_dicts(arrs), n, bool(e["f"]))[0].hex() == e["id"]
        blob = m.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=bool(e["f"]))
        assert m.proof_blob_info(blob)["raw_count"] == e["kind"]
        assert m.blob_proof_ids_host(blob)[0].hex() == e["id"]


@pytest.mark.parametrize("count", [0, 1, 2, 3, 7, 257])
def test_published_roots(m, count):
    ids = pr.kat_ids(count)
    want = KAT["given"]["roots"][str(count)]
    assert pr.mth(ids).hex() == want
    assert m.merkle_root_host(ids).hex() == want


def test_certificate_transparency_vector():
    """The recursive restatement on the Certificate Transparency test suite's 8 leaves."""
    leaves = [bytes.fromhex(h) for h in ("", "00", "10", "2021", "3031", "40414243", "5051525354555657",
                                         "606162636465666768696a6b6c6d6e6f")]
    assert pr.mth(leaves).hex() == "5dc9da79a70659a9ad559cb701ded9a2ab9d823aad2f4960cfe370eff4604328"


# ---------------------------------------------------------------- ids
@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_host_ids_equal_restatement_and_kat(m, refs, name, f):
    n, arrs, ids, kinds = refs[name, f]
    k = KAT["sets"][f"{name}_f{f}"]
    assert (k["count"], k["raw_count"]) == (len(ids), sum(kinds))
    assert hashlib.sha256(b"".join(ids)).hexdigest() == k["ids_sha256"] and pr.mth(ids).hex() == k["root"]
    got = m.proof_ids_host(cr.to_dicts(arrs), n, bool(f))
    assert got == ids
    assert m.merkle_root_host(got).hex() == k["root"]
    if name.startswith("rpverify"):
        assert 0 < sum(kinds) < len(kinds)   # both kinds
    # (the rpverify sets repeat proofs under other V arguments: equal records, equal ids)
    if name.startswith("proofs"):
        assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_blob_ids_equal_struct_ids(m, refs, name, f):
    n, arrs, ids, kinds = refs[name, f]
    blob = m.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=bool(f))
    assert list(np.frombuffer(blob[32:32 + len(ids)], np.uint8)) == kinds
    assert m.blob_proof_ids_host(blob) == ids
    assert m.blob_proof_ids_host(np.frombuffer(blob, np.uint8)) == ids


def test_f_and_kind_are_hashed(refs):
    a, b = refs["rpverify_n16", 0], refs["rpverify_n16", 1]
    assert a[3] == b[3] and all(x != y for x, y in zip(a[2], b[2]))


def test_ab_len_two_and_empty(m, oracle):
    n, arrs, _ = cr.golden_set("proofs_n16")
    two = dict(arrs)
    two["a"] = np.concatenate([arrs["a"], arrs["a"] + np.uint64(1)], axis=1)
    two["b"] = np.concatenate([arrs["b"], arrs["b"] + np.uint64(2)], axis=1)
    for f in (False, True):
        ids, kinds = pr.proof_ids(oracle, two, n, f)
        assert kinds == [1] * 6
        assert m.proof_ids_host(cr.to_dicts(two), n, f) == ids
        assert m.blob_proof_ids_host(m.proofs_to_bytes(cr.to_dicts(two), n, with_blinding=f)) == ids
    assert m.proof_ids_host([], 64) == [] and m.blob_proof_ids_host(m.proofs_to_bytes([], 64)) == []
    assert m.merkle_root_host([]) == hashlib.sha256(b"").digest()


def test_host_threads_give_the_same_ids(m, oracle, monkeypatch):
    """600 proofs (both kinds) are split over three threads by default (256 proofs a thread at least);
    HIPBP_HOST_THREADS = 1 and = 7 (capped at three here) give the same ids, the restatement's."""
    _, a, _ = cr.golden_set("proofs_n16")
    _, b, _ = cr.golden_set("rpverify_n16")
    arrs = {k: np.concatenate([a[k], b[k]]) for k in a}
    arrs = cr.take(arrs, np.arange(600) % len(arrs["V"]))
    arrs["x"][:, 0] += np.arange(600, dtype=np.uint64)   # (600 different records, the kinds unchanged)
    want, kinds = pr.proof_ids(oracle, arrs, 16, True)
    assert len(set(want)) == 600 and 0 < sum(kinds) < 600
    proofs = cr.to_dicts(arrs)
    blob = m.proofs_to_bytes(proofs, 16, with_blinding=True)
    for threads in (None, "1", "7"):
        if threads:
            monkeypatch.setenv("HIPBP_HOST_THREADS", threads)
        assert m.proof_ids_host(proofs, 16, True) == want
        assert m.blob_proof_ids_host(blob) == want


# ---------------------------------------------------------------- the tree
IDS80 = pr.kat_ids(80)


@pytest.mark.parametrize("count", list(range(0, 71)) + [257])
def test_root_equals_recursive_form(m, count):
    ids = IDS80[:count] if count <= 80 else pr.kat_ids(count)
    assert m.merkle_root_host(ids) == pr.mth(ids)
    assert m.merkle_root_host(pr.ids_array(ids)) == pr.mth(ids)   # the array form of the argument


@pytest.mark.parametrize("count", range(1, 34))
def test_paths_and_their_check(m, count):
    ids = IDS80[:count]
    root = pr.mth(ids)
    for i in range(count):
        want = pr.path(i, ids)
        got = m.merkle_path(ids, i)
        assert got == want, (count, i)
        assert len(got) <= 22
        assert m.merkle_verify(ids[i], i, count, got, root)
        for j in range(count):   # any other index
            if j != i:
                assert not m.merkle_verify(ids[i], j, count, got, root), (count, i, j)
        assert not m.merkle_verify(ids[i], count, count, got, root)
        for k in range(len(got)):   # a flipped bit in any entry
            bad = list(got)
            bad[k] = bytes([bad[k][0] ^ 0x80]) + bad[k][1:]
            assert not m.merkle_verify(ids[i], i, count, bad, root)
            bad[k] = got[k][:31] + bytes([got[k][31] ^ 1])
            assert not m.merkle_verify(ids[i], i, count, bad, root)
        if got:
            assert not m.merkle_verify(ids[i], i, count, got[:-1], root)   # one short
        assert not m.merkle_verify(ids[i], i, count, got + [got[-1] if got else root], root)   # one long
        assert not m.merkle_verify(ids[(i + 1) % count], i, count, got, root) or count == 1
        assert not m.merkle_verify(ids[i], i, count, got, ids[i])   # another root


# ---------------------------------------------------------------- errors
def _structs(m, proofs, n, keep):
    arr = (m.RangeProofC * len(proofs))()
    for i, pr_ in enumerate(proofs):
        arr[i] = m._range_proof_struct(pr_, n, keep)
    return arr


def test_error_paths(m, refs):
    n, arrs, ids, _ = refs["rpverify_n16", 1]
    L = m.lib()
    proofs = cr.to_dicts(arrs)
    keep = []
    arr = _structs(m, proofs, n, keep)
    out = np.full(32 * len(proofs), 0xEE, np.uint8)
    call = lambda: L.hipbp_proof_ids_host(arr, ctypes.c_size_t(len(proofs)), ctypes.c_size_t(n), 1, m._p(out))
    arr[5].ip_proof.L_len = 3
    assert call() == 1 and b"proof 5" in L.hipbp_last_error() and (out == 0xEE).all()
    arr[5].ip_proof.L_len = 4
    arr[9].ip_proof.b.length = 2
    assert call() == 1 and b"proof 9" in L.hipbp_last_error() and (out == 0xEE).all()
    arr[9].ip_proof.b.length = 1
    assert L.hipbp_proof_ids_host(arr, ctypes.c_size_t(len(proofs)), ctypes.c_size_t(24), 1, m._p(out)) == 1   # n not a power of two
    assert (out == 0xEE).all()
    assert L.hipbp_proof_ids_host(None, ctypes.c_size_t(3), ctypes.c_size_t(n), 1, m._p(out)) == 1 and (out == 0xEE).all()
    assert call() == 0 and out.tobytes() == b"".join(ids)
    # a malformed blob: the parser's message, nothing written
    blob = np.frombuffer(m.proofs_to_bytes(proofs, n, with_blinding=True), np.uint8)
    out[:] = 0xEE
    for bad in (blob[:-1], np.concatenate([blob, blob[:1]])):
        bad = np.ascontiguousarray(bad)
        assert L.hipbp_blob_proof_ids_host(m._p(bad), ctypes.c_size_t(len(bad)), m._p(out)) == 1 and (out == 0xEE).all()
    flip = blob.copy()
    flip[32 + 3] = 2
    assert L.hipbp_blob_proof_ids_host(m._p(flip), ctypes.c_size_t(len(flip)), m._p(out)) == 1
    assert b"kind" in L.hipbp_last_error() and (out == 0xEE).all()
    with pytest.raises(m.BulletproofError):
        m.blob_proof_ids_host(b"HBPD" + blob.tobytes()[4:])
    # a flipped byte inside a record: a well-formed blob of other proofs, another id for that proof alone
    info = m.proof_blob_info(blob)
    flip = blob.copy()
    i0 = list(blob[32:32 + len(ids)]).index(0)                 # the first compact proof
    flip[32 + cr.pad8(len(ids)) + i0 * cr.sizes(1, 4, 1)[0] + 100] ^= 1   # inside its slot
    assert m.proof_blob_info(flip) == info
    other = m.blob_proof_ids_host(flip)
    assert other[i0] != ids[i0] and other[:i0] == ids[:i0] and other[i0 + 1:] == ids[i0 + 1:]
    # the tree's limits and nulls
    root = np.full(32, 0xEE, np.uint8)
    a = pr.ids_array(ids)
    assert L.hipbp_merkle_root_host(m._p(a), ctypes.c_size_t((1 << 24) + 1), m._p(root)) == 1 and b"2^24" in L.hipbp_last_error()
    assert L.hipbp_merkle_root_host(None, ctypes.c_size_t(2), m._p(root)) == 1 and (root == 0xEE).all()
    path = np.full(32 * 22, 0xEE, np.uint8)
    ln = ctypes.c_size_t(77)
    assert L.hipbp_merkle_path_host(m._p(a), ctypes.c_size_t(len(ids)), ctypes.c_size_t(len(ids)), m._p(path), ctypes.byref(ln)) == 1
    assert b"index" in L.hipbp_last_error() and ln.value == 77 and (path == 0xEE).all()
    with pytest.raises(m.BulletproofError):
        m.merkle_path(ids, len(ids))
    with pytest.raises(ValueError):
        m.merkle_root_host([b"short"])


def test_host_calls_need_no_gpu():
    """One child process with every device hidden: ids from structs and from a blob, root, path, check."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    py = ("import sys, hashlib\n"
          "sys.path.insert(0, 'tests')\n"
          "import codec_ref as cr, cudabulletproof_amd as bp\n"
          "n, arrs, _ = cr.golden_set('rpverify_n64')\n"
          "assert bp.lib().hipbp_device_count() == 0\n"
          "ids = bp.proof_ids_host(cr.to_dicts(arrs), n, True)\n"
          "assert bp.blob_proof_ids_host(bp.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=True)) == ids\n"
          "root = bp.merkle_root_host(ids)\n"
          "assert bp.merkle_verify(ids[5], 5, len(ids), bp.merkle_path(ids, 5), root)\n"
          "print('DIGEST', len(ids), hashlib.sha256(b''.join(ids)).hexdigest(), root.hex())\n")
    r = subprocess.run([sys.executable, "-c", py], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    k = KAT["sets"]["rpverify_n64_f1"]
    assert f"DIGEST 16 {k['ids_sha256']} {k['root']}" in r.stdout, (r.stdout, r.stderr)


# ---------------------------------------------------------------- the lane bodies on the CPU
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
    # 12 message shapes, 31 batches with four checks per proof, 40 trees with seven per leaf, 2 x 19 malformed blobs of 21 proofs
    assert fails == 0 and checks >= 8000, r.stdout[-3000:]
    return r


@needs_hipcc
def test_ids_check(tmp_path):
    _run(_build(tmp_path / "ic", "-O2"))


@needs_hipcc
def test_ids_check_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "ic_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]

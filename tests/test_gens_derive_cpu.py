"""Generators derived from seeds, the parts that need no GPU.  Everything is bit-exact;
the expected value is always hashlib for X and Y and the CPU restatement's fe_mul for T
(tests/gens_derive_ref.py):

* the reference-emitted G, H, g, h of the golden proof sets (all 16 limbs) from the reference's seeds;
* random, all-0xFF and all-zero seeds; blocks across every byte carry of the big-endian index; the
  last block below 2^32; a block cut into two calls;
* the single form on a seed whose digest has bit 255 set: T is the product X * 1, not X;
* the 2^20-point MSM's points (seed byte 5), first and last 64 rows;
* the error paths and count = 0, with sentinel bytes; the host calls in a process that sees no device;
* tests/golden/gens_derive_kat.json, the published answers, against the restatement and the library;
* both lane bodies on the CPU against a byte-at-a-time SHA-256 (tests/gens_derive_check.hip, a
  stand-alone host program), at -O2 and under ASan + UBSan;
* the kernels' resources: no scratch and no spilled VGPR."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gens_derive_ref as gr

ROOT = gr.ROOT
SRC = os.path.join(ROOT, "tests", "gens_derive_check.hip")
KAT = json.load(open(gr.KAT_PATH))


@pytest.fixture(scope="module")
def m():
    import cudabulletproof_amd as mod
    mod.build()
    mod.lib()
    return mod


# ---------------------------------------------------------------- the reference's own generators
@pytest.mark.parametrize("name,n", [("proofs_n16", 16), ("proofs_n64", 64)])
def test_reference_anchor(m, golden, name, n):
    d = golden(name)
    assert d["G"].shape == (n, 16) and d["H"].shape == (n, 16)
    assert np.array_equal(m.derive_base_points_host(1, n), d["G"])
    assert np.array_equal(m.derive_base_points_host(2, n), d["H"])
    assert np.array_equal(m.derive_single_point_host(3), d["g"])
    assert np.array_equal(m.derive_single_point_host(4), d["h"])
    assert m.REFERENCE_SEEDS == {k: bytes([b]) + bytes(31) for k, b in (("G", 1), ("H", 2), ("g", 3), ("h", 4))}
    # the int form of a seed is that byte and 31 zeros
    assert np.array_equal(m.derive_base_points_host(m.REFERENCE_SEEDS["G"], n), d["G"])


def test_restatement_gives_the_reference_generators(oracle, golden):
    d = golden("proofs_n16")
    assert np.array_equal(gr.base_points(oracle, 1, 16), d["G"]) and np.array_equal(gr.base_points(oracle, 2, 16), d["H"])
    assert np.array_equal(gr.single_point(oracle, 3), d["g"]) and np.array_equal(gr.single_point(oracle, 4), d["h"])


# ---------------------------------------------------------------- seeds and index blocks
def _seeds():
    rng = np.random.default_rng(19)
    return [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)] + [b"\xff" * 32, bytes(32)]


@pytest.mark.parametrize("first,count", [(0, 70)] + gr.CARRIES + [gr.LAST_BLOCK])
def test_seeds_and_index_carries(m, oracle, first, count):
    for seed in _seeds():
        got = m.derive_base_points_host(seed, count, first)
        assert got.dtype == np.uint64 and got.shape == (count, 16)
        assert np.array_equal(got, gr.base_points(oracle, seed, count, first)), (seed.hex(), first)
        assert np.array_equal(m.derive_single_point_host(seed), gr.single_point(oracle, seed)), seed.hex()


def test_a_block_cut_into_two_calls(m, oracle):
    seed = _seeds()[0]
    whole = m.derive_base_points_host(seed, 1000)
    assert np.array_equal(whole, gr.base_points(oracle, seed, 1000))
    assert np.array_equal(np.concatenate([m.derive_base_points_host(seed, 300), m.derive_base_points_host(seed, 700, 300)]), whole)


def test_single_form_takes_the_product(m, oracle):
    """X of the seed 01 00..00 has bit 255 set, and X * 1 != X in the reference's arithmetic."""
    p = m.derive_single_point_host(gr.BIT255_SEED)
    X = p[0:4]
    one = np.array([1, 0, 0, 0], np.uint64)
    assert int(X[3]) >> 63 == 1
    assert np.array_equal(p[4:8], one) and np.array_equal(p[8:12], one)
    assert np.array_equal(p[12:16], oracle.fe_mul(X, one))
    assert not np.array_equal(p[12:16], X)
    assert np.array_equal(p, gr.single_point(oracle, gr.BIT255_SEED))


@pytest.mark.parametrize("lo", [0, 2**20 - 64])
def test_msm_points(m, oracle, lo):
    from cudabulletproof_amd import synth
    want = synth.base_points_xy(64, 5, lo)
    for k in range(64):
        want[k, 12:16] = oracle.fe_mul(want[k, 0:4], want[k, 4:8])
    assert np.array_equal(m.derive_base_points_host(5, 64, lo), want)


# ---------------------------------------------------------------- errors and the empty call
def test_errors_and_zero_count(m):
    L = m.lib()
    seed = m._gen_seed(7)
    u64, sz = ctypes.c_uint64, ctypes.c_size_t
    out = np.full((4, 16), 0xEEEEEEEEEEEEEEEE, np.uint64)
    clean = lambda: (out == 0xEEEEEEEEEEEEEEEE).all()
    assert L.hipbp_derive_base_points_host(None, seed, u64(0), sz(2)) == 1
    assert L.hipbp_derive_base_points_host(m._p(out), None, u64(0), sz(2)) == 1 and clean()
    assert L.hipbp_derive_single_point_host(None, seed) == 1
    assert L.hipbp_derive_single_point_host(m._p(out), None) == 1 and clean()
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(2**32), sz(1)) == 1 and clean()
    assert b"2^32" in L.hipbp_last_error()
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(2**32 - 1), sz(2)) == 1 and clean()
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(2**64 - 1), sz(2)) == 1 and clean()
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(5), sz(0)) == 0 and clean()
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(2**32), sz(0)) == 0 and clean()
    # the device entry points check their arguments before anything else: no device is needed to be refused
    assert L.hipbp_derive_base_points(None, seed, u64(0), sz(2), None) == 1
    assert L.hipbp_derive_base_points(m._p(out), None, u64(0), sz(2), None) == 1
    assert L.hipbp_derive_base_points(m._p(out), seed, u64(2**32 - 1), sz(2), None) == 1
    assert L.hipbp_derive_single_point(m._p(out), None, None) == 1 and clean()
    with pytest.raises(m.BulletproofError):
        m.derive_base_points_host(7, 2, 2**32 - 1)
    with pytest.raises(m.BulletproofError):
        m.derive_single_point_host(None)
    for bad in (b"short", 256, -1):
        with pytest.raises(ValueError):
            m.derive_single_point_host(bad)
    assert m.derive_base_points_host(7, 0).shape == (0, 16)
    # the last index itself is fine
    assert L.hipbp_derive_base_points_host(m._p(out), seed, u64(2**32 - 1), sz(1)) == 0 and not clean()


def test_host_calls_need_no_gpu():
    """One child process with every device hidden: the same bytes."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    py = ("import sys\n"
          "sys.path.insert(0, 'tests')\n"
          "import numpy as np, gens_derive_ref as gr, cudabulletproof_amd as bp\n"
          "assert bp.lib().hipbp_device_count() == 0\n"
          "for v in gr.KAT_VECTORS:\n"
          "    print('VEC', gr.digest(bp.derive_base_points_host(v[0], v[2], v[1])))\n"
          "for s in gr.KAT_SINGLES:\n"
          "    print('ONE', gr.digest(bp.derive_single_point_host(s)))\n")
    r = subprocess.run([sys.executable, "-c", py], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert [l.split()[1] for l in r.stdout.splitlines() if l.startswith("VEC")] == [e["sha256"] for e in KAT["vectors"]]
    assert [l.split()[1] for l in r.stdout.splitlines() if l.startswith("ONE")] == [e["sha256"] for e in KAT["singles"]]


# ---------------------------------------------------------------- the published answers
def test_kat_fixture_is_the_restatements(oracle):
    assert gr.make_kat(oracle) == KAT
    assert len(KAT["vectors"]) == 6 and len(KAT["singles"]) == 4


def test_library_gives_the_published_answers(m):
    for e in KAT["vectors"]:
        got = m.derive_base_points_host(bytes.fromhex(e["seed"]), e["count"], e["first"])
        assert gr.digest(got) == e["sha256"], e
    for e in KAT["singles"]:
        assert gr.digest(m.derive_single_point_host(bytes.fromhex(e["seed"]))) == e["sha256"], e


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
    # 15 seeds, 102 indices with four checks each and the single form's three
    assert fails == 0 and checks >= 6000, r.stdout[-3000:]
    return r


@needs_hipcc
def test_gens_derive_check(tmp_path):
    _run(_build(tmp_path / "gd", "-O2"))


@needs_hipcc
def test_gens_derive_check_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "gd_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---------------------------------------------------------------- the kernels' resources
@needs_hipcc
def test_kernels_use_no_scratch(m, tmp_path):
    """bp_gens_derive.hip compiled for gfx950 with the library's flags: every kernel in it reports
    ScratchSize 0 and no spilled VGPR (the hash states and blocks stay in registers), and no LDS."""
    src = os.path.join(m.CSRC, "bp_gens_derive.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "gd.o")],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 2 and any("k_derive_base_points" in s for s in names) and \
        any("k_derive_single_point" in s for s in names), names
    for key in (r"ScratchSize \[bytes/lane\]", "VGPRs Spill", "SGPRs Spill", r"LDS Size \[bytes/block\]"):
        vals = re.findall(key + r": (\d+)", r.stderr)
        assert len(vals) == 2 and all(int(v) == 0 for v in vals), (key, vals)

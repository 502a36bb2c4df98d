"""Batched Pedersen commitments, the parts that need no GPU:

* every reference-emitted row of tests/golden/commit.npz (the reference's compiled pedersen_commit on
  the 8 x 11 edge cross, on a Z = 1 and a Z != 1 (g, h) pair) equals the C restatement composed from
  fe_tobytes, ge_scalarmult, ge_normalize_host and ge_add: the composition the GPU tests compare with;
* the same composition gives the 6 + 6 V the reference's prover emitted (proofs_n16 / proofs_n64);
* no expected point is the absorbing (0, 0, 1, 0);
* the commit workspace's table, the chunking rule and k_commit_terms' lane layout, run on the CPU by
  tests/commit_layout_check.hip, a stand-alone host program, at -O2 and under ASan + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import commit_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "commit_layout_check.hip")
P = 2**255 - 19


def _int(limbs):
    return sum(int(x) << (64 * i) for i, x in enumerate(limbs))


def test_fixture_shape(golden):
    d = golden("commit")
    assert os.path.getsize(os.path.join(cr.GOLDEN, "commit.npz")) <= 40 * 1024
    assert d["out"].shape == (176, 16) and d["v"].shape == (176, 4) and d["gamma"].shape == (176, 4)
    assert d["g"].shape == (2, 16) and d["h"].shape == (2, 16) and list(d["pair"]) == [0] * 88 + [1] * 88
    edges = [0, 1, 2**64 - 1, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1]
    for k in (0, 1):   # the full cross, v-major: 8 values x (the same 8 + 3 masked random blindings)
        v, gam = d["v"][88 * k:88 * k + 88], d["gamma"][88 * k:88 * k + 88]
        assert [_int(x) for x in v[::11]] == edges and all(np.array_equal(v[i], v[i - i % 11]) for i in range(88))
        assert [_int(x) for x in gam[:8]] == edges and all(np.array_equal(gam[i], gam[i % 11]) for i in range(88))
        for x in gam[8:11]:
            b = _int(x).to_bytes(32, "little")
            assert b[31] & 0xC0 == 0x40 and b[0] & 7 == 0
    # pair 0 has Z = 1; pair 1 Z limbs that are not 1 (g's are p + 1, h's a general Z) and never 0 or p
    one = [1, 0, 0, 0]
    assert list(d["g"][0][8:12]) == one and list(d["h"][0][8:12]) == one
    for pt in (d["g"][1], d["h"][1]):
        assert _int(pt[8:12]) not in (0, 1, P)
    assert _int(d["h"][1][8:12]) % P != 1


def test_reference_rows_equal_restatement(golden, oracle):
    d = golden("commit")
    for i in range(len(d["out"])):
        k = int(d["pair"][i])
        got = cr.restate(oracle, d["v"][i], d["gamma"][i], d["g"][k], d["h"][k])
        assert np.array_equal(got, d["out"][i]), i
        assert not np.array_equal(d["out"][i], cr.ABSORBING), i


@pytest.mark.parametrize("n", [16, 64])
def test_restatement_gives_the_reference_provers_V(oracle, n):
    v, gamma, g, h, V = cr.fixture_v_rows(n)
    assert len(V) == 6
    got = cr.restate_many(oracle, v, gamma, g, h)
    assert np.array_equal(got, V)
    assert not any(np.array_equal(x, cr.ABSORBING) for x in V)


# ---------------------------------------------------------------- workspace table, chunks, lane layout
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
    # 8 table checks, 4 + 25 chunk rules and their chunks, 12 counts x (3 checks per lane + 1 per item)
    assert fails == 0 and checks >= 5000, r.stdout[-3000:]
    return r


@needs_hipcc
def test_commit_layout(tmp_path):
    _run(_build(tmp_path / "cl", "-O2"))


@needs_hipcc
def test_commit_layout_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "cl_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]

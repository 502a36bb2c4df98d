"""The seeded prover's derivation (csrc/bp_prove_seed.h, __host__ __device__) compiled as HOST code
(tests/prove_seed_check.hip) and compared with its hashlib restatement (tests/prove_seed_ref.py) and
the committed known answers (tests/golden/prove_seed_kat.json).  The device pass of the same
layouts is checked by tests/test_prove_seeded.py (-m gpu)."""
import json
import os
import shutil
import subprocess

import pytest

import prove_seed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("psc") / "psc"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--cuda-host-only", "-x", "hip",
                    os.path.join(ROOT, "tests", "prove_seed_check.hip"), "-o", str(out)], check=True,
                   capture_output=True)
    return str(out)


def run(exe, cases):
    """cases: (seed bytes, v limbs, gamma limbs, index, n, slots or "all") -> [(key hex, {slot: limbs})]."""
    args = []
    for seed, v, gamma, index, n, slots in cases:
        sl = slots if slots == "all" else ",".join(str(s) for s in slots)
        args.append(":".join([bytes(seed).hex(), ref.limb_bytes(v).hex(), ref.limb_bytes(gamma).hex(), str(index),
                              str(n), sl]))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "key":
            res.append((f[1], {}))
        else:
            res[-1][1][int(f[1])] = tuple(int(x, 16) for x in f[2:6])
    assert len(res) == len(cases)
    return res


def check(exe, cases):
    for (seed, v, gamma, index, n, slots), (khex, got) in zip(cases, run(exe, cases)):
        k = ref.key(seed, v, gamma, index, n)
        assert khex == k.hex(), (index, n)
        want = range(2 * n + 4) if slots == "all" else slots
        assert sorted(got) == sorted(want)
        for s in want:
            assert got[s] == ref.scalar(k, s), (index, n, s)


def test_known_answers(exe):
    """The issue's known answers: the host pass, the hashlib restatement and the committed file agree."""
    with open(os.path.join(ROOT, "tests", "golden", "prove_seed_kat.json")) as f:
        kat = json.load(f)
    seed = bytes.fromhex(kat["seed"])
    assert seed == bytes(range(32))
    cases = [(seed, kat["v"], kat["gamma"], c["index"], kat["n"], sorted(int(s) for s in c["slots"]))
             for c in kat["cases"]]
    for c, (khex, got) in zip(kat["cases"], run(exe, cases)):
        assert khex == c["key"] == ref.key(seed, kat["v"], kat["gamma"], c["index"], kat["n"]).hex()
        for s, limbs in c["slots"].items():
            want = tuple(int(x, 16) for x in limbs)
            assert got[int(s)] == want == ref.scalar(bytes.fromhex(khex), int(s)), (c["index"], s)


@pytest.mark.parametrize("n", [1, 8, 128])
def test_sizes_indices_and_seeds(exe, n):
    """n in {1, 8, 128} x index in {0, 2^32 - 1, 2^32, 2^64 - 1} x the all-zero / all-0xFF / a mixed seed;
    v and gamma with every limb in use (raw limbs at and above p: nothing is canonicalised)."""
    v = [0xFFFFFFFFFFFFFFED, ref.M64, ref.M64, ref.M64]
    gamma = [0x0123456789ABCDEF, 0x8000000000000000, 1, 0xFEDCBA9876543210]
    slots = sorted({0, 3, 4, 4 + n - 1, 4 + n, 2 * n + 3})   # the ends of rnd, sL and sR
    cases = [(seed, v, gamma, index, n, slots)
             for seed in (bytes(32), b"\xff" * 32, bytes(range(7, 39)))
             for index in (0, 2**32 - 1, 2**32, 2**64 - 1)]
    check(exe, cases)


def test_every_slot_and_masks(exe):
    """Every slot of one proof at n = 8 equals hashlib, and generate_random_scalar's masks hold on all
    of them: low three bits clear, bit 255 clear, bit 254 set."""
    case = (bytes(range(100, 132)), [200, 0, 0, 0], [5, 6, 7, 8], 77, 8, "all")
    check(exe, [case])
    (_, got), = run(exe, [case])
    assert sorted(got) == list(range(20))
    assert len(set(got.values())) == 20
    for s, d in got.items():
        assert d[0] & 7 == 0 and d[3] >> 63 == 0 and (d[3] >> 62) & 1 == 1, s

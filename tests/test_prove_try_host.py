"""The accepted prover's retry derivation (csrc/bp_prove_seed.h: seed_try_key, __host__ __device__)
compiled as HOST code (tests/prove_try_check.hip) and compared with its hashlib restatement
(tests/prove_try_ref.py) and the committed known answers (tests/golden/prove_try_kat.json).  The
device pass of the same layout is checked by tests/test_prove_accepted.py (-m gpu)."""
import json
import os
import shutil
import subprocess

import pytest

import prove_seed_ref as ref
import prove_try_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

# DESIGN §14's known answers (seed = bytes 0..31, v = [200,0,0,0], gamma = [5,6,7,8], index 77, n = 8),
# written out here so that the committed file cannot drift from them
KEY_P = "592c76b54299f9fb8922292973579a1b349b718d0290c9f29bcbe01385902818"
TRY_KEYS = {1: "19024586bded058a40df2da63c987716ab9ca962c38cb4dcb3ec5f16cbbae331",
            2: "7df2c4942f495f799ada2db28b5ede37a3546b0cffd8d81c619dbe053a7e9686",
            255: "45f63f60dcd1acd047b6cccd4973ea9485d982f475a17e03bc99ec8847f3c741"}
SLOTS = {(1, 0): "d559e26c33bec638 86128ce4a2de327e f69e7906256a6fb0 7899532839afbdac",
         (1, 19): "d464a464a94b64f0 cadb5ddfd424c8a6 7e78de6ba6604f75 57118f15f03f1ae8",
         (2, 0): "8eefeb251e577700 eac429851d49d611 872b56a8ea8cdb63 756d039246721ffe"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("ptc") / "ptc"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--cuda-host-only", "-x", "hip",
                    os.path.join(ROOT, "tests", "prove_try_check.hip"), "-o", str(out)], check=True,
                   capture_output=True)
    return str(out)


def run(exe, cases):
    """cases: (seed bytes, v limbs, gamma limbs, index, n, a, slots) -> [(key hex, try key hex, {slot: limbs})]."""
    args = [":".join([bytes(seed).hex(), ref.limb_bytes(v).hex(), ref.limb_bytes(gamma).hex(), str(index), str(n), str(a),
                      ",".join(str(s) for s in slots)]) for seed, v, gamma, index, n, a, slots in cases]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "key":
            res.append([f[1], None, {}])
        elif f[0] == "try":
            res[-1][1] = f[1]
        else:
            res[-1][2][int(f[1])] = tuple(int(x, 16) for x in f[2:6])
    assert len(res) == len(cases)
    return res


def test_known_answers(exe):
    """The issue's known answers, the committed file, the host pass and hashlib agree."""
    with open(os.path.join(ROOT, "tests", "golden", "prove_try_kat.json")) as f:
        kat = json.load(f)
    seed = bytes.fromhex(kat["seed"])
    assert seed == bytes(range(32)) and kat["v"] == [200, 0, 0, 0] and kat["gamma"] == [5, 6, 7, 8] and kat["n"] == 8
    by_attempt = {c["attempt"]: c for c in kat["cases"] if c["index"] == 77}
    assert by_attempt[0]["key"] == KEY_P
    for a, k in TRY_KEYS.items():
        assert by_attempt[a]["try_key"] == k, a
    for (a, s), limbs in SLOTS.items():
        assert by_attempt[a]["slots"][str(s)] == limbs.split(), (a, s)
    cases = [(seed, kat["v"], kat["gamma"], c["index"], kat["n"], c["attempt"], sorted(int(s) for s in c["slots"]))
             for c in kat["cases"]]
    for c, (khex, thex, got) in zip(kat["cases"], run(exe, cases)):
        kp = ref.key(seed, kat["v"], kat["gamma"], c["index"], kat["n"])
        assert khex == c["key"] == kp.hex()
        assert thex == c["try_key"] == tref.try_key(kp, c["attempt"]).hex()
        for s, limbs in c["slots"].items():
            want = tuple(int(x, 16) for x in limbs)
            assert got[int(s)] == want == ref.scalar(bytes.fromhex(thex), int(s)), (c["index"], c["attempt"], s)


@pytest.mark.parametrize("n", [1, 8, 128])
def test_attempts_and_sizes(exe, n):
    """a in {0, 1, 2, 255, 2^32 - 1} x n in {1, 8, 128} at the ends of rnd, sL and sR, with every limb of v
    and gamma in use; a = 0 returns key_p itself, every other attempt another key; the masks hold."""
    v = [0xFFFFFFFFFFFFFFED, ref.M64, ref.M64, ref.M64]
    gamma = [0x0123456789ABCDEF, 0x8000000000000000, 1, 0xFEDCBA9876543210]
    seed = bytes(range(7, 39))
    slots = sorted({0, 3, 4, 4 + n - 1, 4 + n, 2 * n + 3})
    attempts = (0, 1, 2, 255, 2**32 - 1)
    cases = [(seed, v, gamma, 2**32 + 5, n, a, slots) for a in attempts]
    keys = set()
    for (_, _, _, index, _, a, _), (khex, thex, got) in zip(cases, run(exe, cases)):
        kp = ref.key(seed, v, gamma, index, n)
        assert khex == kp.hex()
        assert thex == tref.try_key(kp, a).hex(), a
        assert (thex == khex) == (a == 0), a
        keys.add(thex)
        assert sorted(got) == slots
        for s in slots:
            assert got[s] == ref.scalar(bytes.fromhex(thex), s), (a, s)
            d = got[s]
            assert d[0] & 7 == 0 and d[3] >> 63 == 0 and (d[3] >> 62) & 1 == 1, (a, s)
    assert len(keys) == len(attempts)

"""TEST INFRASTRUCTURE shared by tests/test_commit_cpu.py and tests/test_commit_gpu.py: the reference's
pedersen_commit (bulletproof_range_proof.cu:277-296) composed from the C restatement's primitives,
and the inputs of the reference-emitted rows."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABSORBING = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], np.uint64)   # (0, 0, 1, 0)


def restate(oracle, v, gamma, g, h):
    """N(add(N(sm(tobytes(v), g)), N(sm(tobytes(gamma), h)))) for one (v, gamma) of four limbs each."""
    t1 = oracle.ge_normalize_host(oracle.ge_scalarmult(oracle.fe_tobytes(v), g))
    t2 = oracle.ge_normalize_host(oracle.ge_scalarmult(oracle.fe_tobytes(gamma), h))
    return oracle.ge_normalize_host(oracle.ge_add(t1, t2))


def restate_many(oracle, v, gamma, g, h):
    v, gamma = np.asarray(v, np.uint64).reshape(-1, 4), np.asarray(gamma, np.uint64).reshape(-1, 4)
    return np.stack([restate(oracle, a, b, g, h) for a, b in zip(v, gamma)]) if len(v) else np.zeros((0, 16), np.uint64)


def fixture_v_rows(n):
    """The reference prover's own commitments: (v (6,4), gamma (6,4), g, h, V (6,16)) of proofs_n{n}.npz;
    proof p was made with seed p + 1 (make_golden.py), its blinding the seed's first random scalar."""
    from oracle.pyoracle import prover_randomness
    d = np.load(os.path.join(GOLDEN, f"proofs_n{n}.npz"))
    v = np.stack([np.asarray(x, np.uint8).view("<u8") for x in d["value"]]).astype(np.uint64)
    gamma = np.stack([prover_randomness(p + 1, n)[0].view("<u8") for p in range(len(v))]).astype(np.uint64)
    return v, gamma, d["g"], d["h"], d["V"]


def masked(rng, count):
    """count random scalars masked as generate_random_scalar masks them (rp.cu:153-159), (count,4) uint64."""
    b = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    b[:, 31] &= 0x7F
    b[:, 0] &= 0xF8
    b[:, 31] |= 0x40
    return np.ascontiguousarray(b).view("<u8").astype(np.uint64).reshape(count, 4)


def values64(rng, count):
    """count random 64-bit values, (count,4) uint64."""
    v = np.zeros((count, 4), np.uint64)
    v[:, 0] = rng.integers(0, 2**64, count, dtype=np.uint64)
    return v

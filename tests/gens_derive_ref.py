"""The generator derivation restated for the tests: hashlib for X and Y, the CPU
restatement's fe_mul for T.  Nothing here calls the library under test.

  vector form, point i:  X = le(SHA-256(seed | BE32(i)))   Y = le(SHA-256(X's 32 bytes))   Z = 1   T = X * Y
  single form:           X = le(SHA-256(seed))             Y = Z = 1                           T = X * 1
"""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT_PATH = os.path.join(GOLDEN, "gens_derive_kat.json")

# first values whose blocks straddle every byte carry of the big-endian index, with the count used
CARRIES = [(255 - 2, 6), (65535 - 2, 6), (2**24 - 1 - 2, 6)]
LAST_BLOCK = (2**32 - 5, 5)
BIT255_SEED = bytes([1]) + bytes(31)   # SHA-256 of it ends in 0xa5: X has bit 255 set

# the published answers: (seed as hex, first, count) and single seeds
KAT_VECTORS = [(bytes([1]) + bytes(31), 0, 64), (bytes([2]) + bytes(31), 0, 64), (bytes([5]) + bytes(31), 2**20 - 64, 64),
               (bytes(32), 253, 6), (b"\xff" * 32, 2**32 - 5, 5), (bytes(range(32)), 2**24 - 3, 6)]
KAT_SINGLES = [bytes([3]) + bytes(31), bytes([4]) + bytes(31), BIT255_SEED, b"\xff" * 32]


def seed_bytes(seed):
    return bytes([seed]) + bytes(31) if isinstance(seed, int) else bytes(seed)


def _limbs(b32):
    return np.frombuffer(b32, dtype="<u8").astype(np.uint64)


def base_points(oracle, seed, count, first=0):
    """(count,16) uint64: points first .. first + count - 1 of the seed's vector."""
    seed = seed_bytes(seed)
    assert len(seed) == 32 and first + count <= 2**32
    out = np.zeros((count, 16), np.uint64)
    for k in range(count):
        x = hashlib.sha256(seed + int(first + k).to_bytes(4, "big")).digest()
        out[k, 0:4] = _limbs(x)
        out[k, 4:8] = _limbs(hashlib.sha256(x).digest())
        out[k, 8] = 1
        out[k, 12:16] = oracle.fe_mul(out[k, 0:4], out[k, 4:8])
    return out


def single_point(oracle, seed):
    out = np.zeros(16, np.uint64)
    out[0:4] = _limbs(hashlib.sha256(seed_bytes(seed)).digest())
    out[4] = 1
    out[8] = 1
    out[12:16] = oracle.fe_mul(out[0:4], out[4:8])
    return out


def digest(points):
    """SHA-256 of the points' bytes (128 each, little-endian limbs), as hex."""
    return hashlib.sha256(np.ascontiguousarray(points, dtype="<u8").tobytes()).hexdigest()


def make_kat(oracle):
    """The content of tests/golden/gens_derive_kat.json, from the restatement."""
    return dict(
        about="SHA-256 of the derived 128-byte points (X|Y|Z|T, little-endian u64 limbs), DESIGN section 19",
        vectors=[dict(seed=s.hex(), first=f, count=c, sha256=digest(base_points(oracle, s, c, f))) for s, f, c in KAT_VECTORS],
        singles=[dict(seed=s.hex(), sha256=digest(single_point(oracle, s))) for s in KAT_SINGLES])


if __name__ == "__main__":   # python tests/gens_derive_ref.py: rewrite the fixture
    import sys
    sys.path.insert(0, ROOT)
    from oracle import pyoracle
    if not os.path.exists(pyoracle.ORACLE_SO):
        pyoracle.build()
    with open(KAT_PATH, "w") as f:
        json.dump(make_kat(pyoracle.Oracle()), f, indent=1)
        f.write("\n")

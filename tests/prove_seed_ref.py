"""The seeded prover's derivation restated with hashlib: the reference of
tests/test_prove_seed_host.py and tests/test_prove_seeded.py.  Not a test module."""
import hashlib
import struct

import numpy as np

M64 = (1 << 64) - 1


def limb_bytes(limbs):
    """Four u64 limbs as the 32 bytes in memory (little-endian, as stored)."""
    return struct.pack("<4Q", *[int(x) & M64 for x in limbs])


def key(seed, v, gamma, index, n):
    msg = b"hipbpProverKeyV1" + bytes(seed) + limb_bytes(v) + limb_bytes(gamma) + struct.pack("<QI", index & M64, n)
    assert len(msg) == 124
    return hashlib.sha256(msg).digest()


def scalar(k, slot):
    """The scalar of `slot` under key k as four u64 limbs."""
    d = bytearray(hashlib.sha256(b"hipbpProverRndV1" + k + struct.pack("<I", slot)).digest())
    d[0] &= 0xF8
    d[31] &= 0x7F
    d[31] |= 0x40
    return struct.unpack("<4Q", bytes(d))


def derive(seed, v, gamma, index_base, n):
    """v, gamma (B,4) uint64 -> dict(sL (B,n,4), sR (B,n,4), rnd (B,4,4)) uint64."""
    B = len(v)
    out = dict(sL=np.zeros((B, n, 4), np.uint64), sR=np.zeros((B, n, 4), np.uint64), rnd=np.zeros((B, 4, 4), np.uint64))
    for p in range(B):
        k = key(seed, v[p], gamma[p], index_base + p, n)
        for s in range(4):
            out["rnd"][p, s] = scalar(k, s)
        for i in range(n):
            out["sL"][p, i] = scalar(k, 4 + i)
            out["sR"][p, i] = scalar(k, 4 + n + i)
    return out

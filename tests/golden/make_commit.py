"""Generate tests/golden/commit.npz from the reference build (oracle/_ref/libbpref.so): the
reference's own pedersen_commit (bulletproof_range_proof.cu:277) on edge-case inputs, for the batched
GPU commitments' parity tests (tests/test_commit_cpu.py, tests/test_commit_gpu.py).

pedersen_commit has C++ linkage in the library: its mangled name is looked up among the library's
dynamic symbols (nm -D), nothing of the reference is compiled or copied here.

Two (g, h) pairs:
  0  the fixtures' pair (pyoracle gh(): Z = 1)
  1  the g, h of the projective generator set in projective.npz (Z != 1)
For each pair the full cross of
  v     in EDGES = {0, 1, 2^64 - 1, p - 1, p, p + 1, 2^255 - 1, 2^256 - 1}
  gamma in EDGES + three random values masked as generate_random_scalar masks them (SHA-256 of
        "commit-gamma-" || k_le32: byte 31 &= 0x7F, byte 0 &= 0xF8, byte 31 |= 0x40)
in v-major order: row = pair * 88 + iv * 11 + ig.

Stored: g, h (2,16); v, gamma (176,4); out (176,16) the reference's results; pair (176,) the row's pair.

  python tests/golden/make_commit.py
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pyoracle as po  # noqa: E402

P = 2**255 - 19
EDGES = (0, 1, 2**64 - 1, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1)


def limbs(x):
    return np.array([(x >> (64 * i)) & (2**64 - 1) for i in range(4)], np.uint64)


def masked_random(k):
    b = bytearray(hashlib.sha256(b"commit-gamma-" + int(k).to_bytes(4, "little")).digest())
    b[31] &= 0x7F
    b[0] &= 0xF8
    b[31] |= 0x40
    return np.frombuffer(bytes(b), "<u8").astype(np.uint64)


def scalars():
    """(values (8,4), blindings (11,4)) of the cross."""
    e = np.stack([limbs(x) for x in EDGES])
    return e, np.concatenate([e, np.stack([masked_random(k) for k in range(3)])])


def cross():
    """v, gamma (88,4) of one pair's cross, v-major."""
    vs, gs = scalars()
    return np.repeat(vs, len(gs), axis=0), np.tile(gs, (len(vs), 1))


def reference_commit():
    """The reference's compiled pedersen_commit as a ctypes function."""
    syms = subprocess.check_output(["nm", "-D", "--defined-only", po.REF_SO], text=True).split()
    names = [s for s in syms if s.startswith("_Z") and "pedersen_commit" in s]
    assert len(names) == 1, names
    f = getattr(ctypes.CDLL(po.REF_SO), names[0])
    f.restype = None
    return f


def main():
    po.build()
    f = reference_commit()
    g0, h0 = po.Reference().gh()
    pj = np.load(os.path.join(HERE, "projective.npz"))
    pairs = [(g0, h0), (pj["g"], pj["h"])]
    v1, g1 = cross()
    v, gamma, out, pair = [], [], [], []
    for k, (g, h) in enumerate(pairs):
        g, h = np.ascontiguousarray(g, np.uint64), np.ascontiguousarray(h, np.uint64)
        for a, b in zip(v1, g1):
            r = po.ge()
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            f(po._p(r), po._p(a), po._p(b), po._p(g), po._p(h))
            v.append(a); gamma.append(b); out.append(r); pair.append(k)
    path = os.path.join(HERE, "commit.npz")
    np.savez_compressed(path, g=np.stack([p[0] for p in pairs]), h=np.stack([p[1] for p in pairs]), v=np.stack(v),
                        gamma=np.stack(gamma), out=np.stack(out), pair=np.array(pair, np.int64))
    print(f"{path}: {len(out)} rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

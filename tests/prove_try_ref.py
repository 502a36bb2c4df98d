"""The accepted prover's retry derivation restated with hashlib, on top of
tests/prove_seed_ref.py: the reference of tests/test_prove_try_host.py and
tests/test_prove_accepted.py.  Not a test module."""
import hashlib
import struct

import numpy as np

import prove_seed_ref as ref


def try_key(k, a):
    """key_{p,a} from key_p = k (32 bytes): k itself for a = 0."""
    if a == 0:
        return bytes(k)
    msg = b"hipbpProverTryV1" + bytes(k) + struct.pack("<I", a)
    assert len(msg) == 52
    return hashlib.sha256(msg).digest()


def scalars(k, n):
    """Every scalar under key k: dict(rnd (4,4), sL (n,4), sR (n,4)) uint64."""
    return dict(rnd=np.array([ref.scalar(k, s) for s in range(4)], np.uint64),
                sL=np.array([ref.scalar(k, 4 + i) for i in range(n)], np.uint64).reshape(n, 4),
                sR=np.array([ref.scalar(k, 4 + n + i) for i in range(n)], np.uint64).reshape(n, 4))


def derive_at(seed, v, gamma, index_base, n, attempt):
    """v, gamma (B,4) uint64, attempt (B,) -> dict(sL (B,n,4), sR (B,n,4), rnd (B,4,4)) uint64."""
    per = [scalars(try_key(ref.key(seed, v[p], gamma[p], index_base + p, n), int(attempt[p])), n) for p in range(len(v))]
    return {k: np.stack([x[k] for x in per]) for k in ("sL", "sR", "rnd")}

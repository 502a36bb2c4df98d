"""TEST INFRASTRUCTURE shared by tests/test_proof_ids_cpu.py, tests/test_proof_ids_gpu.py and
tests/golden/make_proof_id.py: proof ids and the batch Merkle root restated with hashlib
and struct from the contract's text, on top of the blob's restatement (tests/codec_ref.py).  The
Merkle root and the audit path are RFC 6962's recursive definitions (§2.1 MTH, §2.1.1 PATH), not the
level-by-level form the library builds."""
import hashlib
import struct

import numpy as np

import codec_ref as cr

TAG = b"hipbpProofIdV1"


def record(oracle, arrs, i, f):
    """(kind, the bytes the blob stores for proof i)."""
    u = lambda a: np.ascontiguousarray(a, dtype="<u8").tobytes()
    pts = [arrs[k][i] for k in cr.POINTS] + list(arrs["L"][i]) + list(arrs["R"][i])
    blind = (u(arrs["taux"][i]) + u(arrs["mu"][i])) if f else b""
    if cr.is_compact(oracle, arrs, i):
        return 0, b"".join(u(P[:8]) for P in pts) + u(arrs["t"][i]) + u(arrs["x"][i]) + blind
    return 1, (b"".join(u(P) for P in pts) + u(arrs["t"][i]) + u(arrs["c"][i]) + u(arrs["x"][i]) + blind +
               u(arrs["a"][i]) + u(arrs["b"][i]))


def message(oracle, arrs, n, i, with_blinding=False):
    """(kind, hdr || record) of proof i."""
    f = 1 if with_blinding else 0
    kind, rec = record(oracle, arrs, i, f)
    abl, Lr = arrs["a"].shape[1], arrs["L"].shape[1]
    sc, sr = cr.sizes(abl, Lr, f)
    assert len(rec) == (sr if kind else sc)
    hdr = TAG + bytes([kind, f]) + struct.pack("<IIII", n, abl, Lr, 0)
    assert len(hdr) == 32
    return kind, hdr + rec


def proof_ids(oracle, arrs, n, with_blinding=False):
    """-> (ids: list of 32-byte digests, kinds: list of 0 / 1)."""
    ids, kinds = [], []
    for i in range(len(arrs["V"])):
        k, m = message(oracle, arrs, n, i, with_blinding)
        ids.append(hashlib.sha256(m).digest())
        kinds.append(k)
    return ids, kinds


def ids_array(ids):
    return np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32)


# ------------------------------------------------------------------ RFC 6962 §2.1, recursively
def _split(n):
    """The largest power of two smaller than n (n > 1)."""
    k = 1
    while 2 * k < n:
        k *= 2
    return k


def mth(d):
    if len(d) == 0:
        return hashlib.sha256(b"").digest()
    if len(d) == 1:
        return hashlib.sha256(b"\x00" + d[0]).digest()
    k = _split(len(d))
    return hashlib.sha256(b"\x01" + mth(d[:k]) + mth(d[k:])).digest()


def path(m, d):
    """PATH(m, D[n]) (§2.1.1): the audit path of leaf m, bottom-up."""
    if len(d) == 1:
        return []
    k = _split(len(d))
    if m < k:
        return path(m, d[:k]) + [mth(d[k:])]
    return path(m - k, d[k:]) + [mth(d[:k])]


def kat_ids(count):
    """The issue's Merkle inputs: ids_k = SHA-256(bytes([k & 255, k >> 8]))."""
    return [hashlib.sha256(bytes([k & 255, k >> 8])).digest() for k in range(count)]

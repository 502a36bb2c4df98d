"""TEST INFRASTRUCTURE shared by tests/test_codec_cpu.py, tests/test_codec_gpu.py and
tests/golden/make_codec.py: the compact proof blob ("HBPC" version 1) restated in Python
from the format's description alone, with fe25519_mul through the C restatement (the `oracle`
fixture), and the golden proof sets as the arrays the codec takes."""
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POINTS = ("V", "A", "S", "T1", "T2")
ONE = np.array([1, 0, 0, 0], np.uint64)


def pad8(x):
    return (x + 7) & ~7


def sizes(ab_len, Lr, f):
    """(S_c, S_r)"""
    sc = 64 * (5 + 2 * Lr) + 64 + 64 * f if ab_len == 1 else 0
    return sc, 128 * (5 + 2 * Lr) + 96 + 64 * f + 64 * ab_len


def blob_bytes(count, ab_len, Lr, f, R):
    sc, sr = sizes(ab_len, Lr, f)
    return 32 + pad8(count) + count * sc + pad8(4 * R) + R * sr


def _points(arrs, i):
    return [arrs[k][i] for k in POINTS] + list(arrs["L"][i]) + list(arrs["R"][i])


def is_compact(oracle, arrs, i):
    """Compared on the stored limbs, never mod p."""
    if arrs["a"].shape[1] != 1:
        return False
    t = arrs["t"][i]
    if not (np.array_equal(arrs["a"][i][0], t) and np.array_equal(arrs["c"][i], t) and np.array_equal(arrs["b"][i][0], ONE)):
        return False
    for P in _points(arrs, i):
        if not np.array_equal(P[8:12], ONE) or not np.array_equal(P[12:16], oracle.fe_mul(P[0:4], P[4:8])):
            return False
    return True


def encode(oracle, arrs, n, with_blinding=False):
    """arrs: dict of uint64 arrays V A S T1 T2 (B,16), t c x [taux mu] (B,4), a b (B,abl,4), L R (B,Lr,16)."""
    u = lambda a: np.ascontiguousarray(a, dtype="<u8").tobytes()
    B, abl, Lr, f = len(arrs["V"]), arrs["a"].shape[1], arrs["L"].shape[1], 1 if with_blinding else 0
    sc, _ = sizes(abl, Lr, f)
    kind = [0 if is_compact(oracle, arrs, i) else 1 for i in range(B)]
    raw = [i for i in range(B) if kind[i]]
    out = [b"HBPC" + struct.pack("<HHIIIIQ", 1, f, n, abl, Lr, len(raw), B)]
    out.append(bytes(kind) + bytes(pad8(B) - B))
    blind = lambda i: (u(arrs["taux"][i]) + u(arrs["mu"][i])) if f else b""
    for i in range(B):
        if kind[i]:
            out.append(bytes(sc))
        else:
            out.append(b"".join(u(P[:8]) for P in _points(arrs, i)) + u(arrs["t"][i]) + u(arrs["x"][i]) + blind(i))
    out.append(struct.pack(f"<{len(raw)}I", *raw) + bytes(pad8(4 * len(raw)) - 4 * len(raw)))
    for i in raw:
        out.append(b"".join(u(P) for P in _points(arrs, i)) + u(arrs["t"][i]) + u(arrs["c"][i]) + u(arrs["x"][i]) +
                   blind(i) + u(arrs["a"][i]) + u(arrs["b"][i]))
    blob = b"".join(out)
    assert len(blob) == blob_bytes(B, abl, Lr, f, len(raw))
    return blob


def decode(oracle, blob):
    """-> (n, arrs) with taux / mu when stored."""
    magic, ver, f, n, abl, Lr, R, B = struct.unpack("<4sHHIIIIQ", blob[:32])
    assert magic == b"HBPC" and ver == 1 and f in (0, 1) and len(blob) == blob_bytes(B, abl, Lr, f, R)
    sc, sr = sizes(abl, Lr, f)
    kind = blob[32:32 + B]
    o_c = 32 + pad8(B)
    o_i = o_c + B * sc
    ridx = struct.unpack(f"<{R}I", blob[o_i:o_i + 4 * R])
    o_r = o_i + pad8(4 * R)
    g = lambda b: np.frombuffer(b, "<u8").astype(np.uint64)
    arrs = {k: np.zeros((B, 16), np.uint64) for k in POINTS}
    arrs.update({k: np.zeros((B, 4), np.uint64) for k in ("t", "c", "x") + (("taux", "mu") if f else ())})
    arrs.update(a=np.zeros((B, abl, 4), np.uint64), b=np.zeros((B, abl, 4), np.uint64),
                L=np.zeros((B, Lr, 16), np.uint64), R=np.zeros((B, Lr, 16), np.uint64))
    npts = 5 + 2 * Lr

    def put_points(i, pts):
        for k, P in zip(POINTS, pts[:5]):
            arrs[k][i] = P
        arrs["L"][i] = np.array(pts[5:5 + Lr], np.uint64).reshape(Lr, 16)
        arrs["R"][i] = np.array(pts[5 + Lr:], np.uint64).reshape(Lr, 16)

    for i in range(B):
        if kind[i]:
            j = ridx.index(i)
            rec = blob[o_r + j * sr:o_r + (j + 1) * sr]
            put_points(i, [g(rec[128 * q:128 * q + 128]) for q in range(npts)])
            fs = g(rec[128 * npts:]).reshape(-1, 4)
            names = ["t", "c", "x"] + (["taux", "mu"] if f else [])
            for k, name in enumerate(names):
                arrs[name][i] = fs[k]
            arrs["a"][i] = fs[len(names):len(names) + abl]
            arrs["b"][i] = fs[len(names) + abl:]
        else:
            slot = blob[o_c + i * sc:o_c + (i + 1) * sc]
            pts = []
            for q in range(npts):
                xy = g(slot[64 * q:64 * q + 64])
                pts.append(np.concatenate([xy, ONE, oracle.fe_mul(xy[:4], xy[4:])]))
            put_points(i, pts)
            fs = g(slot[64 * npts:]).reshape(-1, 4)
            arrs["t"][i], arrs["x"][i] = fs[0], fs[1]
            if f:
                arrs["taux"][i], arrs["mu"][i] = fs[2], fs[3]
            arrs["a"][i][0] = arrs["c"][i] = fs[0]
            arrs["b"][i][0] = ONE
    return n, arrs


# ------------------------------------------------------------------ the golden sets as codec arrays
def from_heads(head, V, a, b, L, R):
    """head (B,100) = V,A,S,T1,T2 | taux,mu,t,c,x.  The encoded V is the proof's own (the head's)."""
    head = np.asarray(head, np.uint64)
    arrs = {k: np.ascontiguousarray(head[:, 16 * i:16 * i + 16]) for i, k in enumerate(POINTS)}
    for i, k in enumerate(("taux", "mu", "t", "c", "x")):
        arrs[k] = np.ascontiguousarray(head[:, 80 + 4 * i:84 + 4 * i])
    arrs.update(a=np.asarray(a, np.uint64), b=np.asarray(b, np.uint64), L=np.asarray(L, np.uint64), R=np.asarray(R, np.uint64))
    return arrs


def golden_set(name):
    """name: proofs_n16, proofs_n64, rpverify_n16, rpverify_n64 -> (n, arrs, d): the set's arrays and
    the fixture it came from."""
    if name.startswith("proofs_"):
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        return int(name[8:]), from_heads(d["head"], d["V"], d["a"], d["b"], d["L"], d["R"]), d
    n = int(name[10:])
    d = dict(np.load(os.path.join(GOLDEN, "rpverify.npz")))
    p = f"n{n}_"
    return n, from_heads(d[p + "head"], d[p + "V"], d[p + "a"], d[p + "b"], d[p + "L"], d[p + "R"]), d


def take(arrs, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in arrs.items()}


def to_dicts(arrs):
    """The arrays as the proof dicts the host entry points take."""
    B = len(arrs["V"])
    z = np.zeros(4, np.uint64)
    return [dict(head=np.concatenate([arrs[k][i] for k in POINTS] +
                                     [arrs["taux"][i] if "taux" in arrs else z, arrs["mu"][i] if "mu" in arrs else z,
                                      arrs["t"][i], arrs["c"][i], arrs["x"][i]]),
                 a=arrs["a"][i], b=arrs["b"][i], L=arrs["L"][i], R=arrs["R"][i]) for i in range(B)]


def from_dicts(proofs, blinding):
    head = np.stack([p["head"] for p in proofs])
    arrs = from_heads(head, None, np.stack([p["a"] for p in proofs]), np.stack([p["b"] for p in proofs]),
                      np.stack([p["L"].reshape(-1, 16) for p in proofs]), np.stack([p["R"].reshape(-1, 16) for p in proofs]))
    if not blinding:
        del arrs["taux"], arrs["mu"]
    return arrs


def same(a, b, keys=None):
    keys = keys or sorted(set(a) & set(b))
    return all(np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)) for k in keys)

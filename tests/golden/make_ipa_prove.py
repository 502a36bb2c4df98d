"""Generate tests/golden/ipa_prove.npz from the reference build (oracle/_ref/libbpref.so): the
reference's own inner_product_prove (bulletproof_vectors.cu:277) on derived inputs, for the GPU
prover's parity tests (tests/test_ipa_prove.py).

Only OUTPUTS are stored.  The inputs of case k are derived (case_inputs below) from SHA-256 of
tag || k_le32 || i_le32, bit 255 cleared, and shaped by the case's recipe:
  0 random    a, b random; c_in = <a, b>; zero transcript
  1 a_zero    a all zero
  2 classes   a_j = 0 for even j, b_1 = 0, b_3 = 5: constant, light and heavy terms in one proof
  3 high      every element in [p, 2^255): a_0 = 2^255 - 19, a_1 = 2^255 - 1, b_0 = 2^255 - 1, b_1 = p,
              the rest p + (hash mod 19)
  4 transcript  a non-zero initial transcript with byte 31 >= 0x80
  5 c_wrong   a c_in that is not <a, b>
G, H = base points {1}, {2}; Q = h.

Stored per case: n, recipe, the final a, b, x, c_in, c_final (= <a', b'> of the final vectors), L, R
(concatenated; L_off[k] .. L_off[k + 1]), P = the canonical-tree MSM(a || b, G || H), the reference's
cuda_inner_product_verify verdicts with c_in and with c_final, and the check point for c_final.

  python tests/golden/make_ipa_prove.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pyoracle as po  # noqa: E402

TAG = b"ipa-prove-"
RECIPES = ("random", "a_zero", "classes", "high", "transcript", "c_wrong")
M63 = np.uint64(0x7FFFFFFFFFFFFFFF)
P_LIMBS = np.array([0xFFFFFFFFFFFFFFED, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF], np.uint64)

# (n, recipe) per case, in fixture order
CASES = [(n, 0) for n in (1, 2, 4, 8, 64, 256) for _ in range(3)] + [(8, r) for r in (1, 2, 3, 4, 5)] + \
        [(4096, 0), (4096, 0)]


def _h(kind, case, i):
    return hashlib.sha256(TAG + kind + int(case).to_bytes(4, "little") + int(i).to_bytes(4, "little")).digest()


def _vec(kind, case, n):
    v = np.stack([np.frombuffer(_h(kind, case, i), "<u8") for i in range(n)]).astype(np.uint64)
    v[:, 3] &= M63
    return v


def case_inputs(case, n, recipe):
    """(a (n,4), b (n,4), transcript (32,) uint8, c_override (4,) or None) of fixture case `case`."""
    a, b = _vec(b"a", case, n), _vec(b"b", case, n)
    tr = np.zeros(32, np.uint8)
    c = None
    if recipe == 1:
        a[:] = 0
    elif recipe == 2:
        a[0::2] = 0
        b[1] = 0
        b[3] = (5, 0, 0, 0)
    elif recipe == 3:
        for v in (a, b):
            k = v[:, 0] % np.uint64(19)
            v[:] = P_LIMBS
            v[:, 0] += k            # p + k, k < 19: below 2^255, no carry out of limb 0
        a[0] = P_LIMBS
        a[1] = (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF)
        b[0] = a[1]
        b[1] = P_LIMBS
    elif recipe == 4:
        t = bytearray(_h(b"t", case, 0))
        t[31] |= 0x80
        tr = np.frombuffer(bytes(t), np.uint8).copy()
    elif recipe == 5:
        c = np.frombuffer(_h(b"c", case, 0), "<u8").astype(np.uint64)
        c[3] &= M63
    return a, b, tr, c


def generators(src, n):
    """G, H, Q of every case; src: pyoracle.Reference or pyoracle.Oracle (the same points)."""
    _, Q = src.gh()
    return src.base_points(n, 1), src.base_points(n, 2), Q


def make_case(R, case, n, recipe, inputs=None, verify=True):
    """One case through the reference: dict of the stored outputs.  inputs: (a, b, transcript,
    c_override) in place of case_inputs' (make_ipa_prove_sizes.py's recipes); verify=False leaves
    P, the verdicts and the check point (three more O(n) passes) zero."""
    a, b, tr, c_over = case_inputs(case, n, recipe) if inputs is None else inputs
    G, H, Q = generators(R, n)
    c_in = po.fe()
    R.f("inner_product")(po._p(c_in), po._p(a), po._p(b), po._sz(n))
    if c_over is not None:
        assert not np.array_equal(c_over, c_in)
        c_in = c_over
    pr = R.ipa_prove(a, b, G, H, Q, c_in, tr)
    assert pr is not None and len(pr["a"]) == 1 and len(pr["L"]) == n.bit_length() - 1
    c_final = po.fe()
    R.f("inner_product")(po._p(c_final), po._p(pr["a"]), po._p(pr["b"]), po._sz(1))
    if not verify:
        return dict(a=pr["a"][0], b=pr["b"][0], x=pr["x"], c_in=c_in, c_final=c_final, L=pr["L"].reshape(-1, 16),
                    R=pr["R"].reshape(-1, 16), P=po.ge(), ok_in=False, ok_final=False, check=po.ge())
    P = R.msm("msm_canon", np.concatenate([a, b]), np.concatenate([G, H]))
    ok_in = R.cuda_inner_product_verify(n, pr["a"], pr["b"], c_in, pr["L"], pr["R"], pr["x"], P, G, H, Q)
    ok_final = R.cuda_inner_product_verify(n, pr["a"], pr["b"], c_final, pr["L"], pr["R"], pr["x"], P, G, H, Q)
    _, _, chk = R.ipa_fold(G, H, n, pr["x"], pr["L"], pr["R"], pr["a"][0], pr["b"][0], c_final, Q)
    return dict(a=pr["a"][0], b=pr["b"][0], x=pr["x"], c_in=c_in, c_final=c_final, L=pr["L"].reshape(-1, 16),
                R=pr["R"].reshape(-1, 16), P=P, ok_in=ok_in, ok_final=ok_final, check=chk)


def pack(recs):
    """Per-case dicts -> the fixture's arrays."""
    out = {k: np.stack([r[k] for r in recs]) for k in ("a", "b", "x", "c_in", "c_final", "P", "check")}
    out["ok_in"] = np.array([r["ok_in"] for r in recs], np.uint8)
    out["ok_final"] = np.array([r["ok_final"] for r in recs], np.uint8)
    out["L"] = np.concatenate([r["L"] for r in recs])
    out["R"] = np.concatenate([r["R"] for r in recs])
    out["L_off"] = np.cumsum([0] + [len(r["L"]) for r in recs]).astype(np.int64)
    return out


def main():
    po.build()
    R = po.Reference()
    recs = []
    for case, (n, recipe) in enumerate(CASES):
        recs.append(make_case(R, case, n, recipe))
        print(f"case {case}: n = {n} {RECIPES[recipe]}: ok_in {recs[-1]['ok_in']} ok_final {recs[-1]['ok_final']}",
              flush=True)
    np.savez_compressed(os.path.join(HERE, "ipa_prove.npz"), n=np.array([c[0] for c in CASES], np.int64),
                        recipe=np.array([c[1] for c in CASES], np.int64), **pack(recs))


if __name__ == "__main__":
    main()

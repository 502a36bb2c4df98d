"""Generate tests/golden/ipa_prove_sizes.npz from the reference build (oracle/_ref/libbpref.so): the
reference's own inner_product_prove on derived inputs at the lengths and element values that
ipa_prove.npz (make_ipa_prove.py) leaves out, for tests/test_ipa_prove_sizes.py.

Only OUTPUTS are stored, with make_ipa_prove's make_case and pack.  The cases are numbered from
CASE0 = 100 (case_id), so their SHA-256-derived inputs differ from the older fixture's.  Recipes 0
(random) and 1 (a_zero) are make_ipa_prove's; two are new:
  6 wide            every element is hash | 2^255.  At j = 0 .. 3 and again at n/2 + j (so the
                    a_L b_R and a_R b_L products and both fold operands meet them):
                      a_0 = b_0 = 2^256 - 1       a_1 = 2^256 - 19     b_1 = 2^256 - 38 (= 2p)
                      a_2 = 2^255                 b_2 = 2^255 + 19
                      a_3: top limb MUL_BOUNDED_WORD << 32 | 0xFFFFFFFF (the product gate's word at the bound)
                      b_3: top limb (MUL_BOUNDED_WORD + 1) << 32        (one above it)
                    MUL_BOUNDED_WORD is read from cudabulletproof_amd/csrc/mul512_asm.h.
  7 classes_blocks  by j mod 4, a_j is 0 | light (the hash's low 64 bits, forced non-zero) | heavy
                    (the hash) | p; b_j has the same pattern shifted by two (heavy | p | 0 | light).
                    At EDGE_AT in each half, in a and in b: 1, 2^64 - 1, 2^64, 2^64 + 1, p + 1.  Every
                    256-item block of round 0's work list then holds zero, light and heavy scalars.
c_in = the reference's inner_product of the inputs; zero transcript; G, H, Q as make_ipa_prove.

P, ok_in, ok_final and check (three more O(n) passes) are stored for n <= VERIFY_MAX_N only
(has_verify), zeros elsewhere.  The reference's prover takes about 0.9 ms per element on one CPU
core (58 s at n = 65536), two minutes for the whole file; progress is printed per case.

  python tests/golden/make_ipa_prove_sizes.py
"""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import pyoracle as po  # noqa: E402
from make_ipa_prove import _vec, generators, make_case, pack  # noqa: E402,F401  (_vec hashes with its _h)

CASE0 = 100
VERIFY_MAX_N = 2048
RECIPES = {0: "random", 1: "a_zero", 6: "wide", 7: "classes_blocks"}
P = 2**255 - 19
EDGE_AT = (9, 10, 11, 13, 14)                             # offsets within each half (classes_blocks)
EDGE_VALUES = (1, 2**64 - 1, 2**64, 2**64 + 1, P + 1)     # light, light, heavy, heavy, light (p + 1 -> 1)

# (n, recipe) per case, in fixture order; case k has case_id CASE0 + k
CASES = [(n, 0) for n in (16, 16, 32, 128, 512, 1024, 2048, 8192, 16384, 32768, 65536)] + \
        [(512, 1), (16, 6), (512, 6), (512, 7)]


def mul_bounded_word():
    """The product gate's bound on a factor's top 32-bit word, from the kernels' own header."""
    hdr = os.path.join(os.path.dirname(os.path.dirname(HERE)), "cudabulletproof_amd", "csrc", "mul512_asm.h")
    return int(re.search(r"MUL_BOUNDED_WORD = 0x([0-9A-Fa-f]+)u", open(hdr).read()).group(1), 16)


def limbs(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def wide_values(a3, b3):
    """The eight named values of recipe `wide` as (a_0 .. a_3), (b_0 .. b_3); a3, b3: the hash
    elements whose low three limbs a_3, b_3 keep."""
    w = mul_bounded_word()
    a3, b3 = a3.copy(), b3.copy()
    a3[3] = np.uint64(w << 32 | 0xFFFFFFFF)
    b3[3] = np.uint64((w + 1) << 32)
    return ([limbs(2**256 - 1), limbs(2**256 - 19), limbs(2**255), a3],
            [limbs(2**256 - 1), limbs(2**256 - 38), limbs(2**255 + 19), b3])


def case_inputs(case, n, recipe):
    """(a (n,4), b (n,4), transcript (32,) uint8, None) of the case with case_id `case`."""
    a, b = _vec(b"a", case, n), _vec(b"b", case, n)
    if recipe == 1:
        a[:] = 0
    elif recipe == 6:
        a[:, 3] |= np.uint64(1 << 63)
        b[:, 3] |= np.uint64(1 << 63)
        for h in (0, n // 2):
            va, vb = wide_values(a[h + 3], b[h + 3])
            for j in range(4):
                a[h + j], b[h + j] = va[j], vb[j]
    elif recipe == 7:
        for v, shift in ((a, 0), (b, 2)):
            for j in range(n):
                m = (j + shift) % 4
                if m == 0:
                    v[j] = 0
                elif m == 1:
                    v[j] = (v[j, 0] | np.uint64(1), 0, 0, 0)
                elif m == 3:
                    v[j] = limbs(P)
            for h in (0, n // 2):
                for at, val in zip(EDGE_AT, EDGE_VALUES):
                    v[h + at] = limbs(val)
    elif recipe != 0:
        raise ValueError(recipe)
    return a, b, np.zeros(32, np.uint8), None


def make(R, k):
    """Fixture case k (case_id CASE0 + k) through the reference."""
    n, recipe = CASES[k]
    return make_case(R, CASE0 + k, n, recipe, inputs=case_inputs(CASE0 + k, n, recipe), verify=n <= VERIFY_MAX_N)


def main():
    po.build()
    R = po.Reference()
    recs = []
    for k, (n, recipe) in enumerate(CASES):
        t0 = time.time()
        recs.append(make(R, k))
        print(f"case {CASE0 + k}: n = {n} {RECIPES[recipe]}: ok_in {recs[-1]['ok_in']} ok_final "
              f"{recs[-1]['ok_final']} ({time.time() - t0:.1f} s)", flush=True)
    ns = np.array([c[0] for c in CASES], np.int64)
    np.savez_compressed(os.path.join(HERE, "ipa_prove_sizes.npz"), n=ns,
                        recipe=np.array([c[1] for c in CASES], np.int64),
                        case_id=CASE0 + np.arange(len(CASES), dtype=np.int64),
                        has_verify=(ns <= VERIFY_MAX_N).astype(np.uint8), **pack(recs))


if __name__ == "__main__":
    main()

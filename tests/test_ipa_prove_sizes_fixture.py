"""tests/golden/ipa_prove_sizes.npz (the reference's inner_product_prove outputs at the lengths and
element values ipa_prove.npz leaves out, tests/golden/make_ipa_prove_sizes.py) is consistent with its
case list and input recipes; where the reference build is available, the cases with n <= 512 are
regenerated and must reproduce the stored bytes.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

P = 2**255 - 19
TPB = 256   # bp_ipa_prove.hip: k_ipa_scatter's block


def _int(fe):
    return sum(int(v) << (64 * i) for i, v in enumerate(fe))


def _canon(oracle, fe):
    return int.from_bytes(oracle.fe_tobytes(fe).tobytes(), "little")


def _sclass(v):
    """bp_ipa_prove.hip sclass on a canonical value: 0 zero, 1 light (<= 64 bits), 2 heavy."""
    return 0 if v == 0 else 1 if v < 2**64 else 2


def round0_classes(oracle, a, b):
    """The classes of one proof's round-0 items in k_ipa_scatter's order (4n' + 2 items: a_L | b_R | a_R
    | b_L | c_L | c_R), from the tobytes form.  Class 0 items are written by k_ipa_scatter itself;
    only classes 2 and 1 are queued for k_ipa_terms (slist, then llist)."""
    h = len(a) // 2
    items = np.concatenate([a[:h], b[h:], a[h:], b[:h],
                            oracle.inner_product(a[:h], b[h:])[None], oracle.inner_product(a[h:], b[:h])[None]])
    assert len(items) == 4 * h + 2
    return np.array([_sclass(_canon(oracle, s)) for s in items])


TERMS_LANES = 1024 * TPB   # bp_ipa_prove.hip: k_ipa_terms' largest grid (TERMS_BLOCKS blocks)
GRID_STRIDE_B = 40000      # test_ipa_prove_sizes.py: ipa_prove.npz's n = 8 cases tiled to this many proofs


def n8_queued_per_chunk(oracle, B):
    """ipa_prove.npz's eight n = 8 cases tiled to B proofs (proof p is case p mod 8), cut as ipa_enqueue
    cuts them (two chunks of ceil(B / 2)): round 0's (heavy, light) item counts of each chunk, which
    are k_ipa_terms' ch and cl: its loop runs over ch + cl, heavy items first."""
    import make_ipa_prove as old
    ks = [k for k, (n, _) in enumerate(old.CASES) if n == 8]
    assert len(ks) == 8
    cls = [round0_classes(oracle, *old.case_inputs(k, 8, old.CASES[k][1])[:2]) for k in ks]
    per = [(int((c == 2).sum()), int((c == 1).sum())) for c in cls]
    Bc = (B + 1) // 2
    out = []
    for p0 in range(0, B, Bc):
        chunk = [per[p % 8] for p in range(p0, min(p0 + Bc, B))]
        out.append((sum(h for h, _ in chunk), sum(l for _, l in chunk)))
    return out


def test_grid_stride_batch_queues_past_the_grid(oracle):
    """k_ipa_terms strides over the QUEUED items (zero scalars are constants written by k_ipa_scatter),
    126 (112 heavy, 14 light) per eight n = 8 cases, not 8 x 18.  At B = 30000 a chunk has 270000
    items but queues 236250, fewer than the 262144 lanes: one turn of the loop.  At GRID_STRIDE_B each chunk's heavy items
    alone fill the grid, so the second turn takes the rest of slist and every llist entry
    (llist[i - ch] with i >= 262144)."""
    assert n8_queued_per_chunk(oracle, 30000) == [(210000, 26250)] * 2 and 210000 + 26250 < TERMS_LANES
    for ch, cl in n8_queued_per_chunk(oracle, GRID_STRIDE_B):
        assert ch >= TERMS_LANES and cl > 0, (ch, cl)


def test_case_list_and_shapes(golden):
    from make_ipa_prove_sizes import CASE0, CASES, RECIPES, VERIFY_MAX_N
    d = golden("ipa_prove_sizes")
    K = len(CASES)
    assert CASES == [(n, 0) for n in (16, 16, 32, 128, 512, 1024, 2048, 8192, 16384, 32768, 65536)] + \
        [(512, 1), (16, 6), (512, 6), (512, 7)]
    assert RECIPES == {0: "random", 1: "a_zero", 6: "wide", 7: "classes_blocks"}
    assert [tuple(x) for x in zip(d["n"].tolist(), d["recipe"].tolist())] == CASES
    assert CASE0 == 100 and d["case_id"].tolist() == list(range(100, 100 + K))
    assert VERIFY_MAX_N == 2048 and d["has_verify"].tolist() == [int(n <= 2048) for n, _ in CASES]
    for k in ("a", "b", "x", "c_in", "c_final"):
        assert d[k].shape == (K, 4) and d[k].dtype == np.uint64, k
    for k in ("P", "check"):
        assert d[k].shape == (K, 16) and d[k].dtype == np.uint64, k
        assert not d[k][d["has_verify"] == 0].any(), k
        assert all(row.any() for row in d[k][d["has_verify"] == 1]), k
    assert d["ok_in"].shape == d["ok_final"].shape == (K,)
    assert not d["ok_in"][d["has_verify"] == 0].any() and not d["ok_final"][d["has_verify"] == 0].any()
    rounds = [n.bit_length() - 1 for n, _ in CASES]
    assert d["L_off"].tolist() == np.cumsum([0] + rounds).tolist()
    assert d["L"].shape == d["R"].shape == (sum(rounds), 16)
    assert all(row.any() for row in d["L"]) and all(row.any() for row in d["R"])
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "ipa_prove_sizes.npz")) < 1 << 20


def test_inputs_differ_from_the_older_fixtures():
    """Numbered from 100: no case shares its derived elements with an ipa_prove.npz case."""
    import make_ipa_prove as old
    from make_ipa_prove_sizes import CASE0, _vec
    assert CASE0 >= len(old.CASES)
    assert not np.array_equal(_vec(b"a", CASE0, 16)[:8], _vec(b"a", 9, 8))


def test_c_in_and_c_final(golden, oracle):
    """c_in is <a, b> of the derived inputs (n <= 2048 here: the chain is sequential) and
    c_final = fe_add(0, fe_mul(a, b)) of the final a, b, through the CPU restatement."""
    from make_ipa_prove_sizes import CASE0, CASES, case_inputs
    d = golden("ipa_prove_sizes")
    zero = np.zeros(4, np.uint64)
    for k, (n, recipe) in enumerate(CASES):
        assert np.array_equal(d["c_final"][k], oracle.fe_add(zero, oracle.fe_mul(d["a"][k], d["b"][k]))), k
        if n <= 2048:
            a, b, tr, c_over = case_inputs(CASE0 + k, n, recipe)
            assert c_over is None and not tr.any() and a.shape == b.shape == (n, 4)
            assert np.array_equal(d["c_in"][k], oracle.inner_product(a, b)), k


def test_recipe_a_zero():
    from make_ipa_prove_sizes import CASE0, CASES, case_inputs
    k = CASES.index((512, 1))
    a, b, _, _ = case_inputs(CASE0 + k, 512, 1)
    assert not a.any() and all(v.any() for v in b)


def test_recipe_wide(golden):
    """Every element has bit 255 set, the eight named values stand at j and n/2 + j in both halves,
    and the gate words are the kernels' own MUL_BOUNDED_WORD.  The reference's final a, b of these
    proofs need not be below 2^255 either; at least one stored output of the wide cases is not."""
    from make_ipa_prove_sizes import CASE0, CASES, case_inputs, mul_bounded_word
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "cudabulletproof_amd", "csrc",
                            "mul512_asm.h")).read()
    w = int(re.search(r"MUL_BOUNDED_WORD = 0x([0-9A-F]+)u", hdr).group(1), 16)
    assert mul_bounded_word() == w and w < 0xFFFFFFFF
    d = golden("ipa_prove_sizes")
    ks = [k for k, c in enumerate(CASES) if c[1] == 6]
    assert [CASES[k][0] for k in ks] == [16, 512]
    for k in ks:
        n = CASES[k][0]
        a, b, _, _ = case_inputs(CASE0 + k, n, 6)
        va, vb = [_int(v) for v in a], [_int(v) for v in b]
        assert min(va + vb) >= 2**255
        for h in (0, n // 2):
            assert va[h:h + 3] == [2**256 - 1, 2**256 - 19, 2**255]
            assert vb[h:h + 3] == [2**256 - 1, 2**256 - 38, 2**255 + 19] and vb[h + 1] == 2 * P
            assert int(a[h + 3, 3]) == w << 32 | 0xFFFFFFFF and int(b[h + 3, 3]) == (w + 1) << 32
            # the 32-bit words the product gate reads: a factor's top word at the bound, and one above it
            assert int(a[h + 3, 3]) >> 32 == w and int(b[h + 3, 3]) >> 32 == w + 1
            assert a[h + 3, :3].any() and b[h + 3, :3].any()
    assert any(int(d[key][k][3]) >> 63 for k in ks for key in ("a", "b"))


def test_recipe_classes_blocks(oracle):
    """Round 0's work list as k_ipa_scatter lays it out (4n' + 2 items per proof: a_L | b_R | a_R | b_L
    | c_L | c_R, blocks of 256 lanes), classes from the tobytes form: every full block holds zero,
    light and heavy scalars, and the boundary values fall in the class they are named for."""
    from make_ipa_prove_sizes import CASE0, CASES, EDGE_AT, EDGE_VALUES, case_inputs
    k = CASES.index((512, 7))
    n, np_ = 512, 256
    a, b, _, _ = case_inputs(CASE0 + k, n, 7)
    cls = round0_classes(oracle, a, b)
    assert len(cls) == 4 * np_ + 2
    full = len(cls) // TPB
    assert full == 4
    for blk in range(full):
        c = np.bincount(cls[blk * TPB:(blk + 1) * TPB], minlength=3)
        assert c.min() >= 32, (blk, c.tolist())          # and no class is a rarity in its block
    # the boundaries: raw value -> the class of its tobytes form
    assert EDGE_VALUES == (1, 2**64 - 1, 2**64, 2**64 + 1, P + 1)
    want = {0: 0, P: 0, 1: 1, 2**64 - 1: 1, P + 1: 1, 2**64: 2, 2**64 + 1: 2}
    for vec, shift in ((a, 0), (b, 2)):
        for h in (0, np_):
            for at, val in zip(EDGE_AT, EDGE_VALUES):
                assert _int(vec[h + at]) == val
                assert _sclass(_canon(oracle, vec[h + at])) == want[val], hex(val)
        for j in range(n):
            if j % np_ in EDGE_AT:
                continue
            raw, m = _int(vec[j]), (j + shift) % 4
            assert (raw == 0, 0 < raw < 2**64, 2**64 <= raw < 2**255, raw == P)[m], (j, hex(raw))
            assert _sclass(_canon(oracle, vec[j])) == (0, 1, 2, 0)[m]
    assert _canon(oracle, np.array([0xFFFFFFFFFFFFFFED, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF],
                                   np.uint64)) == 0


def test_regenerated_small_cases_reproduce_the_fixture(golden):
    from oracle import pyoracle as po
    if not po.have_reference():
        try:
            po.build()
        except Exception:   # noqa: BLE001
            pass
    if not po.have_reference():
        pytest.skip("the reference build (oracle/_ref/libbpref.so) is not available")
    from make_ipa_prove import pack
    from make_ipa_prove_sizes import CASES, make
    d = golden("ipa_prove_sizes")
    idx = [k for k, (n, _) in enumerate(CASES) if n <= 512]
    assert len(idx) == 9
    R = po.Reference()
    got = pack([make(R, k) for k in idx])
    lo = d["L_off"]
    for key in ("a", "b", "x", "c_in", "c_final", "P", "check", "ok_in", "ok_final"):
        assert np.array_equal(got[key], d[key][idx]), key
    for key in ("L", "R"):
        assert np.array_equal(got[key], np.concatenate([d[key][lo[k]:lo[k + 1]] for k in idx])), key

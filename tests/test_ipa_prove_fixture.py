"""tests/golden/ipa_prove.npz (the reference's inner_product_prove outputs, tests/golden/make_ipa_prove.py)
is consistent with its case list and input recipes; where the reference build is available, the
n = 8 cases are regenerated and must reproduce the stored bytes.  CPU only.

Every input of THIS fixture has bit 255 clear (asserted below as a property of its recipes); that is
not the prover's contract, which is the reference's bits for any limbs: ipa_prove_sizes.npz
(test_ipa_prove_sizes_fixture.py) holds the cases with elements up to 2^256 - 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

P = 2**255 - 19


def _int(fe):
    return sum(int(v) << (64 * i) for i, v in enumerate(fe))


def test_case_list_and_shapes(golden):
    from make_ipa_prove import CASES, RECIPES
    d = golden("ipa_prove")
    K = len(CASES)
    assert [tuple(x) for x in zip(d["n"].tolist(), d["recipe"].tolist())] == CASES
    assert all(0 <= r < len(RECIPES) for _, r in CASES)
    # the issue's case list: three random instances per n, five edge cases at n = 8, two at n = 4096
    for n in (1, 2, 4, 8, 64, 256):
        assert CASES.count((n, 0)) == 3
    assert [c for c in CASES if c[1]] == [(8, r) for r in (1, 2, 3, 4, 5)] and CASES.count((4096, 0)) == 2
    for k in ("a", "b", "x", "c_in", "c_final"):
        assert d[k].shape == (K, 4) and d[k].dtype == np.uint64, k
    for k in ("P", "check"):
        assert d[k].shape == (K, 16) and d[k].dtype == np.uint64, k
    assert d["ok_in"].shape == d["ok_final"].shape == (K,)
    rounds = [n.bit_length() - 1 for n, _ in CASES]
    assert d["L_off"].tolist() == np.cumsum([0] + rounds).tolist()
    assert d["L"].shape == d["R"].shape == (sum(rounds), 16)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "ipa_prove.npz")) < 1 << 20


def test_input_recipes(golden, oracle):
    """The derived inputs have the properties the cases are named for, and the stored c_in, c_final and
    n = 1 outputs follow from them through the CPU restatement's field arithmetic."""
    from make_ipa_prove import CASES, case_inputs
    d = golden("ipa_prove")
    for k, (n, recipe) in enumerate(CASES):
        a, b, tr, c_over = case_inputs(k, n, recipe)
        assert a.shape == b.shape == (n, 4) and tr.shape == (32,)
        assert int(a[:, 3].max()) < 2**63 and int(b[:, 3].max()) < 2**63
        ip = oracle.inner_product(a, b) if n <= 256 else None
        if recipe == 1:
            assert not a.any()
        if recipe == 2:
            light = lambda v: not v[1:].any() and v[0] != 0
            assert not a[0::2].any() and all(v[1:].any() for v in a[1::2])     # constant / heavy
            assert not b[1].any() and light(b[3]) and int(b[3][0]) == 5         # constant / light
        if recipe == 3:
            vals = [_int(v) for v in np.concatenate([a, b])]
            assert all(P <= v < 2**255 for v in vals) and P in vals and 2**255 - 1 in vals
        assert (tr[31] >= 0x80 and tr.any()) if recipe == 4 else not tr.any()
        if recipe == 5:
            assert c_over is not None and np.array_equal(d["c_in"][k], c_over) and not np.array_equal(c_over, ip)
        elif ip is not None:
            assert c_over is None and np.array_equal(d["c_in"][k], ip)
        assert np.array_equal(d["c_final"][k], oracle.fe_add(np.zeros(4, np.uint64), oracle.fe_mul(d["a"][k], d["b"][k])))
        if n == 1:   # no rounds: a, b are the inputs, x = 0
            assert np.array_equal(d["a"][k], a[0]) and np.array_equal(d["b"][k], b[0]) and not d["x"][k].any()


def test_regenerated_n8_cases_reproduce_the_fixture(golden):
    from oracle import pyoracle as po
    if not po.have_reference():
        try:
            po.build()
        except Exception:   # noqa: BLE001
            pass
    if not po.have_reference():
        pytest.skip("the reference build (oracle/_ref/libbpref.so) is not available")
    from make_ipa_prove import CASES, make_case, pack
    d = golden("ipa_prove")
    idx = [k for k, (n, _) in enumerate(CASES) if n == 8]
    R = po.Reference()
    got = pack([make_case(R, k, 8, CASES[k][1]) for k in idx])
    lo = d["L_off"]
    for key in ("a", "b", "x", "c_in", "c_final", "P", "check", "ok_in", "ok_final"):
        assert np.array_equal(got[key], d[key][idx]), key
    for key in ("L", "R"):
        assert np.array_equal(got[key], np.concatenate([d[key][lo[k]:lo[k + 1]] for k in idx])), key

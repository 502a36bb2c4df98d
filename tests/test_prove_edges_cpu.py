"""The conditions of tests/test_prove_edges_gpu.py, on the CPU: under the model of tests/prove_edges.py every
block reaches the path it was built for (scalar classes, prefix-table boundaries, uniform waves, empty work
lists), and the oracle accepts / refuses the inputs as the GPU tests assume.  A block that stops reaching
its path fails here.  The tallies asserted are printed (pytest -s shows them)."""
import numpy as np

import prove_edges as pe


def _ab_items(oracle):
    return [it for key in ("A", "B") for pr in pe.call(key) for it in pe.items(oracle, pr)]


def test_blocks_have_the_specified_sizes():
    A, B = pe.call("A"), pe.call("B")
    assert sum(p["tag"][2] in pe.E and p["tag"][1] != "ordinary" for p in A) == 180
    assert sum(p["tag"][1] == "ordinary" for p in A) == 87 and len(A) == 9 * 29 + 87
    assert [p["tag"][1] for p in A[:4]] == ["gamma", "gamma", "gamma", "ordinary"]
    assert len(B) == 60
    assert [len(pe.call(k)) for k in ("C1", "C2", "C8", "C64")] == [25, 25, 60, 60]
    assert [len(pe.call(k)) for k in ("D", "D255", "Ea", "Eb", "Ec", "Ed")] == [70, 70, 3, 5, 1, 65]
    for K, (lo, at, hi) in zip(pe.KS, zip(*[iter(pe.BOUNDARY)] * 3)):
        assert [pe.clz256(x) for x in (lo, at, hi)] == [K + 1, K, K - 1]


def test_every_slot_kind_meets_every_class(oracle):
    """A u B: sL, sR, gamma, alpha, rho each hold class 0, 1 and 2 items; a class-0 item that is non-zero as raw
    bytes (e = p in a canonicalised slot); e = p in a raw slot stays class 2."""
    tally = {k: [0, 0, 0] for k in pe.KINDS}
    zero_from_p = {k: 0 for k in pe.KINDS}
    for kind, s, raw in _ab_items(oracle):
        if kind in tally:
            tally[kind][pe.sclass(s)] += 1
            zero_from_p[kind] += raw == pe.P and pe.sclass(s) == 0
            if raw == pe.P:
                assert pe.sclass(s) == (2 if kind in pe.RAW_KINDS else 0), kind
    print("classes (constant, light, heavy) per slot kind:", tally)
    print("class-0 items with non-zero raw bytes (e = p):", zero_from_p)
    for kind in pe.KINDS:
        assert all(tally[kind]), (kind, tally[kind])
        assert (zero_from_p[kind] > 0) == (kind not in pe.RAW_KINDS), kind


def test_prefix_table_boundaries(oracle):
    """A u B, for each K: canonicalised scalars on both sides of clz = K (the table start and the dtab start) and at
    clz = K - 1, K and K + 1 exactly; among the raw alpha / rho scalars a prefix index with its top bit set (the
    tables' upper half, which only a raw scalar reaches) and a prefix index 0 (the dtab start)."""
    its = _ab_items(oracle)
    for K in pe.KS:
        canon = [s for kind, s, _ in its if kind not in pe.RAW_KINDS and s]
        raw = [s for kind, s, _ in its if kind in pe.RAW_KINDS]
        short, long_ = sum(pe.clz256(s) >= K for s in canon), sum(pe.clz256(s) < K for s in canon)
        at = {d: sum(pe.clz256(s) == K + d for s in canon) for d in (-1, 0, 1)}
        idx = [pe.prefix_index(s, K) for s in raw]
        top, zero = sum(i >> (K - 1) for i in idx), sum(i == 0 for i in idx)
        keys = sorted({pe.sm_ops_prefix(s, K) for s in canon + raw if pe.sclass(s) == 2})
        print(f"K = {K}: canonical clz >= K {short}, < K {long_}, at K-1/K/K+1 {at[-1]}/{at[0]}/{at[1]}; raw rows with "
              f"the top index bit {top}, index 0 {zero}; sort keys {keys[0]}..{keys[-1]} ({len(keys)} distinct)")
        assert short and long_ and all(at.values())
        assert top and zero
        assert keys[-1] == 512 - 2 * K              # 2^256 - 1 raw: the longest chain there is
    # without tables the raw 2^256 - 1 has the key 512, the last of the sort's 513 bins (MSM_BINS)
    assert max(pe.sm_ops_prefix(s, 0) for kind, s, _ in its if kind in pe.RAW_KINDS) == 512


def test_uniform_calls(oracle):
    """D: every heavy item of the first call holds the same 32 bytes, at least 128 of them, so after the 2n table
    lanes a full wave of the terms0 launch is uniform, on different bases.  The second call (2^255 + 1) has two
    heavy scalars: the raw 2^255 + 1 of alpha and rho, and 2^128 + 20 in sL, sR and gamma, which is what the
    reference's fe25519_tobytes makes of the limbs of 2^255 + 1 (not 20: its reduction is not the canonical
    one above 2^255).  The chain-length sort puts each scalar's items side by side, and with or without tables
    each of them fills at least one whole wave: the raw one at the tables' upper half (top index bit set)."""
    ls = pe.lists(oracle, pe.call("D"))
    print(f"D: heavy {len(ls['heavy'])}, light {len(ls['light'])}")
    assert set(ls["heavy"]) == {pe.D_HEAVY} and len(ls["heavy"]) >= 128
    assert pe.sclass(pe.D_HEAVY) == 2 and pe.clz256(pe.D_HEAVY) == 1 and pe.D_HEAVY not in pe.E
    raw, folded = 2**255 + 1, pe.canon(oracle, 2**255 + 1)
    ls = pe.lists(oracle, pe.call("D255"))
    print(f"D255: heavy {len(ls['heavy'])} ({ls['heavy'].count(raw)} raw 2^255+1, {ls['heavy'].count(folded)} of "
          f"tobytes(2^255+1) = {pe.name(folded)}), light {len(ls['light'])}")
    assert folded == 2**128 + 20 and set(ls["heavy"]) == {raw, folded} and ls["heavy"].count(raw) == 140 >= 128
    for K in (0,) + pe.KS:
        for key in ("D", "D255"):
            uw = pe.uniform_waves(oracle, pe.call(key), K)
            print(f"{key}, K = {K}: uniform full waves {({pe.name(s): c for s, c in uw.items()})}")
            assert all(c >= 1 for c in uw.values()) and set(uw) == ({pe.D_HEAVY} if key == "D" else {raw, folded})
        assert K == 0 or pe.prefix_index(raw, K) >> (K - 1) == 1


def test_degenerate_lists(oracle):
    ls = {k: pe.lists(oracle, pe.call(k)) for k in ("Ea", "Eb", "Ec", "Ed")}
    for k, v in ls.items():
        print(f"{k}: heavy {len(v['heavy'])}, light {len(v['light'])}, queued per proof {sorted(set(v['queued']))}")
    assert not ls["Ea"]["heavy"] and not ls["Ea"]["light"]
    assert not ls["Eb"]["heavy"] and len(ls["Eb"]["light"]) == 5 * (2 * 8 + 4)
    assert len(pe.call("Ec")) == 1 and ls["Ec"]["heavy"]
    assert [q == 0 for q in ls["Ed"]["queued"]] == [False] * 64 + [True]


def test_oracle_accepts_A_B_D_E(oracle):
    for key in ("A", "B", "D", "D255", "Ea", "Eb", "Ec", "Ed"):
        got = pe.oracle_proofs(oracle, key)
        assert all(w is not None for w in got), (key, [pe.call(key)[i]["tag"] for i, w in enumerate(got) if w is None])


def test_value_cross_patterns(oracle):
    """C: the oracle's valid pattern over the value list is the same under all five blindings; at n = 8 and n = 64
    at least 5 values are accepted and at least 5 refused."""
    for n in (1, 2, 8, 64):
        vals = pe.c_values(n)
        ok = np.array([w is not None for w in pe.oracle_proofs(oracle, f"C{n}")]).reshape(5, len(vals))
        print(f"n = {n}: valid over {[pe.name(v) for v in vals]}: {''.join('FT'[int(x)] for x in ok[0])}")
        assert (ok == ok[0]).all()
        assert ok[0].any() and not ok[0].all()
        if n >= 8:
            assert ok[0].sum() >= 5 and (~ok[0]).sum() >= 5


def test_refused_rows_are_the_documented_ones():
    """The header's statement for valid = 0, which the GPU test pins: identity points, everything else zero."""
    r = pe.refused_rows(8)
    assert all(r[k].tolist() == [0] * 4 + [1, 0, 0, 0] * 2 + [0] * 4 for k in ("V", "A", "S", "T1", "T2"))
    assert not any(r[k].any() for k in pe.FIELDS[5:]) and r["L"].shape == (3, 16) and pe.refused_rows(1)["L"].shape == (0, 16)


def test_verifier_batch_shape(oracle):
    ar, heads, tags, want = pe.verifier_batch(oracle)
    assert len(tags) == 187 and heads.shape == (187, 100)
    edited = [t for t in tags if t[1] != "untouched"]
    assert len(edited) == 140 and {t[1] for t in edited} == set(pe.V_FIELDS)
    ok = sum(w["ok"] for w in want)
    early = sum(not w["ok"] and not w["check"].any() for w in want)
    print(f"verifier batch: cuda verify accepts {ok}/187, early rejects {early}, std accepts {sum(w['ok_std'] for w in want)}")
    # the fold runs on edited a and b rows (c recomputed), and some edited rows end at the <a, b> != c reject
    ab = [p for p, t in enumerate(tags) if t[1] in ("a[0]", "b[0]")]
    assert any(want[p]["check"].any() for p in ab) and any(not want[p]["check"].any() for p in ab)


def test_point_golden_pins_raw_scalars(oracle, golden):
    """The oracle's ge_scalarmult takes the alpha / rho bytes raw.  tests/golden/point.npz (the reference's own
    ge25519_scalarmult, checked by test_oracle_golden.py) holds raw scalars with bit 255 set, the all-ones scalar
    and 0, on edge points; tests/golden/scalar_edges.npz adds every value of E on h itself."""
    sc = golden("point")["scalars"]
    assert not sc[0].any() and (sc[2] == 255).all()
    assert sum(int(s[31]) >> 7 for s in sc) >= 3
    assert [pe._int(s) for s in golden("scalar_edges")["scalars"]] == pe.E

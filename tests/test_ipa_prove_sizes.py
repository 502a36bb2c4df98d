"""GPU parity of the stand-alone IPA prover (hipbp_batch_inner_product_prove, its _gens and host
forms) at the lengths and element values tests/test_ipa_prove.py leaves out, against the reference's
own inner_product_prove outputs in tests/golden/ipa_prove_sizes.npz (make_ipa_prove_sizes.py; the
inputs are derived here by the same recipes): every power of two from 16 to the documented maximum
65536 that ipa_prove.npz lacks, elements with bit 255 set (2^256 - 1, 2p, the product gate's word at
and above MUL_BOUNDED_WORD), and zero / light / heavy scalars with their boundary values in every
block of a many-block work list.  Everything is bit-exact: this is integer arithmetic.

Measured wall time of the n >= 8192 tests on one MI355X (pytest's call durations; the inputs'
derivation, the upload and the compare included): one proof at n = 8192 0.12 s, 16384 0.23 s,
32768 0.46 s, 65536 0.87 s; n = 65536 at B = 3 0.70 s (its inputs are derived by then); the
n = 16 / 65536 / 16 regrowth test 0.70 s.  The chains are sequential in n and the times are linear
in it, 13 us per element.  No test is near 10 s, so 16384 and 32768 stay; the whole file takes 6 s.
"""
import os
import sys

import numpy as np
import pytest

from test_ipa_prove import OUT_KEYS, Env, tile
from test_ipa_prove_sizes_fixture import GRID_STRIDE_B, TERMS_LANES, n8_queued_per_chunk

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

NCASES = 15


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, k):
        v = self[k] = self.make(k)
        return v


class SizesEnv(Env):
    """test_ipa_prove's Env over ipa_prove_sizes.npz; inputs and generators are derived on first use
    (n = 65536: 131072 hashes, 8 MB of points per generator vector)."""

    def __init__(self, bp, golden, oracle):
        # (not Env.__init__: that one reads the older fixture and its case list)
        import torch
        from make_ipa_prove_sizes import CASE0, CASES, case_inputs, generators
        assert len(CASES) == NCASES
        self.bp, self.torch, self.oracle = bp, torch, oracle
        self.dev = torch.device("cuda:0")
        self.d = golden("ipa_prove_sizes")
        self.cases = CASES
        self.inp = _Lazy(lambda k: case_inputs(CASE0 + k, *CASES[k]))
        self.gen_np = _Lazy(lambda n: generators(oracle, n))
        self.gen = _Lazy(lambda n: tuple(self.T(x) for x in self.gen_np[n]))

    def of_recipe(self, n, *recipes):
        return [k for k, c in enumerate(self.cases) if c[0] == n and c[1] in recipes]


@pytest.fixture(scope="module")
def env(bp, golden, oracle):
    return SizesEnv(bp, golden, oracle)


@pytest.fixture(scope="module")
def old_env(bp, golden, oracle):
    return Env(bp, golden, oracle)


class _ws_budget:
    """HIPBP_IPA_WS_MB for the calls inside."""

    def __init__(self, mb):
        self.mb = str(mb)

    def __enter__(self):
        self.old = os.environ.get("HIPBP_IPA_WS_MB")
        os.environ["HIPBP_IPA_WS_MB"] = self.mb

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["HIPBP_IPA_WS_MB"]
        else:
            os.environ["HIPBP_IPA_WS_MB"] = self.old


# ----------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("case", range(NCASES))
def test_case_alone_matches_reference(env, case):
    """One proof per call: a, b, c, x, L, R, c_final bit for bit.  Cases 0 .. 10: n = 16, 16, 32, 128,
    512, 1024, 2048, 8192, 16384, 32768, 65536 (at 65536 round 0's 262146 items exceed k_ipa_terms'
    1024 x 256 lanes: the one length at which a single proof takes the grid-stride loop round again,
    and a 28 MB workspace); 11: a all zero at n = 512; 12, 13: every element >= 2^255 at n = 16, 512;
    14: zero, light and heavy scalars in every block at n = 512."""
    env.check(env.host(env.prove([case])), [case])


def test_wide_and_ordinary_proofs_share_waves_n16(env):
    """B = 67 tiles the three n = 16 cases in shuffled order: no multiple of a wave, and the proofs
    with every element >= 2^255 sit in the same waves as ordinary ones in every kernel."""
    idx = env.of_n(16)
    assert [env.cases[k][1] for k in idx] == [0, 0, 6]
    idx = tile([idx[p] for p in np.random.default_rng(16).permutation(len(idx))], 67)
    env.check(env.host(env.prove(idx)), idx)


def test_edge_cases_in_one_batch_n512(env):
    """The n = 512 cases in one call, shuffled: random, a all zero, wide, classes_blocks.  1026 items
    per proof in round 0; two chunks of two proofs, 2052 items and 9 blocks each."""
    idx = env.of_n(512)
    assert sorted(env.cases[k][1] for k in idx) == [0, 1, 6, 7]
    idx = [idx[p] for p in np.random.default_rng(512).permutation(len(idx))]
    env.check(env.host(env.prove(idx)), idx)


# ----------------------------------------------------------------------------- the grid stride
@pytest.mark.parametrize("B", [30000, GRID_STRIDE_B])
def test_many_short_proofs(old_env, B):
    """ipa_prove.npz's eight n = 8 cases tiled to B proofs, two chunks, every proof compared with the
    reference's outputs.  k_ipa_terms strides over the queued items (heavy, then light; zero scalars
    are k_ipa_scatter's constants), 112 + 14 per eight proofs in round 0.
    B = 30000: 270000 items a chunk, more than the 1024 x 256 = 262144 lanes in k_ipa_elem and
    k_ipa_scatter, but 236250 queued: k_ipa_terms' loop still takes one turn.
    B = 40000: 280000 heavy and 35000 light items a chunk, so the loop's second turn takes the last
    17856 slist entries and every llist entry, at i - ch with i >= 262144 (asserted from the inputs'
    classes)."""
    idx = tile(old_env.of_n(8), B)
    queued = n8_queued_per_chunk(old_env.oracle, B)
    assert len(queued) == 2
    if B == GRID_STRIDE_B:
        assert all(ch >= TERMS_LANES and cl > 0 for ch, cl in queued), queued
    got = old_env.host(old_env.prove(idx))
    want = old_env.want(idx)
    for k in OUT_KEYS:
        assert got[k].shape == want[k].shape, k
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(idx), -1).any(axis=1))
        assert not len(bad), f"{k}: {len(bad)} proofs differ from the reference, the first at {bad[:8].tolist()}"


def test_grid_stride_two_long_proofs_in_one_chunk(env):
    """n = 65536 at B = 3: chunks of two proofs and one.  The first has 524292 items in round 0, two
    full strides of k_ipa_terms and a remainder, with item ids above 2^18 per proof; all three
    outputs are the fixture's."""
    (k,) = env.of_n(65536)
    idx = [k, k, k]
    env.check(env.host(env.prove(idx)), idx)


# ----------------------------------------------------------------------------- workspaces
def test_workspace_regrowth_on_one_stream(env):
    """n = 16, then n = 65536, then n = 16 again on one fresh stream, nothing waited for in between:
    the stream's workspace grows from a few KB to 28 MB under the first call's queued work and is
    reused oversized by the third."""
    torch = env.torch
    small, (big,) = env.of_n(16), env.of_n(65536)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        o1 = env.prove(small, stream=s)
        o2 = env.prove([big], stream=s)
        o3 = env.prove(small[::-1], stream=s)
    env.check(env.host(o1), small)
    env.check(env.host(o2), [big])
    env.check(env.host(o3), small[::-1])
    env.bp.release_stream_workspaces(s)


def test_one_proof_per_chunk_n2048(env):
    """A 1 MB workspace budget at n = 2048 (0.85 MB per proof) holds one proof and no second: bmax = 1,
    so B = 3 runs as three chunks, the third in the first's workspace behind it."""
    (k,) = env.of_n(2048)
    with _ws_budget(1):
        got = env.host(env.prove([k, k, k]))
    env.check(got, [k, k, k])


# ----------------------------------------------------------------------------- generator sets
@pytest.mark.parametrize("n,bits,recipes", [(16, 6, (0, 6)), (512, 4, (1, 6, 7))])
def test_gens_form_has_the_plain_forms_bits(env, n, bits, recipes):
    """The prefix-table start of a scalar multiplication on scalars that come from wide elements and
    on the class boundaries: the same bits as the plain form and as the reference."""
    idx = env.of_recipe(n, *recipes)
    assert len(idx) == 3
    G, H, Q = env.gen[n]
    g = env.T(env.oracle.gh()[0])
    gens = env.bp.Generators(n, G, H, g, Q, prefix_bits=bits)
    try:
        with_tables = env.host(env.prove(idx, gens=gens))
    finally:
        gens.close()
    plain = env.host(env.prove(idx))
    for k in OUT_KEYS:
        assert np.array_equal(with_tables[k], plain[k]), k
    env.check(with_tables, idx)


# ----------------------------------------------------------------------------- host form
@pytest.mark.parametrize("n,recipe", [(16, 6), (512, 7)])
def test_host_form_matches_reference(env, n, recipe):
    """hipbp_inner_product_prove_host (through the numpy wrapper over it) on the n = 16 wide case and
    the n = 512 classes_blocks case."""
    (case,) = env.of_recipe(n, recipe)
    a, b, tr, _ = env.inp[case]
    G, H, Q = env.gen_np[n]
    w = env.bp.inner_product_prove(a, b, G, H, Q, env.d["c_in"][case], tr)
    want = env.want([case])
    Lr = n.bit_length() - 1
    assert w is not None and w["n"] == n and w["L_len"] == Lr
    for k in ("a", "b", "c", "x", "L", "R"):
        assert np.array_equal(np.asarray(w[k], np.uint64), want[k][0]), k


# ----------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("n", [16, 32, 128, 512, 1024, 2048])
def test_round_trip_through_the_verifier(env, n):
    """Every case with has_verify: prove -> P = msm_batch(a || b, G || H) -> batch_inner_product_verify
    with c_final and with c: P, the verdicts and the check point are the reference's.  The wide cases
    hand the MSM scalars and the verifier a final a, b with bit 255 set."""
    torch, bp, d = env.torch, env.bp, env.d
    idx = env.of_n(n)
    assert all(d["has_verify"][idx])
    B = len(idx)
    a, b, _, _ = env.inputs(idx)
    G, H, Q = env.gen[n]
    out = env.prove(idx)
    P = torch.zeros(B, 16, dtype=torch.int64, device=env.dev)
    bp.msm_batch(P, torch.cat([a, b], dim=1).contiguous(), torch.cat([G, H]).contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(P.cpu().numpy().view(np.uint64), d["P"][idx])
    for which, want_ok in (("c_final", d["ok_final"][idx]), ("c", d["ok_in"][idx])):
        batch = bp.ipa_proof_batch(n, out, c=which)
        ok = torch.zeros(B, dtype=torch.uint8, device=env.dev)
        chk = torch.zeros(B, 16, dtype=torch.int64, device=env.dev)
        bp.batch_inner_product_verify(batch, P, G, H, Q, ok, chk)
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy().astype(bool), want_ok.astype(bool)), which
        if which == "c_final":
            assert np.array_equal(chk.cpu().numpy().view(np.uint64), d["check"][idx])


def test_every_verifiable_case_is_in_the_round_trip(env):
    ns = sorted({n for (n, _), v in zip(env.cases, env.d["has_verify"]) if v})
    assert ns == [16, 32, 128, 512, 1024, 2048]

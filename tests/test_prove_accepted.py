"""The accepted prover on the GPU: batch_generate_range_proof_accepted against the CPU
restatement run attempt by attempt (tests/prove_try_ref.py for the scalars, the oracle's
generate_range_proof and its two verifiers for the verdicts), against the explicit prover fed with
derive_prover_scalars_at, and against the library's own batched verify; max_attempts 1 and 2, split
invariance, the selection over several blocks, derive_prover_scalars_at against hashlib, the
argument errors and the workspace release."""
import ctypes

import numpy as np
import pytest

import prove_seed_ref as ref
import prove_try_ref as tref
from test_prove_seeded import KEYS, SEED, inputs, same

pytestmark = pytest.mark.gpu

IB = 7   # index_base of every call here


@pytest.fixture(scope="module")
def T():
    import torch
    dev = torch.device("cuda:0")
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


@pytest.fixture(scope="module")
def gens_for(oracle):
    cache = {}

    def get(n):
        if n not in cache:
            g, h = oracle.gh()
            cache[n] = (oracle.base_points(n, 1), oracle.base_points(n, 2), g, h)
        return cache[n]
    return get


def oracle_attempts(oracle, n, v, gamma, gens, check, max_attempts=8, index_base=IB):
    """The expected attempts vector: per proof, attempt by attempt, key -> try key -> scalars ->
    generate_range_proof -> the verifier of `check`; 0 for a refused value or no accepted attempt."""
    G, H, g, h = gens
    verify = oracle.cuda_range_proof_verify if check == 1 else oracle.range_proof_verify
    out = np.zeros(len(v), np.uint8)
    for p in range(len(v)):
        kp = ref.key(SEED, v[p], gamma[p], index_base + p, n)
        for a in range(max_attempts):
            sc = tref.scalars(tref.try_key(kp, a), n)
            sLR = np.concatenate([sc["sL"].view(np.uint8).reshape(n, 32), sc["sR"].view(np.uint8).reshape(n, 32)], axis=1)
            pr = oracle.generate_range_proof(v[p].view(np.uint8), gamma[p].view(np.uint8), sLR,
                                             sc["rnd"].view(np.uint8).reshape(4, 32), n, G, H, g, h)
            if pr is None:
                break
            if verify(pr["head"], pr["V"], n, pr["a"], pr["b"], pr["L"], pr["R"], G, H, g, h)[0]:
                out[p] = a + 1
                break
    return out


@pytest.fixture(scope="module")
def batch8(oracle, gens_for):
    """n = 8, B = 70, default_rng(rs), proof 17 refused, with the oracle's attempts under check 1,
    computed once per rs.  70 proofs: two waves of the selection's block, the second partly idle.
    rs = 3: 63 ones, 6 twos, a zero at 17.  rs = 10: 61 ones, 6 twos, threes at proofs 4 and 56 (so
    its round 3 selects from a compact list), a zero at 17."""
    cache = {}

    def get(rs):
        if rs not in cache:
            n, B = 8, 70
            v, gamma = inputs(B, n, np.random.default_rng(rs), refuse=17)
            cache[rs] = (n, B, v, gamma, oracle_attempts(oracle, n, v, gamma, gens_for(n), 1))
        return cache[rs]
    return get


@pytest.fixture(scope="module")
def case8(batch8):
    """The batch with third attempts (default_rng(10))."""
    n, B, v, gamma, want = batch8(10)
    assert np.flatnonzero(want == 3).tolist() == [4, 56] and want.max() == 3
    return n, B, v, gamma, want


def accepted_equals_explicit(bp, T, n, vd, gd, G, H, g, h, o, gens=None, index_base=IB):
    """Every output tensor of `o` equals the explicit prover on the scalars of the attempt that `o`
    reports (attempt index max(attempts, 1) - 1: the last one tried for the proofs never accepted
    is the caller's to pass)."""
    import torch
    att = (torch.clamp(o["attempts"], min=1) - 1).to(torch.uint8)
    sc = bp.derive_prover_scalars_at(n, vd, gd, SEED, attempt=att, index_base=index_base)
    e = bp.batch_generate_range_proof(n, vd, gd, sc["sL"], sc["sR"], sc["rnd"], G, H, g, h, gens=gens)
    torch.cuda.synchronize()
    same(o, e)


@pytest.mark.parametrize("with_gens", [False, True])
@pytest.mark.parametrize("rs", [3, 10])
def test_accepted_equals_oracle(bp, T, oracle, gens_for, batch8, rs, with_gens):
    """attempts equals the oracle's vector; every output tensor equals batch_generate_range_proof on
    derive_prover_scalars_at(attempt = max(attempts, 1) - 1), bit for bit; batch_range_proof_verify
    of the result gives ok == (attempts > 0) on every valid proof (the refused value's zeroed proof
    has attempts 0 by definition, but both of the reference's verifiers accept it: its verdict is
    checked against the oracle's).  Plain and with a Generators set at prefix_bits = 8.
    The condition of the test, so that it cannot pass on nothing: retries happen, in the rs = 10
    batch a third attempt too, and every proof converges within 8.  (default_rng(3) is the batch
    the feature was specified with; the oracle finds no third attempt in it, hence the second batch.)"""
    import torch
    n, B, v, gamma, want = batch8(rs)
    assert (want == 2).any() and want.max() <= 8
    assert (want == 3).any() or rs != 10
    assert np.flatnonzero(want == 0).tolist() == [17]
    G, H, g, h = (T(x) for x in gens_for(n))
    gens = bp.Generators(n, G, H, g, h, prefix_bits=8) if with_gens else None
    vd, gd = T(v), T(gamma)
    o = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, max_attempts=8, check=1,
                                               gens=gens)
    assert np.array_equal(o["attempts"].cpu().numpy(), want)
    assert o["valid"].cpu().numpy().tolist() == [int(p != 17) for p in range(B)]
    accepted_equals_explicit(bp, T, n, vd, gd, G, H, g, h, o, gens=gens)
    ok = torch.zeros(B, dtype=torch.uint8, device=G.device)
    bp.batch_range_proof_verify(bp.RangeProofBatch(n, **{k: o[k] for k in bp.RangeProofBatch.FIELDS}), G, H, g, h, ok)
    torch.cuda.synchronize()
    okn, att = ok.cpu().numpy() != 0, o["attempts"].cpu().numpy()
    valid = np.arange(B) != 17
    assert np.array_equal(okn[valid], att[valid] > 0)
    d = {k: o[k][17].cpu().numpy().view(np.uint64) for k in KEYS if k != "valid"}
    head = np.concatenate([d[k] for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")])
    assert not head[[i for i in range(100) if i % 16 not in (4, 8) or i >= 80]].any()   # the zeroed proof
    assert okn[17] == oracle.cuda_range_proof_verify(head, d["V"], n, d["a"], d["b"], d["L"], d["R"], *gens_for(n))[0]
    if gens is not None:
        gens.close()


def test_one_attempt_is_the_seeded_prover(bp, T, gens_for, case8):
    """max_attempts = 1: the seeded prover's output in every tensor, attempts = the plain verify's
    verdicts where valid (the verifier accepts the refused value's zeroed proof; its attempts is 0)."""
    import torch
    n, B, v, gamma, want = case8
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    o = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, max_attempts=1)
    s = bp.batch_generate_range_proof_seeded(n, vd, gd, SEED, G, H, g, h, index_base=IB)
    ok = torch.zeros(B, dtype=torch.uint8, device=G.device)
    bp.batch_range_proof_verify(bp.RangeProofBatch(n, **{k: s[k] for k in bp.RangeProofBatch.FIELDS}), G, H, g, h, ok)
    torch.cuda.synchronize()
    same(o, s)
    assert int(ok[17]) == 1 and int(s["valid"][17]) == 0
    assert torch.equal(o["attempts"], ok * s["valid"])
    assert np.array_equal(o["attempts"].cpu().numpy(), (want == 1).astype(np.uint8))


def test_two_attempts_keep_the_last_proof(bp, T, gens_for, case8):
    """max_attempts = 2: the proofs that need a third attempt (4 and 56) end with attempts 0, valid 1
    and the proof of attempt index 1; every other proof as with max_attempts = 8."""
    import torch
    n, B, v, gamma, want = case8
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    o = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, max_attempts=2)
    w2 = np.where(want <= 2, want, 0).astype(np.uint8)
    assert np.array_equal(o["attempts"].cpu().numpy(), w2)
    assert int(o["valid"][4]) == 1 and int(o["valid"][56]) == 1
    att = torch.from_numpy(np.where(want >= 2, 1, 0).astype(np.uint8)).to(G.device)   # index 1 where a retry ran
    sc = bp.derive_prover_scalars_at(n, vd, gd, SEED, attempt=att, index_base=IB)
    e = bp.batch_generate_range_proof(n, vd, gd, sc["sL"], sc["sR"], sc["rnd"], G, H, g, h)
    torch.cuda.synchronize()
    same(o, e)


def test_split_invariance(bp, T, gens_for, case8):
    """The 70 proofs in calls of 23 and 47, each with its own index_base, give the proofs and the
    attempts of the single call."""
    import torch
    n, B, v, gamma, want = case8
    G, H, g, h = (T(x) for x in gens_for(n))
    run = lambda lo, hi: bp.batch_generate_range_proof_accepted(n, T(v[lo:hi]), T(gamma[lo:hi]), SEED, G, H, g, h,
                                                                index_base=IB + lo)
    whole, lo, hi = run(0, B), run(0, 23), run(23, B)
    assert np.array_equal(whole["attempts"].cpu().numpy(), want)
    for k in KEYS + ("attempts",):
        assert torch.equal(whole[k], torch.cat([lo[k], hi[k]])), k


def test_selection_over_several_blocks(bp, T, gens_for):
    """B = 600 at n = 8 (three blocks of the selection, the last partly idle, refused values in two of
    them): one call equals calls of 256, 256 and 88 proofs, each of which selects within one block,
    and the explicit prover on the reported attempts' scalars.  Retries occur in every part."""
    import torch
    n, B = 8, 600
    v, gamma = inputs(B, n, np.random.default_rng(11), refuse=300)
    v[599, 0] |= np.uint64(1 << n)
    G, H, g, h = (T(x) for x in gens_for(n))
    run = lambda lo, hi: bp.batch_generate_range_proof_accepted(n, T(v[lo:hi]), T(gamma[lo:hi]), SEED, G, H, g, h,
                                                                index_base=IB + lo)
    whole = run(0, B)
    parts = [run(0, 256), run(256, 512), run(512, B)]
    for k in KEYS + ("attempts",):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    att = whole["attempts"].cpu().numpy()
    assert all((p["attempts"] >= 2).any() for p in parts)
    assert np.flatnonzero(whole["valid"].cpu().numpy() == 0).tolist() == [300, 599]
    assert att[300] == 0 and att[599] == 0
    accepted_equals_explicit(bp, T, n, T(v), T(gamma), G, H, g, h, whole)


@pytest.mark.parametrize("n", [1, 8, 64])
def test_derive_at_equals_hashlib(bp, T, n):
    """derive_prover_scalars_at bit for bit at B = 5, attempts [0, 1, 2, 0, 255]; attempt=None equals
    derive_prover_scalars."""
    import torch
    B = 5
    v, gamma = inputs(B, n, np.random.default_rng(n))
    att = np.array([0, 1, 2, 0, 255], np.uint8)
    want = tref.derive_at(SEED, v, gamma, IB, n, att)
    vd, gd = T(v), T(gamma)
    got = bp.derive_prover_scalars_at(n, vd, gd, SEED, attempt=torch.from_numpy(att).to(vd.device), index_base=IB)
    none = bp.derive_prover_scalars_at(n, vd, gd, SEED, index_base=IB)
    plain = bp.derive_prover_scalars(n, vd, gd, SEED, index_base=IB)
    torch.cuda.synchronize()
    for k in ("rnd", "sL", "sR"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint64), want[k]), k
        assert torch.equal(none[k], plain[k]), k


@pytest.mark.parametrize("check", [1, 2])
@pytest.mark.parametrize("rs", [564, 566])
def test_n64_both_checks(bp, T, oracle, gens_for, rs, check):
    """n = 64, B = 24, default_rng(rs), no refused value, against the oracle under
    cuda_range_proof_verify (check 1) and range_proof_verify (check 2) semantics; the proofs equal
    the explicit prover's on the reported attempts.  rs = 566: a second attempt at proof 14 under
    check 1 and at proof 9 under check 2, asserted.  (default_rng(564) is the batch the feature was
    specified with; the oracle accepts all of its first attempts under both checks.)"""
    n, B = 64, 24
    v, gamma = inputs(B, n, np.random.default_rng(rs))
    want = oracle_attempts(oracle, n, v, gamma, gens_for(n), check)
    assert want.min() >= 1 and ((want == 2).any() or rs != 566)
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    o = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, check=check)
    assert np.array_equal(o["attempts"].cpu().numpy(), want)
    accepted_equals_explicit(bp, T, n, vd, gd, G, H, g, h, o)


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("check", [1, 2])
def test_gens_matches_plain_both_checks(bp, T, gens_for, check, bits):
    """The accepted prover on a Generators set == the plain call on the same four generators, bit for
    bit: every output tensor and attempts, under check 1 and check 2, without tables and with 4-bit
    ones (the check-1 verify then takes them too).  n = 4, 3 proofs: the smallest shape with L, R
    rounds and with tables; a set whose g and h were swapped on the way gives other proofs.  The three
    values are 0, the one value validate_range_input admits at n = 4 (for n % 8 != 7 it wants byte
    n / 8 of the value and every byte above it zero); the proofs differ by their gamma and index."""
    import torch
    n, B = 4, 3
    v, gamma = inputs(B, n, np.random.default_rng(41))
    v[:] = 0
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    plain = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, check=check)
    gens = bp.Generators(n, G, H, g, h, prefix_bits=bits)
    got = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, check=check, gens=gens)
    torch.cuda.synchronize()
    assert plain["valid"].cpu().numpy().all()   # (proofs were made: no value of the batch is refused)
    assert torch.equal(got["attempts"], plain["attempts"])
    same(got, plain)
    gens.close()


def test_argument_errors_write_nothing(bp, T, gens_for):
    """max_attempts 0 and 17, check 3, a non-NULL sL and a null attempts give HIPBP_ERR_ARG and write
    nothing; count = 0 returns HIPBP_OK."""
    import torch
    B, n = 4, 8
    v, gamma = inputs(B, n, np.random.default_rng(1))
    vd, gd = T(v), T(gamma)
    G, H, g, h = (T(x) for x in gens_for(n))
    L = bp.lib()
    c = lambda t: ctypes.c_void_p(t.data_ptr())
    sd = (ctypes.c_uint8 * 32).from_buffer_copy(SEED)
    FILL = 0x5A5A5A5A5A5A5A5A
    fresh = lambda *shape: torch.full(shape, FILL, dtype=torch.int64, device=vd.device)

    def call(max_attempts=8, check=1, sL=None, attempts=True, count=B):
        out = {k: fresh(B, 16) for k in ("V", "A", "S", "T1", "T2")}
        out.update({k: fresh(B, 4) for k in ("taux", "mu", "t", "c", "x", "a", "b")})
        out.update(L=fresh(B, 3, 16), R=fresh(B, 3, 16), valid=torch.full((B,), 0x5A, dtype=torch.uint8, device=vd.device))
        att = torch.full((B,), 0x5A, dtype=torch.uint8, device=vd.device)
        ic = bp.ProveInputC(count, n, vd.data_ptr(), gd.data_ptr(), sL.data_ptr() if sL is not None else None, None, None)
        oc = bp.ProofOutC(*[out[k].data_ptr() for k in KEYS])
        rc = L.hipbp_batch_generate_range_proof_accepted(ctypes.byref(ic), sd, ctypes.c_uint64(0), ctypes.c_int(max_attempts),
                                                         ctypes.c_int(check), c(G), c(H), c(g), c(h), ctypes.byref(oc),
                                                         c(att) if attempts else None, None)
        torch.cuda.synchronize()
        assert all(bool((t == (0x5A if k == "valid" else FILL)).all()) for k, t in out.items())
        assert bool((att == 0x5A).all())
        return rc

    assert call(max_attempts=0) == 1   # HIPBP_ERR_ARG
    assert call(max_attempts=17) == 1
    assert call(check=3) == 1
    assert call(sL=fresh(B, 8, 4)) == 1
    assert call(attempts=False) == 1
    assert call(count=0) == 0
    with pytest.raises(bp.BulletproofError):
        bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, max_attempts=0)
    with pytest.raises(ValueError):
        bp.batch_generate_range_proof_accepted(n, vd, gd, SEED[:31], G, H, g, h)


def test_release_then_same_bits(bp, T, gens_for, case8):
    """release_stream_workspaces after a call frees the retry workspace with the rest; a second call
    on the same stream rebuilds it and gives the same bits."""
    import torch
    n, B, v, gamma, want = case8
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    st = torch.cuda.Stream(G.device)
    torch.cuda.synchronize()
    o0 = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, stream=st)
    bp.release_stream_workspaces(st)
    o1 = bp.batch_generate_range_proof_accepted(n, vd, gd, SEED, G, H, g, h, index_base=IB, stream=st)
    bp.release_stream_workspaces(st)
    for k in KEYS + ("attempts",):
        assert torch.equal(o0[k], o1[k]), k
    assert np.array_equal(o1["attempts"].cpu().numpy(), want)

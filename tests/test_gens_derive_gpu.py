"""Generators derived from seeds on the GPU.  Everything is bit-exact: the device calls
against the host calls (which tests/test_gens_derive_cpu.py holds to hashlib and the CPU restatement's
fe_mul), Generators.from_seeds against the reference-emitted generators of the golden proof sets, and
a seeded set against an uploaded one through the verifier, the prover and the MSM."""
import ctypes

import numpy as np
import pytest

import gens_derive_ref as gr

pytestmark = pytest.mark.gpu

SENT = -0x1111111111111112   # 0xEEEE... as int64
SEED = bytes(range(7, 39))


def _u(t):
    return t.cpu().numpy().view(np.uint64)


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda:0")


# ---------------------------------------------------------------- device == host
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_at_wave_and_block_edges(bp, count):
    """Each count into a buffer one point longer, whose last point keeps its sentinel."""
    import torch
    buf = torch.full((count + 1, 16), SENT, dtype=torch.int64, device="cuda:0")
    got = bp.derive_base_points(SEED, count, out=buf[:count])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(_u(buf[:count]), bp.derive_base_points_host(SEED, count))
    assert (buf[count] == SENT).all()


@pytest.mark.parametrize("first,count", gr.CARRIES + [gr.LAST_BLOCK, (2**32 - 257, 257)])
def test_index_carries_and_the_last_block(bp, first, count):
    import torch
    for seed in (SEED, b"\xff" * 32, bytes(32)):
        got = bp.derive_base_points(seed, count, first=first)
        torch.cuda.synchronize()
        assert got.shape == (count, 16) and got.dtype == torch.int64
        assert np.array_equal(_u(got), bp.derive_base_points_host(seed, count, first))


def test_split_call_and_a_stream_of_ones_own(bp):
    import torch
    whole = bp.derive_base_points_host(SEED, 1000)
    buf = torch.full((1000, 16), SENT, dtype=torch.int64, device="cuda:0")
    bp.derive_base_points(SEED, 300, out=buf[:300])
    bp.derive_base_points(SEED, 700, first=300, out=buf[300:])
    torch.cuda.synchronize()
    assert np.array_equal(_u(buf), whole)
    st = torch.cuda.Stream()
    got = bp.derive_base_points(SEED, 1000, stream=st)
    one = bp.derive_single_point(SEED, stream=st)
    st.synchronize()
    assert np.array_equal(_u(got), whole)
    assert np.array_equal(_u(one), bp.derive_single_point_host(SEED))


def test_single_points(bp, golden):
    import torch
    d = golden("proofs_n16")
    for k in ("G", "H", "g", "h"):
        p = bp.derive_single_point(bp.REFERENCE_SEEDS[k])
        torch.cuda.synchronize()
        assert np.array_equal(_u(p), bp.derive_single_point_host(bp.REFERENCE_SEEDS[k])), k
    assert np.array_equal(_u(bp.derive_single_point(3)), d["g"]) and np.array_equal(_u(bp.derive_single_point(4)), d["h"])
    p = _u(bp.derive_single_point(gr.BIT255_SEED))
    assert np.array_equal(p, bp.derive_single_point_host(gr.BIT255_SEED))
    assert int(p[3]) >> 63 == 1 and not np.array_equal(p[12:16], p[0:4])   # T = X * 1, not X


# ---------------------------------------------------------------- Generators.from_seeds
@pytest.mark.parametrize("n", [1, 16, 64])
def test_from_seeds_points(bp, golden, n):
    import torch
    gens = bp.Generators.from_seeds(n)
    try:
        assert (gens.n, gens.bits) == (n, 0)
        G, H, g, h = (_u(t) for t in gens.points())
        if n == 1:
            want = (bp.derive_base_points_host(1, 1), bp.derive_base_points_host(2, 1), bp.derive_single_point_host(3),
                    bp.derive_single_point_host(4))
        else:
            d = golden(f"proofs_n{n}")
            want = (d["G"], d["H"], d["g"], d["h"])
        for got, w in zip((G, H, g, h), want):
            assert np.array_equal(got, w)
    finally:
        gens.close()
    # seeds of the caller's own, one in each form, and a non-default stream
    st = torch.cuda.Stream()
    gens = bp.Generators.from_seeds(n, seed_G=SEED, seed_H=9, seed_g=b"\xff" * 32, seed_h=gr.BIT255_SEED, stream=st)
    try:
        G, H, g, h = (_u(t) for t in gens.points())
        assert np.array_equal(G, bp.derive_base_points_host(SEED, n)) and np.array_equal(H, bp.derive_base_points_host(9, n))
        assert np.array_equal(g, bp.derive_single_point_host(b"\xff" * 32))
        assert np.array_equal(h, bp.derive_single_point_host(gr.BIT255_SEED))
    finally:
        gens.close()


def test_points_of_an_uploaded_set(bp):
    rng = np.random.default_rng(5)
    up = [rng.integers(0, 2**64, size=s, dtype=np.uint64) for s in ((16, 16), (16, 16), (16,), (16,))]
    gens = bp.Generators(16, *[_T(a) for a in up], prefix_bits=4)
    try:
        for got, w in zip(gens.points(), up):
            assert np.array_equal(_u(got), w)
    finally:
        gens.close()


# ---------------------------------------------------------------- the same bits downstream
@pytest.mark.parametrize("K", [0, 8])
def test_seeded_set_downstream(bp, golden, K):
    """n = 64: the golden batch through batch_range_proof_verify_gens, 8 proofs from the prover and two
    canonical MSM rows, on a seeded set and on an uploaded one: the same outputs (with K = 8 they come
    through the prefix tables, so the tables agree too), and the recorded verdicts, P and check points."""
    import torch
    from cudabulletproof_amd import synth
    from oracle import pyoracle
    n = 64
    d = golden("proofs_n64")
    dev = torch.device("cuda:0")
    seeded = bp.Generators.from_seeds(n, prefix_bits=K)
    uploaded = bp.Generators(n, _T(d["G"]), _T(d["H"]), _T(d["g"]), _T(d["h"]), prefix_bits=K)
    try:
        hs = [pyoracle.head_fields(h) for h in d["head"]]
        ref = dict(V=d["V"], A=np.stack([h["A"] for h in hs]), S=np.stack([h["S"] for h in hs]),
                   T1=np.stack([h["T1"] for h in hs]), T2=np.stack([h["T2"] for h in hs]),
                   t=np.stack([h["t"] for h in hs]), a=d["a"], b=d["b"], c=np.stack([h["c"] for h in hs]),
                   x=np.stack([h["x"] for h in hs]), L=d["L"], R=d["R"])
        batch = bp.RangeProofBatch.from_numpy(n, ref, dev)
        outs = []
        for gens in (seeded, uploaded):
            ok = torch.zeros(batch.count, dtype=torch.uint8, device=dev)
            P = torch.zeros(batch.count, 16, dtype=torch.int64, device=dev)
            chk = torch.zeros(batch.count, 16, dtype=torch.int64, device=dev)
            bp.batch_range_proof_verify_gens(batch, gens, ok, P, chk)
            torch.cuda.synchronize()
            outs.append((ok.cpu(), P.cpu(), chk.cpu()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert np.array_equal(outs[0][0].numpy().astype(bool), d["ok_cuda"].astype(bool))
        assert np.array_equal(outs[0][1].numpy().view(np.uint64), d["P"])
        assert np.array_equal(outs[0][2].numpy().view(np.uint64), d["check"])

        pi = synth.prove_inputs(8, n, seed=19)
        args = [_T(pi[k]) for k in ("v", "gamma", "sL", "sR", "rnd")]
        o0 = bp.batch_generate_range_proof(n, *args, None, None, None, None, gens=seeded)
        o1 = bp.batch_generate_range_proof(n, *args, None, None, None, None, gens=uploaded)
        torch.cuda.synchronize()
        for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R", "valid"):
            assert torch.equal(o0[k], o1[k]), k
        assert int(o0["valid"].sum()) > 0

        s = _T(synth._rand_fe(np.random.default_rng(64 + K), (2 * 2 * n,)))
        r0 = torch.zeros(2, 16, dtype=torch.int64, device=dev)
        r1 = torch.zeros(2, 16, dtype=torch.int64, device=dev)
        bp.msm_batch_gens(r0, s, seeded)
        bp.msm_batch_gens(r1, s, uploaded)
        torch.cuda.synchronize()
        assert torch.equal(r0, r1) and bool((r0 != 0).any())
    finally:
        seeded.close()
        uploaded.close()


# ---------------------------------------------------------------- size
def test_largest_set(bp):
    """from_seeds(65536) without tables: all 131 074 points equal the host derivation."""
    gens = bp.Generators.from_seeds(65536)
    try:
        G, H, g, h = (_u(t) for t in gens.points())
    finally:
        gens.close()
    assert np.array_equal(G, bp.derive_base_points_host(1, 65536))
    assert np.array_equal(H, bp.derive_base_points_host(2, 65536))
    assert np.array_equal(g, bp.derive_single_point_host(3)) and np.array_equal(h, bp.derive_single_point_host(4))


def test_the_msm_inputs_last_rows(bp):
    import torch
    from cudabulletproof_amd import synth
    lo = 2**20 - 4096
    _, pts = synth.msm_config3(lo, 2**20, torch.device("cuda:0"))
    got = bp.derive_base_points(5, 4096, first=lo)
    torch.cuda.synchronize()
    assert np.array_equal(_u(got), pts)


# ---------------------------------------------------------------- errors
def test_errors(bp):
    import torch
    out = torch.full((4, 16), SENT, dtype=torch.int64, device="cuda:0")
    with pytest.raises(bp.BulletproofError, match="2\\^32"):
        bp.derive_base_points(SEED, 4, first=2**32 - 3, out=out)
    with pytest.raises(bp.BulletproofError):
        bp.derive_base_points(SEED, 4, first=2**32, out=out)
    with pytest.raises(bp.BulletproofError):
        bp.derive_base_points(None, 4, out=out)
    with pytest.raises(bp.BulletproofError):
        bp.derive_single_point(None)
    with pytest.raises(ValueError):
        bp.derive_base_points(SEED, 3, out=out)
    for n in (0, 3, 2 * 65536):
        with pytest.raises(bp.BulletproofError, match="bad n"):
            bp.Generators.from_seeds(n)
    with pytest.raises(bp.BulletproofError, match="prefix bits"):
        bp.Generators.from_seeds(16, prefix_bits=25)
    L = bp.lib()
    sd = bp._gen_seed(1)
    assert L.hipbp_gens_create_seeded(ctypes.c_size_t(16), sd, None, sd, sd, 0, None) is None
    assert L.hipbp_gens_copy_points(None, None, None, None, None, None, None, None) == 1
    torch.cuda.synchronize()
    assert (out == SENT).all()
    bp.derive_base_points(SEED, 0, first=2**32, out=out[:0])   # nothing to write: fine
    torch.cuda.synchronize()
    assert (out == SENT).all()

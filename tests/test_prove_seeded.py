"""The seeded prover on the GPU: derive_prover_scalars against its hashlib restatement
(tests/prove_seed_ref.py), batch_generate_range_proof_seeded against the explicit prover fed with the
derived scalars, split invariance, binding, the host entry point and the argument errors."""
import ctypes
import os

import numpy as np
import pytest

import prove_seed_ref as ref

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
KEYS = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R", "valid")


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


def inputs(B, n, rng, refuse=None):
    """v (B,4): values below 2^n (proof `refuse` has bit n set: validate_range_input refuses it);
    gamma (B,4): four random limbs, unmasked (the key binds them as stored)."""
    v = np.zeros((B, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << min(n, 62), B, dtype=np.uint64)
    if refuse is not None:
        assert n < 64
        v[refuse, 0] |= np.uint64(1 << n)
    gamma = rng.integers(0, 1 << 63, (B, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (B, 4), dtype=np.uint64)
    return v, gamma


def same(o0, o1, rows=None):
    import torch
    for k in KEYS:
        a, b = (o0[k], o1[k]) if rows is None else (o0[k][rows], o1[k][rows])
        assert torch.equal(a, b), k


@pytest.mark.parametrize("index_base", [0, 2**32 - 2])
@pytest.mark.parametrize("n", [1, 8, 64])
def test_derivation_equals_hashlib(bp, T, n, index_base):
    """derive_prover_scalars bit for bit: B = 5 (660 lanes at n = 64: several blocks and waves, a last
    block partly idle); index_base 2^32 - 2 puts the carry into LE64's high word inside the batch."""
    import torch
    B = 5
    v, gamma = inputs(B, n, np.random.default_rng(n))
    want = ref.derive(SEED, v, gamma, index_base, n)
    got = bp.derive_prover_scalars(n, T(v), T(gamma), SEED, index_base=index_base)
    torch.cuda.synchronize()
    for k in ("rnd", "sL", "sR"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint64), want[k]), k


@pytest.mark.parametrize("with_gens", [False, True])
@pytest.mark.parametrize("n", [1, 8, 64])
def test_seeded_equals_explicit(bp, T, gens_for, n, with_gens):
    """batch_generate_range_proof_seeded = batch_generate_range_proof on the derived scalars, every
    output tensor including valid; B = 33 with one refused value where n < 64; plain and with a
    Generators set at prefix_bits = 8."""
    import torch
    B = 33
    v, gamma = inputs(B, n, np.random.default_rng(100 + n), refuse=17 if n < 64 else None)
    G, H, g, h = (T(x) for x in gens_for(n))
    gens = bp.Generators(n, G, H, g, h, prefix_bits=8) if with_gens else None
    vd, gd = T(v), T(gamma)
    sc = bp.derive_prover_scalars(n, vd, gd, SEED, index_base=7)
    o0 = bp.batch_generate_range_proof(n, vd, gd, sc["sL"], sc["sR"], sc["rnd"], G, H, g, h, gens=gens)
    o1 = bp.batch_generate_range_proof_seeded(n, vd, gd, SEED, G, H, g, h, index_base=7, gens=gens)
    torch.cuda.synchronize()
    same(o0, o1)
    if n < 64:
        assert int(o1["valid"][17]) == 0
    if n >= 8:
        assert int(o1["valid"].sum()) == B - (1 if n < 64 else 0)
    if gens is not None:
        gens.close()


@pytest.mark.parametrize("bits", [0, 4])
def test_seeded_gens_matches_plain_seeded(bp, T, gens_for, bits):
    """The seeded prover on a Generators set == the plain seeded call on the same four generators, bit
    for bit, without tables and with 4-bit ones: n = 4, 3 proofs, the smallest shape with L, R rounds
    and with tables (the test above hands the set to both of its sides, where a g/h swap inside the
    set's view would cancel).  The values are 0, the one value validate_range_input admits at n = 4."""
    import torch
    n, B = 4, 3
    v, gamma = inputs(B, n, np.random.default_rng(42))
    v[:] = 0
    G, H, g, h = (T(x) for x in gens_for(n))
    vd, gd = T(v), T(gamma)
    plain = bp.batch_generate_range_proof_seeded(n, vd, gd, SEED, G, H, g, h, index_base=7)
    gens = bp.Generators(n, G, H, g, h, prefix_bits=bits)
    got = bp.batch_generate_range_proof_seeded(n, vd, gd, SEED, G, H, g, h, index_base=7, gens=gens)
    torch.cuda.synchronize()
    assert plain["valid"].cpu().numpy().all()   # (proofs were made)
    same(got, plain)
    gens.close()


def test_split_invariance(bp, T, gens_for):
    """One call of B = 37 equals calls of 20 and 17 with index_base 0 and 20, concatenated."""
    import torch
    n, B = 8, 37
    v, gamma = inputs(B, n, np.random.default_rng(5), refuse=30)
    G, H, g, h = (T(x) for x in gens_for(n))
    whole = bp.batch_generate_range_proof_seeded(n, T(v), T(gamma), SEED, G, H, g, h)
    lo = bp.batch_generate_range_proof_seeded(n, T(v[:20]), T(gamma[:20]), SEED, G, H, g, h, index_base=0)
    hi = bp.batch_generate_range_proof_seeded(n, T(v[20:]), T(gamma[20:]), SEED, G, H, g, h, index_base=20)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(whole[k], torch.cat([lo[k], hi[k]])), k


def test_binding(bp, T, gens_for):
    """The seed, a proof's value, its gamma and its index each change that proof's A and S; the other
    proofs of the batch keep every byte (unless index_base moved them too)."""
    import torch
    n, B = 8, 6
    v, gamma = inputs(B, n, np.random.default_rng(9))
    G, H, g, h = (T(x) for x in gens_for(n))
    run = lambda v_, g_, seed, ib: bp.batch_generate_range_proof_seeded(n, T(v_), T(g_), seed, G, H, g, h, index_base=ib)
    base = run(v, gamma, SEED, 0)
    changed = lambda o, p: not torch.equal(o["A"][p], base["A"][p]) and not torch.equal(o["S"][p], base["S"][p])

    o = run(v, gamma, SEED[:31] + b"\x20", 0)            # one seed bit
    assert all(changed(o, p) for p in range(B))
    o = run(v, gamma, SEED, 1)                           # every proof's index moves
    assert all(changed(o, p) for p in range(B))
    v2 = v.copy()
    v2[2, 0] ^= np.uint64(1)                             # one value
    o = run(v2, gamma, SEED, 0)
    assert changed(o, 2)
    same(o, base, rows=[0, 1, 3, 4, 5])
    g2 = gamma.copy()
    g2[3, 3] ^= np.uint64(1 << 40)                       # one gamma
    o = run(v, g2, SEED, 0)
    assert changed(o, 3)
    same(o, base, rows=[0, 1, 2, 4, 5])
    torch.cuda.synchronize()
    assert int(base["valid"].sum()) == B


@pytest.mark.parametrize("chunk", [None, 4])
def test_host_entry_point(bp, T, gens_for, chunk, monkeypatch):
    """batch_generate_range_proof_host at n = 16, count = 9 (one value refused) returns the device
    call's bytes, in one chunk and in three chunks over the two streams (HIPBP_PROVE_HOST_CHUNK = 4);
    batch_range_proof_verify_host on its structs gives the verdicts batch_range_proof_verify gives
    the device tensors (equal arrays: the reference's arithmetic rejects some honest proofs).  Every
    vector of every proof is freed through libc free inside the wrapper."""
    import torch
    n, B, ib = 16, 9, 2**32 - 3
    if chunk is not None:
        monkeypatch.setenv("HIPBP_PROVE_HOST_CHUNK", str(chunk))
    v, gamma = inputs(B, n, np.random.default_rng(16), refuse=5)
    Gn, Hn, gn, hn = gens_for(n)
    G, H, g, h = T(Gn), T(Hn), T(gn), T(hn)
    dev = bp.batch_generate_range_proof_seeded(n, T(v), T(gamma), SEED, G, H, g, h, index_base=ib)
    ok_dev = torch.zeros(B, dtype=torch.uint8, device=G.device)
    bp.batch_range_proof_verify(bp.RangeProofBatch(n, **{k: dev[k] for k in bp.RangeProofBatch.FIELDS}), G, H, g, h, ok_dev)
    torch.cuda.synchronize()
    d = {k: dev[k].cpu().numpy().view(np.uint64) if k != "valid" else dev[k].cpu().numpy() for k in KEYS}

    proofs, valid = bp.batch_generate_range_proof_host(v, gamma, n, Gn, Hn, gn, hn, SEED, index_base=ib)
    assert len(proofs) == B
    assert np.array_equal(valid, d["valid"].astype(bool)) and not valid[5] and valid.sum() == B - 1
    for p, pr in enumerate(proofs):
        head = np.concatenate([d[k][p] for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")])
        assert np.array_equal(pr["head"], head), p
        if valid[p]:
            assert pr["n"] == n and pr["L_len"] == 4
            for k in ("a", "b", "L", "R"):
                assert np.array_equal(pr[k], d[k][p]), (p, k)
        else:   # the zeroed proof: ip_proof all zero, nothing to free
            assert pr["n"] == 0 and pr["L_len"] == 0 and all(len(pr[k]) == 0 for k in ("a", "b", "L", "R"))
    ok_host = bp.batch_range_proof_verify_host(proofs, d["V"], n, Gn, Hn, gn, hn, num_gpus=1)
    assert np.array_equal(ok_host, ok_dev.cpu().numpy().astype(bool))


def test_argument_errors_write_nothing(bp, T, gens_for):
    """Non-NULL sL in the seeded call, n = 3 and n = 256 give HIPBP_ERR_ARG and write nothing; a 31-byte
    seed raises ValueError at every Python entry point."""
    import torch
    B = 4
    v, gamma = inputs(B, 8, np.random.default_rng(1))
    vd, gd = T(v), T(gamma)
    G, H, g, h = (T(x) for x in gens_for(8))
    L = bp.lib()
    c = lambda t: ctypes.c_void_p(t.data_ptr())
    sd = (ctypes.c_uint8 * 32).from_buffer_copy(SEED)
    FILL = 0x5A5A5A5A5A5A5A5A
    fresh = lambda *shape: torch.full(shape, FILL, dtype=torch.int64, device=vd.device)

    def seeded(n, sL=None):
        out = {k: fresh(B, 16) for k in ("V", "A", "S", "T1", "T2")}
        out.update({k: fresh(B, 4) for k in ("taux", "mu", "t", "c", "x", "a", "b")})
        out.update(L=fresh(B, 8, 16), R=fresh(B, 8, 16), valid=torch.full((B,), 0x5A, dtype=torch.uint8, device=vd.device))
        ic = bp.ProveInputC(B, n, vd.data_ptr(), gd.data_ptr(), sL.data_ptr() if sL is not None else None, None, None)
        oc = bp.ProofOutC(*[out[k].data_ptr() for k in KEYS])
        rc = L.hipbp_batch_generate_range_proof_seeded(ctypes.byref(ic), sd, ctypes.c_uint64(0), c(G), c(H), c(g), c(h),
                                                       ctypes.byref(oc), None)
        torch.cuda.synchronize()
        assert rc == 1, (n, rc)   # HIPBP_ERR_ARG
        assert all(bool((t == (0x5A if k == "valid" else FILL)).all()) for k, t in out.items()), n

    seeded(8, sL=fresh(B, 8, 4))
    seeded(3)
    seeded(256)
    for n in (3, 256):
        sL, sR, rnd = fresh(B, 256, 4), fresh(B, 256, 4), fresh(B, 4, 4)
        rc = L.hipbp_derive_prover_scalars(sd, c(vd), c(gd), ctypes.c_uint64(0), ctypes.c_size_t(B), ctypes.c_size_t(n),
                                           c(sL), c(sR), c(rnd), None)
        torch.cuda.synchronize()
        assert rc == 1 and all(bool((t == FILL).all()) for t in (sL, sR, rnd)), n
        with pytest.raises(bp.BulletproofError):
            bp.derive_prover_scalars(n, vd, gd, SEED)
    with pytest.raises(ValueError):
        bp.derive_prover_scalars(8, vd, gd, SEED[:31])
    with pytest.raises(ValueError):
        bp.batch_generate_range_proof_seeded(8, vd, gd, SEED[:31], G, H, g, h)
    Gn, Hn, gn, hn = gens_for(8)
    with pytest.raises(ValueError):
        bp.batch_generate_range_proof_host(v, gamma, 8, Gn, Hn, gn, hn, SEED[:31])
    with pytest.raises(bp.BulletproofError):
        bp.batch_generate_range_proof_host(v, gamma, 3, Gn, Hn, gn, hn, SEED)


def test_release_frees_every_workspace_of_a_stream(bp, T, gens_for, oracle):
    """hipbp_release_stream_workspaces over a stream that used every per-stream workspace: on one
    fresh stream, two rounds of the explicit prover, the seeded prover, batch_inner_product_prove
    (B = 3: two chunks, so the side stream and its events exist), batch_range_proof_verify (a cached
    pipeline), msm (n = 300), then the release.  Round 2, on rebuilt workspaces, gives round 1's bits;
    the three proofs verify.  Inputs: inputs(3, 8, default_rng(0)), the first seed for which the CPU
    restatement of the reference's prover and verifier accepts all three proofs (checked here too)."""
    import torch
    n, B = 8, 3
    rng = np.random.default_rng(0)
    v, gamma = inputs(B, n, rng)
    Gn, Hn, gn, hn = gens_for(n)
    G, H, g, h = T(Gn), T(Hn), T(gn), T(hn)
    vd, gd = T(v), T(gamma)
    sc = {k: T(x) for k, x in ref.derive(SEED, v, gamma, 0, n).items()}
    ia, ib = (T(rng.integers(0, 2**63, (B, n, 4), dtype=np.uint64)) for _ in range(2))
    ic = T(rng.integers(0, 2**63, (B, 4), dtype=np.uint64))
    ms, mP = T(rng.integers(0, 2**63, (300, 4), dtype=np.uint64)), T(oracle.base_points(300, 21))
    st = torch.cuda.Stream(G.device)
    rounds = []
    for _ in range(2):
        ok = torch.zeros(B, dtype=torch.uint8, device=G.device)
        m = torch.zeros(16, dtype=torch.int64, device=G.device)
        torch.cuda.synchronize()
        o0 = bp.batch_generate_range_proof(n, vd, gd, sc["sL"], sc["sR"], sc["rnd"], G, H, g, h, stream=st)
        o1 = bp.batch_generate_range_proof_seeded(n, vd, gd, SEED, G, H, g, h, stream=st)
        ip = bp.batch_inner_product_prove(n, ia, ib, ic, G, H, h, stream=st)
        bp.batch_range_proof_verify(bp.RangeProofBatch(n, **{k: o0[k] for k in bp.RangeProofBatch.FIELDS}), G, H, g, h, ok,
                                    stream=st)
        bp.msm(m, ms, mP, stream=st)
        bp.release_stream_workspaces(st)   # waits for st first
        rounds.append([o0[k] for k in KEYS] + [o1[k] for k in KEYS] +
                      [ip[k] for k in ("a", "b", "c", "x", "c_final", "L", "R")] + [ok, m])
    for k, (a, b) in enumerate(zip(*rounds)):
        assert torch.equal(a, b), k
    same(o0, o1)
    assert rounds[1][-2].cpu().numpy().tolist() == [1, 1, 1]
    d = {k: o0[k].cpu().numpy().view(np.uint64) for k in KEYS if k != "valid"}
    for p in range(B):
        head = np.concatenate([d[k][p] for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")])
        assert oracle.cuda_range_proof_verify(head, d["V"][p], n, d["a"][p], d["b"][p], d["L"][p], d["R"][p],
                                              Gn, Hn, gn, hn)[0], p
    bp.release_stream_workspaces(torch.cuda.Stream(G.device))   # a stream that never ran anything

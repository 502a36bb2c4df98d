"""Batched Pedersen commitments on the GPU (hipbp_batch_pedersen_commit, _gens, _open, _host), exact
equality throughout.  The expected points are the reference-emitted rows of tests/golden/commit.npz,
the reference prover's own V (proofs_n16 / proofs_n64), and the C restatement's composition
(tests/commit_ref.py), which tests/test_commit_cpu.py pins to both."""
import ctypes

import numpy as np
import pytest

import commit_ref as cr

pytestmark = pytest.mark.gpu

IDENTITY = np.array([0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], np.uint64)   # (0, 1, 1, 0)
COUNTS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def T():
    import torch
    dev = torch.device("cuda:0")
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


def N(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()


@pytest.fixture(scope="module")
def pairs(golden, oracle):
    """The two (G, H, g, h) of n = 16: the fixtures' set (Z = 1) and the projective one."""
    d, pj, c = golden("proofs_n16"), golden("projective"), golden("commit")
    g, h = oracle.gh()
    assert np.array_equal(g, d["g"]) and np.array_equal(h, d["h"])
    assert np.array_equal(c["g"][0], g) and np.array_equal(c["h"][0], h)
    assert np.array_equal(c["g"][1], pj["g"]) and np.array_equal(c["h"][1], pj["h"])
    return [(d["G"], d["H"], g, h), (pj["G"], pj["H"], pj["g"], pj["h"])]


@pytest.fixture(scope="module")
def gens(bp, T, pairs):
    """Generator sets per (pair, K), made on first use, closed at the end of the module."""
    cache = {}

    def get(k, K):
        if (k, K) not in cache:
            G, H, g, h = pairs[k]
            cache[(k, K)] = bp.Generators(16, T(G), T(H), T(g), T(h), prefix_bits=K)
        return cache[(k, K)]
    yield get
    for gs in cache.values():
        gs.close()


@pytest.fixture(scope="module")
def random130(oracle, pairs):
    """130 seeded random 64-bit values and masked blindings with their restatement on pair 0."""
    rng = np.random.default_rng(20)
    v, gamma = cr.values64(rng, 130), cr.masked(rng, 130)
    _, _, g, h = pairs[0]
    return v, gamma, cr.restate_many(oracle, v, gamma, g, h)


@pytest.fixture(scope="module")
def commit(bp, T):
    def run(v, gamma, g, h, gens=None, stream=None):
        return N(bp.batch_pedersen_commit(T(v), T(gamma), T(g), T(h), gens=gens, stream=stream))
    return run


def reference_rows(golden, pairs):
    """[(v, gamma, g, h, expected, pair index)]: commit.npz's two crosses and the 12 fixture V."""
    c = golden("commit")
    rows = [(c["v"][88 * k:88 * k + 88], c["gamma"][88 * k:88 * k + 88], pairs[k][2], pairs[k][3],
             c["out"][88 * k:88 * k + 88], k) for k in (0, 1)]
    for n in (16, 64):
        v, gamma, g, h, V = cr.fixture_v_rows(n)
        assert np.array_equal(g, pairs[0][2]) and np.array_equal(h, pairs[0][3])
        rows.append((v, gamma, g, h, V, 0))
    return rows


# ---------------------------------------------------------------- 1. reference rows, every path
@pytest.mark.parametrize("path", ["plain", "gens1", "gens8", "gens12", "host"])
def test_reference_rows(bp, golden, pairs, gens, commit, path):
    for v, gamma, g, h, want, k in reference_rows(golden, pairs):
        if path == "plain":
            got = commit(v, gamma, g, h)
        elif path == "host":
            got = bp.batch_pedersen_commit_host(v, gamma, g, h)
        else:
            got = commit(v, gamma, g, h, gens=gens(k, int(path[4:])))
        assert got.shape == want.shape and got.dtype == np.uint64
        bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
        assert not bad, (path, k, bad[:8])


# ---------------------------------------------------------------- 2. wave and class boundaries
@pytest.mark.parametrize("count", COUNTS)
def test_wave_and_class_boundaries(pairs, random130, commit, count):
    v, gamma, want = random130
    _, _, g, h = pairs[0]
    assert np.array_equal(commit(v[:count], gamma[:count], g, h), want[:count])


# ---------------------------------------------------------------- 3. table boundary
def _with_leading_zeros(rng, lz):
    """A random 256-bit scalar with exactly lz leading zero bits, (4,) uint64."""
    x = int.from_bytes(rng.bytes(32), "little") >> lz
    x |= 1 << (255 - lz)
    assert x.bit_length() == 256 - lz
    return np.array([(x >> (64 * i)) & (2**64 - 1) for i in range(4)], np.uint64)


@pytest.mark.parametrize("k", [0, 1])
def test_table_boundary(oracle, pairs, gens, commit, k):
    """K = 8: blindings with K - 1, K and K + 1 leading zeros (table start, and the two dtab starts
    beside it) crossed with values of 191, 192 and 255 leading zeros."""
    rng = np.random.default_rng(3)
    gam = [_with_leading_zeros(rng, lz) for lz in (7, 8, 9)]
    val = [_with_leading_zeros(rng, lz) for lz in (191, 192, 255)]
    v = np.stack([a for a in val for _ in gam])
    gamma = np.stack([b for _ in val for b in gam])
    _, _, g, h = pairs[k]
    plain = commit(v, gamma, g, h)
    assert np.array_equal(commit(v, gamma, g, h, gens=gens(k, 8)), plain)
    assert np.array_equal(plain, cr.restate_many(oracle, v, gamma, g, h))


# ---------------------------------------------------------------- 4. uniform-scalar waves
def test_uniform_scalar_waves(oracle, pairs, random130, commit):
    v, gamma, want = random130
    _, _, g, h = pairs[0]
    # 64 identical pairs: both classes' waves take the uniform-scalar loop
    got = commit(np.repeat(v[5:6], 64, axis=0), np.repeat(gamma[5:6], 64, axis=0), g, h)
    assert np.array_equal(got, np.repeat(want[5:6], 64, axis=0))
    # v = 0 in every lane (uniform: the 256 doublings of the identity), distinct gamma (the lane loop)
    z = np.zeros((64, 4), np.uint64)
    assert np.array_equal(commit(z, gamma[:64], g, h), cr.restate_many(oracle, z, gamma[:64], g, h))


# ---------------------------------------------------------------- 5. the edge cross in one wave
@pytest.mark.parametrize("count", [64, 65])
@pytest.mark.parametrize("k", [0, 1])
def test_edge_cross_in_one_wave(golden, pairs, commit, k, count):
    """The 8 x 8 edge cross fills one wave per class (the rare canonicalisation inputs p - 1 .. 2^256 - 1
    beside ordinary lanes); at 65 a masked random row starts a second wave."""
    c = golden("commit")
    rows = [88 * k + iv * 11 + ig for iv in range(8) for ig in range(8)] + [88 * k + 2 * 11 + 9]
    rows = rows[:count]
    _, _, g, h = pairs[k]
    assert np.array_equal(commit(c["v"][rows], c["gamma"][rows], g, h), c["out"][rows])


# ---------------------------------------------------------------- 6. agreement with the prover
def test_agrees_with_the_prover(bp, oracle, T, commit):
    from oracle.pyoracle import prover_randomness
    n, B = 8, 5
    rng = np.random.default_rng(8)
    v = np.zeros((B, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << n, B, dtype=np.uint64)
    v[3, 0] |= np.uint64(1 << n)                       # bit n set: the prover refuses it (rp.cu:238)
    gam = np.zeros((B, 4), np.uint64)
    sL, sR, rnd = np.zeros((B, n, 4), np.uint64), np.zeros((B, n, 4), np.uint64), np.zeros((B, 4, 4), np.uint64)
    for p in range(B):
        gamma, sLR, rnd4 = prover_randomness(500 + p, n)
        gam[p] = gamma.view("<u8")
        sL[p] = sLR[:, :32].copy().view("<u8").reshape(n, 4)
        sR[p] = sLR[:, 32:].copy().view("<u8").reshape(n, 4)
        rnd[p] = rnd4.view("<u8").reshape(4, 4)
    G, H = oracle.base_points(n, 1), oracle.base_points(n, 2)
    g, h = oracle.gh()
    o = bp.batch_generate_range_proof(n, T(v), T(gam), T(sL), T(sR), T(rnd), T(G), T(H), T(g), T(h))
    V, valid = N(o["V"]), N(o["valid"])
    assert valid.tolist() == [1, 1, 1, 0, 1]
    got = commit(v, gam, g, h)
    for p in range(B):
        if valid[p]:
            assert np.array_equal(got[p], V[p]), p
        else:
            assert np.array_equal(V[p], IDENTITY), p
    assert np.array_equal(got[3], cr.restate(oracle, v[3], gam[3], g, h))


# ---------------------------------------------------------------- 7. open
@pytest.mark.parametrize("k", [0, 1])
def test_open(bp, T, pairs, gens, random130, commit, k):
    v, gamma, _ = random130
    v, gamma = v[:8], gamma[:8]
    _, _, g, h = pairs[k]
    V = commit(v, gamma, g, h)
    want = np.ones(8, np.uint8)
    for row, limb in ((1, 0), (2, 4 + 3), (3, 8 + 1), (4, 12 + 2)):   # one limb of X, Y, Z, T
        V[row, limb] ^= np.uint64(1) << np.uint64(17)
        want[row] = 0
    plain = N(bp.batch_pedersen_open(T(V), T(v), T(gamma), T(g), T(h)))
    assert plain.dtype == np.uint8 and np.array_equal(plain, want)
    for K in (0, 8):
        assert np.array_equal(N(bp.batch_pedersen_open(T(V), T(v), T(gamma), None, None, gens=gens(k, K))), want)
    good = commit(v, gamma, g, h)
    assert N(bp.batch_pedersen_open(T(good), T(v), T(gamma), T(g), T(h))).tolist() == [1] * 8


# ---------------------------------------------------------------- 8. host form, error paths
def test_host_form_in_shards(bp, pairs, random130, commit, monkeypatch):
    v, gamma, want = random130
    _, _, g, h = pairs[0]
    dev = commit(v, gamma, g, h)
    assert np.array_equal(dev, want)
    monkeypatch.setenv("HIPBP_HOST_SHARDS", "3")
    assert np.array_equal(bp.batch_pedersen_commit_host(v, gamma, g, h, num_gpus=0), dev)
    monkeypatch.delenv("HIPBP_HOST_SHARDS")
    assert np.array_equal(bp.batch_pedersen_commit_host(v, gamma, g, h, num_gpus=1), dev)


def test_error_paths(bp, T, pairs, gens, random130):
    import torch
    L = bp.lib()
    v, gamma, _ = random130
    v, gamma = np.ascontiguousarray(v[:4]), np.ascontiguousarray(gamma[:4])
    g, h = (np.ascontiguousarray(x, np.uint64) for x in pairs[0][2:])
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    sz, ci = ctypes.c_size_t, ctypes.c_int
    # too many GPUs: the verifier's message, a sentinel-filled out untouched
    ndev = bp.require_gpu()
    out = np.full((4, 16), 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = L.hipbp_batch_pedersen_commit_host(p(out), p(v), p(gamma), sz(4), p(g), p(h), ci(ndev + 1))
    assert rc == 1 and L.hipbp_last_error().decode() == f"num_gpus = {ndev + 1} but {ndev} HIP device(s) visible"
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    with pytest.raises(bp.BulletproofError, match=r"num_gpus = \d+ but \d+ HIP device\(s\) visible"):
        bp.batch_pedersen_commit_host(v, gamma, g, h, num_gpus=ndev + 1)
    # count = 0: OK, nothing written
    assert L.hipbp_batch_pedersen_commit_host(p(out), p(v), p(gamma), sz(0), p(g), p(h), ci(1)) == 0
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    assert bp.batch_pedersen_commit_host(v[:0], gamma[:0], g, h).shape == (0, 16)
    dv, dg, dgen, dh = T(v), T(gamma), T(g), T(h)
    dout = torch.full((4, 16), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dv.device)
    dok = torch.full((4,), 7, dtype=torch.uint8, device=dv.device)
    s = bp._stream_ptr(None)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    gs = ctypes.c_void_p(gens(0, 8).h)
    assert L.hipbp_batch_pedersen_commit(q(dout), q(dv), q(dg), sz(0), q(dgen), q(dh), s) == 0
    assert L.hipbp_batch_pedersen_commit_gens(q(dout), q(dv), q(dg), sz(0), gs, s) == 0
    assert L.hipbp_batch_pedersen_open(q(dok), q(dout), q(dv), q(dg), sz(0), q(dgen), q(dh), None, s) == 0
    assert bp.batch_pedersen_commit(dv[:0], dg[:0], dgen, dh).shape == (0, 16)
    # a null pointer: HIPBP_ERR_ARG, nothing written
    for k in range(5):
        a = [q(dout), q(dv), q(dg), q(dgen), q(dh)]
        a[k] = None
        assert L.hipbp_batch_pedersen_commit(a[0], a[1], a[2], sz(4), a[3], a[4], s) == 1, k
        ah = [p(out), p(v), p(gamma), p(g), p(h)]
        ah[k] = None
        assert L.hipbp_batch_pedersen_commit_host(ah[0], ah[1], ah[2], sz(4), ah[3], ah[4], ci(1)) == 1, k
    for k in range(4):
        a = [q(dout), q(dv), q(dg), gs]
        a[k] = None
        assert L.hipbp_batch_pedersen_commit_gens(a[0], a[1], a[2], sz(4), a[3], s) == 1, k
    for k in range(6):
        a = [q(dok), q(dout), q(dv), q(dg), q(dgen), q(dh)]
        a[k] = None
        assert L.hipbp_batch_pedersen_open(a[0], a[1], a[2], a[3], sz(4), a[4], a[5], None, s) == 1, k
    assert L.hipbp_batch_pedersen_open(q(dok), q(dout), None, q(dg), sz(4), None, None, gs, s) == 1
    torch.cuda.synchronize()
    assert (dout == 0x5A5A5A5A5A5A5A5A).all() and (dok == 7).all() and (out == 0xA5A5A5A5A5A5A5A5).all()


# ---------------------------------------------------------------- 9. workspaces and chunks
def test_side_stream_release_and_chunks(bp, pairs, random130, commit, monkeypatch):
    import torch
    v, gamma, want = random130
    _, _, g, h = pairs[0]
    side = torch.cuda.Stream()
    first = commit(v, gamma, g, h, stream=side)
    side.synchronize()
    bp.release_stream_workspaces(side)
    again = commit(v, gamma, g, h, stream=side)
    side.synchronize()
    bp.release_stream_workspaces(side)
    assert np.array_equal(first, want) and np.array_equal(again, want)
    monkeypatch.setenv("HIPBP_COMMIT_CHUNK", "64")      # three chunks: 64, 64, 2
    assert np.array_equal(commit(v, gamma, g, h), want)
    assert np.array_equal(bp.batch_pedersen_commit_host(v, gamma, g, h), want)
    monkeypatch.delenv("HIPBP_COMMIT_CHUNK")
    assert np.array_equal(commit(v, gamma, g, h), want)


# ---------------------------------------------------------------- 10. the chain-length sort
@pytest.mark.parametrize("count", COUNTS)
def test_sort_switch_same_bytes(bp, T, pairs, gens, random130, commit, monkeypatch, count):
    v, gamma, want = random130
    _, _, g, h = pairs[0]
    for sw in ("1", "0", "1"):
        monkeypatch.setenv("HIPBP_COMMIT_SORT", sw)
        assert np.array_equal(commit(v[:count], gamma[:count], g, h), want[:count]), sw
        assert np.array_equal(commit(v[:count], gamma[:count], g, h, gens=gens(0, 8)), want[:count]), sw
        V = T(want[:count])
        assert N(bp.batch_pedersen_open(V, T(v[:count]), T(gamma[:count]), T(g), T(h))).all(), sw


def test_sort_threshold_same_bytes(oracle, pairs, commit, monkeypatch):
    """4160 commitments: with the switch unset a chunk of 4096 or more is sorted (the whole call, and
    the first of its two chunks at HIPBP_COMMIT_CHUNK=4096, whose last 64 are not); the switch at 0
    and 1 gives the same bytes, and 16 rows spread over the call equal the restatement."""
    rng = np.random.default_rng(21)
    count = 4160
    v, gamma = cr.values64(rng, count), cr.masked(rng, count)
    v[::7, 0] >>= np.uint64(40)                         # mixed chain lengths in the value class
    _, _, g, h = pairs[0]
    monkeypatch.delenv("HIPBP_COMMIT_SORT", raising=False)
    got = commit(v, gamma, g, h)
    rows = list(range(0, count, count // 15))[:15] + [count - 1]
    assert np.array_equal(got[rows], cr.restate_many(oracle, v[rows], gamma[rows], g, h))
    monkeypatch.setenv("HIPBP_COMMIT_CHUNK", "4096")
    assert np.array_equal(commit(v, gamma, g, h), got)
    monkeypatch.delenv("HIPBP_COMMIT_CHUNK")
    for sw in ("0", "1"):
        monkeypatch.setenv("HIPBP_COMMIT_SORT", sw)
        assert np.array_equal(commit(v, gamma, g, h), got), sw

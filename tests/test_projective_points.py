"""Projective and otherwise arbitrary input points through every scalar-multiplication path.

The engine takes a point as the reference does: sixteen limbs, whatever they hold.  Z need not be
1, T need not be X*Y, no coordinate need be below p.  Three wave-uniform shortcuts depend on a
point's Z limbs being exactly 1,0,0,0 (sm_lane and sm_uniform in ge25519_dev.h, the first bucket
tree level in bp_pippenger.hip); the generators' prefix tables are built with the general product.
These tests feed those paths waves whose lanes disagree about Z: affine beside projective, and
"disguised ones" (p + 1, 2p + 1, 1 + 2^255: 1 mod p or nearly, but other limbs) beside real ones.
Everything is bit-exact against the CPU restatement (oracle/) and against what the reference itself
emitted (tests/golden/projective.npz, point.npz).

The input builder below is also what tests/golden/make_golden.py (section `projective`) draws the
fixture's inputs from.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

# ----------------------------------------------------------------------------- input builder
M = 2**64 - 1
P_INT = 2**255 - 19
# the Z classes: a name and the 256-bit value (None: random limbs drawn per point)
Z_CLASSES = (("one", 1), ("p+1", P_INT + 1), ("2p+1", 2 * P_INT + 1), ("1+2^255", 1 + 2**255), ("zero", 0),
             ("two", 2), ("p", P_INT), ("p-1", P_INT - 1), ("2^256-1", 2**256 - 1), ("rand256", None),
             ("rand255", None))
ZC = {name: i for i, (name, _) in enumerate(Z_CLASSES)}
NCLS = len(Z_CLASSES)
# Z = 0 is special: scalar * (X, Y, 0, T) is the point (0, 0, 1, 0) once device-normalized, for
# every scalar without a long run of leading zeros (the first add gives D = C = 0, so F = G = 0),
# and that point absorbs every sum it enters (A = B = C = 0, so E = H = 0).
# A Z = 0 lane therefore carries a zero scalar wherever a test wants a result that still depends
# on its other terms (the lane still decides its wave's path); generator sets and proof points
# use the other projective classes (LIVE).  test_zero_z_collapses pins the collapse itself.
LIVE = tuple(i for i in range(1, NCLS) if i != ZC["zero"])


def live_cycle(k, start=0):
    return [LIVE[(start + i) % len(LIVE)] for i in range(k)]


def park_zero_z(s, zcls, classes=("zero",)):
    """Zero scalars on the Z = 0 points (the bucket MSM adds raw points, and there Z = p absorbs
    as well: it parks both)."""
    for c in classes:
        s[np.asarray(zcls) == ZC[c]] = 0
    return s


def live(point):
    """The result is not the absorbing point: the comparison says something about every term."""
    assert np.asarray(point)[..., :8].any(axis=-1).all(), "collapsed to (0, 0, 1, 0)"
    return point


def limbs(v):
    return np.array([(v >> (64 * i)) & M for i in range(4)], np.uint64)


def to_int(f):
    return sum(int(f[i]) << (64 * i) for i in range(4))


assert [int(x) for x in limbs(P_INT + 1)] == [0xFFFFFFFFFFFFFFEE, M, M, 0x7FFFFFFFFFFFFFFF]
assert [int(x) for x in limbs(2 * P_INT + 1)] == [M - 36, M, M, M]
assert [int(x) for x in limbs(1 + 2**255)] == [1, 0, 0, 1 << 63]


def rand256(rng, k, top=True):
    v = rng.integers(0, 2**64, size=(k, 4), dtype=np.uint64)
    if not top:
        v[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    return v


def edge_scalars(rng, n):
    from make_golden import edge_fe
    return edge_fe(rng, n)


def proj_points(rng, zcls):
    """len(zcls) points, point i with the Z of class zcls[i].  X, Y and T are full 256-bit random
    words (bit 255 set on half of them), a quarter of them replaced by make_golden.edge_fe's edge
    limbs.  The affine points and every second projective one get T = X*Y mod p; the other
    projective ones keep an arbitrary T."""
    from make_golden import edge_fe
    zcls = np.asarray(zcls, np.int64)
    n = len(zcls)
    pts = np.zeros((n, 16), np.uint64)
    for col in (0, 4, 12):
        v, e = rand256(rng, n), edge_fe(rng, n)
        use = rng.random(n) < 0.25
        v[use] = e[use]
        pts[:, col:col + 4] = v
    nproj = 0
    for i, z in enumerate(zcls):
        name, val = Z_CLASSES[z]
        pts[i, 8:12] = rand256(rng, 1, top=name == "rand256")[0] if val is None else limbs(val)
        if z != 0:
            nproj += 1
            if nproj % 2:
                continue
        pts[i, 12:16] = limbs(to_int(pts[i, 0:4]) * to_int(pts[i, 4:8]) % P_INT)
    return pts


def every_class(rng, n):
    """n class indices holding every Z class (n >= NCLS), in shuffled order."""
    return rng.permutation(np.arange(n) % NCLS)


def msm_classes(rng, n):
    """The Z classes of the fixture's MSM rows."""
    if n == 1:
        return [ZC["p+1"]]
    if n < NCLS:
        return ([ZC["one"], ZC["p+1"], ZC["rand256"], ZC["one"], ZC["1+2^255"]] * n)[:n]
    return every_class(rng, n)


def gen_set(rng, n):
    """A generator set: G all projective, H alternating affine and projective, g.Z = p + 1,
    h.Z random."""
    G = proj_points(rng, live_cycle(n))
    H = proj_points(rng, [0 if i % 2 == 0 else LIVE[(i // 2) % len(LIVE)] for i in range(n)])
    g = proj_points(rng, [ZC["p+1"], ZC["rand256"]])
    return G, H, g[0].copy(), g[1].copy()


def proof_shaped(rng, n, B):
    """B proof-shaped random inputs (a = [t], b = [1], c = t, so <a, b> = c) in RangeProofBatch
    layout plus taux, mu, Vp: half of the proof points (V, A, S, T1, T2, L, R) projective, of
    every Z class but 0 in turn, at shuffled places."""
    Lr = max(n.bit_length() - 1, 0)
    per = 5 + 2 * Lr
    k = B * per
    z = np.zeros(k, np.int64)
    z[:k // 2] = live_cycle(k // 2)
    pts = proj_points(rng, rng.permutation(z)).reshape(B, per, 16)
    arr = {name: pts[:, i].copy() for i, name in enumerate(("V", "A", "S", "T1", "T2"))}
    arr["L"] = pts[:, 5:5 + Lr].copy()
    arr["R"] = pts[:, 5 + Lr:].copy()
    arr["t"] = rand256(rng, B, top=False)
    arr["x"] = rand256(rng, B, top=False)
    arr["taux"] = rand256(rng, B, top=False)
    arr["mu"] = rand256(rng, B, top=False)
    arr["t"][0] = 0                                  # a zero scalar: 256 doublings of the identity
    if B > 2:
        arr["x"][1, 1:] = 0                          # a short challenge: a long leading-zero run
    arr["a"] = arr["t"][:, None].copy()
    arr["b"] = np.zeros((B, 1, 4), np.uint64)
    arr["b"][:, 0, 0] = 1
    arr["c"] = arr["t"].copy()
    arr["Vp"] = arr["V"].copy()
    return arr


def heads_of(arr):
    return np.concatenate([arr[k] for k in ("Vp", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")], axis=1)


def sprinkle(s):
    """Zero and short scalars as in test_msm_multiblock_vs_oracle."""
    s[::5] = 0
    s[1::7, 1:] = 0
    return s


# ----------------------------------------------------------------------------- GPU helpers
def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda:0")


def _u(t):
    return t.cpu().numpy().view(np.uint64)


def gpu_msm(bp, s, P):
    import torch
    out = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    bp.msm(out, _T(s), _T(P))
    torch.cuda.synchronize()
    return _u(out)


def gpu_msm_batch(bp, s, P, count):
    import torch
    out = torch.zeros(count, 16, dtype=torch.int64, device="cuda:0")
    bp.msm_batch(out, _T(s), _T(P))
    torch.cuda.synchronize()
    return _u(out)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("projective")


# ----------------------------------------------------------------------------- a. point.npz on the GPU
def test_point_golden_on_gpu(bp, oracle, golden):
    """The reference's ge25519_add and ge25519_scalarmult results on edge-limb projective points
    (point.npz), reproduced by the GPU.  hipbp_point_tree over [p, q] is device-normalize(add(p, q));
    an MSM of one term is device-normalize(scalarmult(s, p))."""
    import torch
    d = golden("point")
    out = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    for i in range(len(d["p"])):
        bp.point_tree(out, _T(np.stack([d["p"][i], d["q"][i]])))
        torch.cuda.synchronize()
        assert np.array_equal(_u(out), oracle.ge_normalize_dev(d["add"][i])), i
    for i in range(len(d["scalars"])):
        s = np.ascontiguousarray(d["scalars"][i]).view("<u8").astype(np.uint64)[None]
        P = d["p"][i][None]
        want = oracle.ge_normalize_dev(d["scalarmult"][i])
        assert np.array_equal(gpu_msm(bp, s, P), want), i
        for shared in (False, True):
            assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P, shared=shared), want), (i, shared)


# ----------------------------------------------------------------------------- b. lane MSM, unsorted
@pytest.mark.parametrize("n", [1, 5, 64, 130])
def test_msm_fixture_rows(bp, oracle, fx, n):
    """The reference's own msm_canon over builder points (every Z class at n >= 64, the Z = 0
    points with zero scalars)."""
    s, P, want = fx[f"msm_s{n}"], fx[f"msm_P{n}"], live(fx[f"msm_canon{n}"])
    assert np.array_equal(oracle.msm_canon(s, P), want)
    assert np.array_equal(gpu_msm(bp, s, P), want)
    for shared in (False, True):
        assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P, shared=shared), want), shared


def test_zero_z_collapses(bp, oracle, fx):
    """A point with Z = 0 and a full-length scalar: its term is (0, 0, 1, 0), which absorbs the
    whole sum.  The reference's row (the n = 5 row with one Z zeroed) and a wave with one such lane."""
    s, P, want = fx["msm_s5z"], fx["msm_P5z"], fx["msm_canon5z"]
    assert not want[:8].any() and int(want[8]) == 1
    assert np.array_equal(oracle.msm_canon(s, P), want)
    assert np.array_equal(gpu_msm(bp, s, P), want)
    assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P, shared=True), want)
    rng = np.random.default_rng(5)
    z = np.zeros(64, np.int64)
    z[40] = ZC["zero"]
    P, s = proj_points(rng, z), rand256(rng, 64)
    s[40, 3] |= np.uint64(1 << 63)
    assert np.array_equal(gpu_msm(bp, s, P), want)
    assert np.array_equal(oracle.msm_canon(s, P), want)


def _mixed_waves(pos, cls):
    rng = np.random.default_rng(1000 + 64 * ZC[cls] + pos)
    z = np.zeros(256, np.int64)
    z[64 + pos] = ZC[cls]
    z[128:192] = 1 + np.arange(64) % (NCLS - 1)
    z[192:256:2] = live_cycle(32)
    P = proj_points(rng, z)
    s = park_zero_z(sprinkle(edge_scalars(rng, 256)), z)
    s[64 + pos] = rand256(rng, 1)[0]                 # the odd lane does work
    return s, P


@pytest.mark.parametrize("pos,cls", [(0, "p+1"), (31, "p+1"), (63, "p+1"), (31, "1+2^255"), (31, "2p+1")])
def test_lane_msm_mixed_waves(bp, oracle, pos, cls):
    """n = 256 < MSM_SORT_MIN: lane = item.  Wave 0 all Z = 1; wave 1 Z = 1 except lane `pos`,
    a disguised one; wave 2 all projective, every class; wave 3 half and half."""
    s, P = _mixed_waves(pos, cls)
    want = live(oracle.msm_canon(s, P))
    assert np.array_equal(gpu_msm(bp, s, P), want)
    assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P), want)


def test_lane_msm_short_last_wave(bp, oracle):
    """n = 200: the last wave has 8 active lanes, one of them projective."""
    rng = np.random.default_rng(200)
    z = np.zeros(200, np.int64)
    z[195] = ZC["p+1"]
    P = proj_points(rng, z)
    s = sprinkle(rand256(rng, 200))
    s[195] = rand256(rng, 1)[0]
    want = live(oracle.msm_canon(s, P))
    assert np.array_equal(gpu_msm(bp, s, P), want)
    z[195], z[3] = 0, ZC["rand255"]      # and the other way round: only a full wave is mixed
    P = proj_points(rng, z)
    assert np.array_equal(gpu_msm(bp, s, P), live(oracle.msm_canon(s, P)))


@pytest.mark.parametrize("n", [1, 17, 64])
def test_msm_shared_small_mixed(bp, oracle, n):
    """The n <= 64 kernel of cuda_point_vector_multi_scalar_mul_shared on one mixed wave."""
    rng = np.random.default_rng(64 + n)
    z = np.zeros(n, np.int64)
    z[n // 2] = ZC["2p+1"]
    if n > 8:
        z[n - 1], z[3] = ZC["zero"], ZC["rand256"]
    P = proj_points(rng, z)
    s = edge_scalars(rng, n)
    if n > 8:
        sprinkle(s)
    park_zero_z(s, z)
    s[n // 2] = rand256(rng, 1)[0]
    want = live(oracle.msm_canon(s, P))
    assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P, shared=True), want)
    assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P), want)


# ----------------------------------------------------------------------------- c. lane MSM, sorted
def test_lane_msm_sorted_scattered_projective(bp, oracle):
    """n = 4096 + 64 >= MSM_SORT_MIN: lanes take items in chain-length order, so the quarter of
    the points that is projective (scattered indices) lands in waves of the sort's choosing."""
    n = 4096 + 64
    rng = np.random.default_rng(n)
    z = np.zeros(n, np.int64)
    idx = rng.permutation(n)[:n // 4]
    z[idx] = 1 + np.arange(len(idx)) % (NCLS - 1)
    P = proj_points(rng, z)
    s = rand256(rng, n)
    s[::9] = 0
    s[1::7, 1:] = 0
    s[2::13, 2:] = 0
    park_zero_z(s, z)
    assert np.array_equal(gpu_msm(bp, s, P), live(oracle.msm_canon(s, P)))


# ----------------------------------------------------------------------------- d. uniform-scalar waves
UNIFORM_SCALARS = (0, 1, 2**255, 2**256 - 1, 0x5A17C3E1F00DFACE0123456789ABCDEF0FEDCBA987654321DEADBEEF00C0FFEE)


def test_uniform_scalar_waves(bp, oracle):
    """n = 128, one scalar per whole wave (sm_uniform): wave 0 all affine, wave 1 with one
    projective lane; then the waves swapped."""
    rng = np.random.default_rng(128)
    z = np.zeros(128, np.int64)
    z[64 + 17] = ZC["p+1"]
    for swap in (False, True):
        P = proj_points(rng, np.roll(z, 64) if swap else z)
        for k, v in enumerate(UNIFORM_SCALARS):
            s = np.tile(limbs(v), (128, 1))
            s[64:] = limbs(UNIFORM_SCALARS[(k + 1) % len(UNIFORM_SCALARS)])
            assert np.array_equal(gpu_msm(bp, s, P), live(oracle.msm_canon(s, P))), (swap, k)


@pytest.mark.parametrize("mixed", [False, True])
def test_uniform_scalar_waves_straddle_batch(bp, oracle, mixed):
    """msm_batch, n = 48, count = 4: 192 items in three waves, one scalar per wave, so every wave
    straddles two MSMs; all points affine, or one of them projective."""
    n, count = 48, 4
    rng = np.random.default_rng(48 + mixed)
    z = np.zeros(n, np.int64)
    if mixed:
        z[41] = ZC["1+2^255"]
    P = proj_points(rng, z)
    for k in range(0, len(UNIFORM_SCALARS), 2):
        s = np.zeros((count * n, 4), np.uint64)
        for w in range(3):
            s[64 * w:64 * w + 64] = limbs(UNIFORM_SCALARS[(k + w) % len(UNIFORM_SCALARS)])
        got = gpu_msm_batch(bp, s, P, count)
        for m in range(count):
            assert np.array_equal(got[m], live(oracle.msm_canon(s[m * n:(m + 1) * n], P))), (k, m)


# ----------------------------------------------------------------------------- e. projective generator sets
def _fixture_gens(fx):
    return fx["G"], fx["H"], fx["g"], fx["h"]


def _set_for(fx, n):
    if n == 16:
        return _fixture_gens(fx)
    return gen_set(np.random.default_rng(7000 + n), n)


@pytest.mark.parametrize("n,K", [(16, 0), (16, 5), (64, 6)])
def test_msm_batch_gens_projective(bp, oracle, fx, n, K):
    """msm_batch_gens over a projective generator set's G || H == msm_batch on the same points ==
    the oracle.  256 items, four waves: one whole wave each of a scalar with exactly K leading zeros
    (the last the prefix table misses: sm_uniform's dtab start), with K - 1 (its `pre` start) and of
    0; the fourth wave per-lane scalars (sm_lane_loop's table start)."""
    import torch
    G, H, g, h = _set_for(fx, n)
    GH = np.concatenate([G, H])
    count = 256 // (2 * n)
    rng = np.random.default_rng(n + K)
    s = rand256(rng, 256)
    s[0:64] = limbs(1 << (255 - K))
    s[64:128] = limbs((1 << (256 - K)) | 5) if K else limbs(2**256 - 1)
    s[128:192] = 0
    s[192 + 3] = 0
    s[192 + 4] = limbs(1 << (255 - K))
    gens = bp.Generators(n, _T(G), _T(H), _T(g), _T(h), prefix_bits=K)
    try:
        r1 = torch.zeros(count, 16, dtype=torch.int64, device="cuda:0")
        bp.msm_batch_gens(r1, _T(s), gens)
        torch.cuda.synchronize()
        r1 = _u(r1)
    finally:
        gens.close()
    assert np.array_equal(r1, gpu_msm_batch(bp, s, GH, count))
    for m in range(count):
        assert np.array_equal(r1[m], live(oracle.msm_canon(s[m * 2 * n:(m + 1) * 2 * n], GH))), m


def _case_arrays(fx):
    from test_gpu_parity import _std_arrays
    return _std_arrays(fx["head"], fx["V"], fx["a"], fx["b"], fx["L"], fx["R"])


def _all_forms(bp, monkeypatch, n, B, mode, arrays, gset, Pg, K):
    """The pipeline's outputs under HIPBP_QUAD unset, 0, 1, 2, 3, each without and with K-bit
    prefix tables: all equal; returned once."""
    import torch
    from test_gpu_parity import _pipeline_outputs
    G, H, g, h = gset
    outs = []
    for q in (None, "0", "1", "2", "3"):
        if q is None:
            monkeypatch.delenv("HIPBP_QUAD", raising=False)
        else:
            monkeypatch.setenv("HIPBP_QUAD", q)
        for bits in (0, K):
            outs.append((q, bits, _pipeline_outputs(bp, n, B, mode, arrays, G, H, g, h, Pg, bits=bits)[0]))
    for q, bits, o in outs[1:]:
        for k, (a, b) in enumerate(zip(outs[0][2], o)):
            assert torch.equal(a, b), (q, bits, k)
    o = outs[0][2]
    return o[0].numpy().astype(bool), _u(o[1]), _u(o[2]), o[3].numpy(), _u(o[4])


@pytest.mark.parametrize("n,B,K", [(16, 70, 5), (4, 5, 2)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pipeline_projective_everything(bp, oracle, fx, monkeypatch, n, B, K, mode):
    """The verify pipeline over a projective generator set and proofs whose points are half
    projective: every verdict, P, check point, mode-2 flag and polynomial side equals the oracle's
    for every proof, in the lane, quad, pair and row forms, without and with prefix tables."""
    from test_gpu_parity import _check_std_vs_oracle
    gset = _set_for(fx, n)
    G, H, g, h = gset
    rng = np.random.default_rng(100 * n + B)
    arrays = proof_shaped(rng, n, B)
    Pin = proj_points(rng, np.arange(B) % NCLS)
    ok, P, chk, fl, poly = _all_forms(bp, monkeypatch, n, B, mode, arrays, gset, _T(Pin), K)
    live(chk)
    if mode:
        live(P)
    if mode == 2:
        _check_std_vs_oracle(oracle, n, arrays, heads_of(arrays), G, H, g, h, (ok, P, chk, fl, poly))
        return
    heads = heads_of(arrays)
    for p in range(B):
        if mode == 1:
            okr, Pr, chkr, _, _ = oracle.cuda_range_proof_verify(heads[p], arrays["V"][p], n, arrays["a"][p],
                                                                 arrays["b"][p], arrays["L"][p], arrays["R"][p],
                                                                 G, H, g, h)
            assert np.array_equal(P[p], Pr), p
        else:
            okr, chkr, _, _ = oracle.cuda_inner_product_verify(n, arrays["a"][p], arrays["b"][p], arrays["c"][p],
                                                               arrays["L"][p], arrays["R"][p], arrays["x"][p],
                                                               Pin[p], G, H, h)
        assert ok[p] == okr, p
        assert np.array_equal(chk[p], chkr), p     # <a, b> = c in every proof: a check point is formed


def test_fixture_cases_match_reference(bp, fx, monkeypatch):
    """The eight reference-judged cases of projective.npz (four reference proofs under the
    projective generator set, four proof-shaped random inputs): the reference's verdicts, P, check
    points and sub-check flags, from the pipeline in both range modes, the single-proof call and
    the host-struct batch call."""
    n, K = 16, 5
    gset = _fixture_gens(fx)
    arrays = _case_arrays(fx)
    B = len(fx["head"])
    late = ~fx["early"].astype(bool)
    live(fx["P"])
    live(fx["check"][late])
    for mode in (1, 2):
        ok, P, chk, fl, _ = _all_forms(bp, monkeypatch, n, B, mode, arrays, gset, None, K)
        assert np.array_equal(P, fx["P"]), mode
        assert np.array_equal(chk[late], fx["check"][late]), mode
        if mode == 1:
            assert np.array_equal(ok, fx["ok_cuda"].astype(bool))
        else:
            assert np.array_equal(ok, fx["ok_cpu"].astype(bool))
            rf = fx["flags"].astype(np.int64)
            f = fl.astype(np.int64)
            assert np.array_equal(rf & 1 != 0, f & 2 != 0)        # enhanced_range_check
            assert np.array_equal(rf & 2 != 0, f & 28 != 0)       # robust_polynomial_identity_check
            assert np.array_equal(rf & 4 != 0, f & 32 != 0)       # inner_product_verify
    proofs = [dict(head=fx["head"][i], a=fx["a"][i], b=fx["b"][i], L=fx["L"][i], R=fx["R"][i]) for i in range(B)]
    for i in range(B):
        assert bp.cuda_range_proof_verify(proofs[i], fx["V"][i], n, *gset) == bool(fx["ok_cuda"][i]), i
    got = bp.batch_range_proof_verify_host(proofs, fx["V"], n, *gset)
    assert np.array_equal(got, fx["ok_cuda"].astype(bool))


def _prove(bp, n, inputs, gset, gens=None):
    import torch
    v, gam, sL, sR, rnd = inputs
    G, H, g, h = gset
    args = [_T(x) for x in (v, gam, sL, sR, rnd)]
    if gens is None:
        out = bp.batch_generate_range_proof(n, *args, _T(G), _T(H), _T(g), _T(h))
    else:
        out = bp.batch_generate_range_proof(n, *args, None, None, None, None, gens=gens)
    torch.cuda.synchronize()
    return {k: (_u(t) if k != "valid" else t.cpu().numpy()) for k, t in out.items() if k != "_keep"}


def _same_proof(o, p, pr):
    from oracle.pyoracle import head_fields
    hf = head_fields(pr["head"])
    assert o["valid"][p] == 1, p
    for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x"):
        assert np.array_equal(o[k][p], hf[k]), (p, k)
    for k in ("a", "b", "L", "R"):
        assert np.array_equal(o[k][p], pr[k]), (p, k)


@pytest.mark.parametrize("n", [8, 16])
def test_prover_projective_generators(bp, oracle, fx, n):
    """batch_generate_range_proof over a projective generator set, plain and with a Generators set
    (K = 4): every proof byte equals the oracle's prover's."""
    from test_gpu_parity import _prove_inputs
    B, K = 5, 4
    gset = _set_for(fx, n)
    rng = np.random.default_rng(n)
    values = [np.concatenate([rng.integers(0, 256, n // 8).astype(np.uint8), np.zeros(32 - n // 8, np.uint8)])
              for _ in range(B)]
    v, gam, sL, sR, rnd, rb = _prove_inputs([900 + 3 * p + n for p in range(B)], values, n)
    want = [oracle.generate_range_proof(values[p], *rb[p], n, *gset) for p in range(B)]
    live(np.stack([w["head"][:80].reshape(5, 16) for w in want]))
    live(np.stack([w["L"] for w in want]))
    gens = bp.Generators(n, *[_T(x) for x in gset], prefix_bits=K)
    try:
        for o in (_prove(bp, n, (v, gam, sL, sR, rnd), gset), _prove(bp, n, (v, gam, sL, sR, rnd), gset, gens)):
            for p in range(B):
                _same_proof(o, p, want[p])
    finally:
        gens.close()


def test_prover_reproduces_fixture_proofs(bp, fx):
    """The four reference proofs of projective.npz, byte for byte, plain and with tables."""
    from test_gpu_parity import _prove_inputs
    n, K = 16, 4
    gset = _fixture_gens(fx)
    seeds = [int(x) for x in fx["seed"]]
    v, gam, sL, sR, rnd, _ = _prove_inputs(seeds, fx["value"], n)
    gens = bp.Generators(n, *[_T(x) for x in gset], prefix_bits=K)
    try:
        for o in (_prove(bp, n, (v, gam, sL, sR, rnd), gset), _prove(bp, n, (v, gam, sL, sR, rnd), gset, gens)):
            for p in range(len(seeds)):
                _same_proof(o, p, dict(head=fx["head"][p], a=fx["a"][p], b=fx["b"][p], L=fx["L"][p], R=fx["R"][p]))
    finally:
        gens.close()


def ipa_case(fx, k):
    """Case k of the fixture's inner-product proofs: (n, inputs dict, outputs dict)."""
    ns = [int(x) for x in fx["ipa_n"]]
    n, o = ns[k], sum(ns[:k])
    lo = fx["ipa_L_off"]
    inp = dict(a=fx["ipa_a_in"][o:o + n], b=fx["ipa_b_in"][o:o + n], G=fx["ipa_G"][o:o + n], H=fx["ipa_H"][o:o + n],
               Q=fx["ipa_Q"][k], tr=fx["ipa_tr"][k])
    out = {key: fx["ipa_" + key][k] for key in ("a", "b", "x", "c_in", "c_final", "P", "check", "ok_in", "ok_final")}
    out["L"], out["R"] = fx["ipa_L"][lo[k]:lo[k + 1]], fx["ipa_R"][lo[k]:lo[k + 1]]
    return n, inp, out


@pytest.mark.parametrize("k", [0, 1])
def test_ipa_prover_projective_generators(bp, fx, k):
    """batch_inner_product_prove on the fixture's two reference proofs (n = 1, 8; projective G, H,
    Q), plain and with a Generators set: the reference's a, b, x, L, R, c_final."""
    import torch
    n, inp, want = ipa_case(fx, k)
    Lr = n.bit_length() - 1
    tr = np.ascontiguousarray(inp["tr"]).view("<u8").astype(np.uint64)[None]
    args = (_T(inp["a"][None]), _T(inp["b"][None]), _T(want["c_in"][None]))
    Gd, Hd, Qd = _T(inp["G"]), _T(inp["H"]), _T(inp["Q"])
    gens = bp.Generators(n, Gd, Hd, Qd, Qd, prefix_bits=3)
    try:
        for gs in (None, gens):
            o = bp.batch_inner_product_prove(n, *args, Gd, Hd, Qd, transcript=_T(tr), gens=gs)
            torch.cuda.synchronize()
            assert np.array_equal(_u(o["a"])[0, 0], want["a"]) and np.array_equal(_u(o["b"])[0, 0], want["b"])
            assert np.array_equal(_u(o["x"])[0], want["x"]) and np.array_equal(_u(o["c"])[0], want["c_in"])
            assert np.array_equal(_u(o["c_final"])[0], want["c_final"])
            assert np.array_equal(_u(o["L"])[0].reshape(Lr, 16), want["L"].reshape(Lr, 16))
            assert np.array_equal(_u(o["R"])[0].reshape(Lr, 16), want["R"].reshape(Lr, 16))
    finally:
        gens.close()


# ----------------------------------------------------------------------------- f. Pippenger
def _pip_layouts(n):
    # the lone projective point is no disguised one: 1 * (p + 1) folds to the bits of 1 * 1, so with
    # affine partners a p + 1 there could not tell the shortcut from the general product
    return {"all": [(i, 1 + i % (NCLS - 1)) for i in range(n)], "first": [(0, ZC["rand256"])],
            "middle": [(n // 2, ZC["2p+1"])], "last": [(n - 1, ZC["rand255"])],
            "halves": [(i, 1 + i % (NCLS - 1)) for i in range(n // 2, n)]}


def _pip_inputs(n, c, layout):
    rng = np.random.default_rng(31 * n + c + len(layout))
    z = np.zeros(n, np.int64)
    for i, cls in _pip_layouts(n)[layout]:
        z[i] = cls
    P = proj_points(rng, z)
    s = rand256(rng, 2 * n)
    s[::7] = 0
    s[1::5, 1:] = 0
    s[3::11] = s[3]                              # a crowded bucket in every window
    park_zero_z(s[:n], z, ("zero", "p"))
    park_zero_z(s[n:], z, ("zero", "p"))
    return s, P


@pytest.mark.parametrize("layout", ["all", "first", "middle", "last", "halves"])
@pytest.mark.parametrize("n,c", [(300, 8), (1000, 12), (4096, 12)])
def test_msm_pippenger_projective(bp, oracle, n, c, layout):
    """The bucket MSM's first tree level (its Z = 1 shortcut is a wave-uniform test) on all
    projective points, one projective point among affine ones (first, middle, last index) and
    halves: msm_pippenger, msm_pippenger_batch (count 2) and windows + Horner equal the oracle."""
    import torch
    W = bp.pippenger_num_windows(c)
    s, P = _pip_inputs(n, c, layout)
    want = [live(oracle.msm_pippenger(s[:n], P, c)), live(oracle.msm_pippenger(s[n:], P, c))]
    sd, Pd = _T(s), _T(P)
    one = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    two = torch.zeros(2, 16, dtype=torch.int64, device="cuda:0")
    Sw = torch.zeros(W, 16, dtype=torch.int64, device="cuda:0")
    hor = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    bp.msm_pippenger(one, sd[:n], Pd, c)
    bp.msm_pippenger_batch(two, sd, Pd, c)
    bp.msm_pippenger_windows(Sw, sd[:n], Pd, 0, W, c)
    bp.msm_pippenger_horner(hor, Sw, c)
    torch.cuda.synchronize()
    assert np.array_equal(_u(one), want[0])
    assert np.array_equal(_u(two), np.stack(want))
    assert np.array_equal(_u(hor), want[0])


@pytest.mark.parametrize("var,val", [("HIPBP_PIP_KEYS16", "0"), ("HIPBP_PIP_KEYS16", "1"),
                                     ("HIPBP_PIP_TAIL_LAYER", "1"), ("HIPBP_PIP_TAIL_LAYER", "2"),
                                     ("HIPBP_PIP_TAIL_LAYER", "6")])
def test_msm_pippenger_projective_knobs(bp, oracle, monkeypatch, var, val):
    """The (300, 8) halves case under the key-path and tail-layer settings the Pippenger parity
    tests toggle."""
    import torch
    n, c = 300, 8
    s, P = _pip_inputs(n, c, "halves")
    monkeypatch.setenv(var, val)
    two = torch.zeros(2, 16, dtype=torch.int64, device="cuda:0")
    bp.msm_pippenger_batch(two, _T(s), _T(P), c)
    torch.cuda.synchronize()
    want = live(np.stack([oracle.msm_pippenger(s[:n], P, c), oracle.msm_pippenger(s[n:], P, c)]))
    assert np.array_equal(_u(two), want)

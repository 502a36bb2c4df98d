"""GPU parity of the reference C ABI's vector entry points (part 1 of include/cudabulletproof_hip.h)
at every launch shape: block sizes that are no power of two, ragged last waves, the LDS / wave-tail
hand-over, the 1024-block cap and the grid-stride loop's later turns, the reduce's 256 slots, the
batched form's stride, every element of the field ops at counts around the wave and block sizes, and
the MSM's chain-length sort on bins it had not seen.  Expected values are the CPU restatement's
(oracle.ip_gpu*, fe_*, msm_canon); the swept lengths are ip_orders_ref's lists, which
tests/test_ip_orders_ref.py shows to agree with a second, thread-level model of the reference's
kernels and to tell every modelled launch mistake apart.  Inputs are prefixes of one pair of long
vectors of full 256-bit limbs in which every 64-element stretch carries an edge value.

Everything is integer arithmetic and compared with np.array_equal.

Measured wall time on one MI355X (pytest's call durations, the oracle's work included): the
512-call sweep 0.17 s, the 607-call _shared sweep 0.16 s, the 204 grid lengths 0.08 s, the reduce
boundaries with their flips 0.50 s, the second to fourth turns with their flips 0.68 s (its largest
input is 3 * 2^18 + 77 elements, 25 MB per vector); the batched form 0.08 s at 300 vectors and
under 5 ms otherwise; each field-op count under 5 ms after 0.09 s for the shared expected values,
the pool against itself 0.01 s, the square kernel's sets 0.03 s; each MSM case 0.41-0.50 s and each
msm_batch case 0.41-0.82 s, nearly all of it the oracle's msm_canon.  The module's first test also
pays 1.5 s of setup (the library, the device, the 2 x 25 MB draw).  31 tests, 7.7 s in all; none is
near 10 s, so nothing is split.
"""
import ctypes
import itertools

import numpy as np
import pytest

import ip_orders_ref as ref

pytestmark = pytest.mark.gpu

P = ref.P25519
M64 = 2**64 - 1


@pytest.fixture(scope="module")
def ab():
    """The one long (a, b) pair; every case is a prefix of it, and no test changes it."""
    a, b = ref.draw_inputs(ref.MAX_N)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


# ------------------------------------------------------------------ a. the shared path
def test_inner_product_every_n_to_512(bp, oracle, ab):
    """cuda_field_vector_inner_product for every n in 1..512: k_ip_shared with blockDim = n."""
    a, b = ab
    bad = [n for n in ref.DISPATCH_N
           if not np.array_equal(bp.cuda_field_vector_inner_product(a[:n], b[:n]), oracle.ip_gpu(a[:n], b[:n]))]
    assert not bad, bad


def test_inner_product_shared_every_n(bp, oracle, ab):
    """cuda_field_vector_inner_product_shared for every n in 1..600, around 768 and 1024, and 5000:
    above 512 one block of 512 threads, elements from 512 on unread."""
    a, b = ab
    bad = [n for n in ref.SHARED_GPU_N
           if not np.array_equal(bp.cuda_field_vector_inner_product(a[:n], b[:n], shared=True),
                                 oracle.ip_gpu(a[:n], b[:n], shared=True))]
    assert not bad, bad
    n = 5000   # ... unread: the tail does not reach the result, on the GPU as in the restatement
    a2 = a[:n].copy()
    a2[512:] ^= np.uint64(1)
    assert np.array_equal(bp.cuda_field_vector_inner_product(a2, b[:n], shared=True),
                          oracle.ip_gpu(a[:n], b[:n], shared=True))


# ------------------------------------------------------------------ b. the grid path
def _grid_sweep(bp, oracle, ab, ns):
    a, b = ab
    return [n for n in ns
            if not np.array_equal(bp.cuda_field_vector_inner_product(a[:n], b[:n]), oracle.ip_gpu(a[:n], b[:n]))]


def test_grid_3_to_70_blocks(bp, oracle, ab):
    """n = 256 nb - r, nb = 3..70, r in {0, 1, 255}: full, one-short and one-element last blocks;
    k_ip_reduce's guard at every partial count below its 256 slots."""
    ns = [n for n in ref.GRID_N if n <= 70 * 256]
    assert len(ns) == 68 * 3
    assert not _grid_sweep(bp, oracle, ab, ns)


def _flip(v, idx):
    v[idx, 1] ^= np.uint64(1 << 20)


def _grid_with_flips(bp, oracle, ab, ns):
    """GPU == oracle at each n, and again with one bit of a and b flipped in the last live element
    and in the first dead one (where the model says there is one): the oracle's result moves or
    stays as the model's live set says, and the GPU follows."""
    a, b = ab
    a2, b2 = a.copy(), b.copy()
    bad = []
    for n in ns:
        want = oracle.ip_gpu(a[:n], b[:n])
        if not np.array_equal(bp.cuda_field_vector_inner_product(a[:n], b[:n]), want):
            bad.append((n, "as drawn"))
        if n <= 65536:
            continue
        live = ref.ip_grid(None, a, b, n)[1]
        dead = np.setdiff1d(np.arange(n), live, assume_unique=True)
        for what, idx in (("last live", int(live[-1])), ("first dead", int(dead[0]) if len(dead) else None)):
            if idx is None:
                continue
            _flip(a2, idx), _flip(b2, idx)
            moved = oracle.ip_gpu(a2[:n], b2[:n])
            got = bp.cuda_field_vector_inner_product(a2[:n], b2[:n])
            _flip(a2, idx), _flip(b2, idx)
            if np.array_equal(moved, want) != (what == "first dead"):
                bad.append((n, what, idx, "the oracle disagrees with the model's live set"))
            if not np.array_equal(got, moved):
                bad.append((n, what, idx))
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    assert not bad, bad


def test_grid_reduce_slot_boundaries(bp, oracle, ab):
    """255, 256, 257, 1023 and 1024 blocks, each with a full and a ragged last block: k_ip_reduce
    reads 256 partials, and blocks 256.. are dead."""
    ns = [n for n in ref.GRID_N if 70 * 256 < n < ref.TURN]
    assert len(ns) == 9   # (1024 full blocks is n = 262144, swept with the second turn)
    _grid_with_flips(bp, oracle, ab, ns)


def test_grid_second_and_later_turns(bp, oracle, ab):
    """n >= 262144: the capped grid's threads take a second, third and fourth turn."""
    ns = [n for n in ref.GRID_N if n >= ref.TURN]
    assert len(ns) == 8 and max(ns) == 3 * ref.TURN + 77
    _grid_with_flips(bp, oracle, ab, ns)


# ------------------------------------------------------------------ c. the batched form
def _batch(ab, n, nv):
    a, b = ab
    return a[:n * nv].reshape(nv, n, 4), b[:n * nv].reshape(nv, n, 4)


@pytest.mark.parametrize("nv", [1, 5, 300])
def test_batch_inner_product_shapes(bp, oracle, ab, nv):
    bad = []
    for n, k in ref.BATCH_CASES:
        if k == nv:
            a, b = _batch(ab, n, nv)
            if not np.array_equal(bp.cuda_batch_field_vector_inner_product(a, b), oracle.ip_gpu_batch(a, b)):
                bad.append(n)
    assert not bad, bad


def test_batch_inner_product_second_turn(bp, oracle, ab):
    """Two vectors of n >= 262144: the stride nb * 256 is capped at 1024 blocks, and x-block 0 turns again."""
    cases = [c for c in ref.BATCH_CASES if c[0] >= ref.TURN]
    assert len(cases) == 3
    bad = []
    for n, nv in cases:
        a, b = _batch(ab, n, nv)
        if not np.array_equal(bp.cuda_batch_field_vector_inner_product(a, b), oracle.ip_gpu_batch(a, b)):
            bad.append(n)
    assert not bad, bad


def test_batch_inner_product_takes_vector_0s_length(bp, oracle, ab):
    """Raw C ABI: later FieldVectors longer than vector 0; every vector is taken at vector 0's
    length (cuda_inner_product.cu:306) and the extra elements are ignored."""
    a, b = ab
    n, lens = 257, [257, 300, 1000, 258, 257]
    offs = np.concatenate([[0], np.cumsum(lens)])
    FV = bp.FieldVector
    av = (FV * len(lens))(*[FV(a.ctypes.data + 32 * int(o), l) for o, l in zip(offs, lens)])
    bv = (FV * len(lens))(*[FV(b.ctypes.data + 32 * int(o), l) for o, l in zip(offs, lens)])
    out = np.zeros((len(lens), 4), np.uint64)
    bp.lib().cuda_batch_field_vector_inner_product(ctypes.c_void_p(out.ctypes.data), av, bv,
                                                   ctypes.c_size_t(len(lens)))
    want = oracle.ip_gpu_batch(np.stack([a[o:o + n] for o in offs[:-1]]), np.stack([b[o:o + n] for o in offs[:-1]]))
    assert np.array_equal(out, want)


# ------------------------------------------------------------------ d. the field ops
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)


@pytest.fixture(scope="module")
def field_want(oracle, ab):
    """Per-element expected results over the longest count, computed once; shorter counts are prefixes."""
    a, b = ab
    n = max(COUNTS)
    f, g = a[:n], b[:n]
    return {"add": np.stack([oracle.fe_add(f[i], g[i]) for i in range(n)]),
            "sub": np.stack([oracle.fe_sub(f[i], g[i]) for i in range(n)]),
            "mul": np.stack([oracle.fe_mul(f[i], g[i]) for i in range(n)]),
            "square": np.stack([oracle.fe_square_kernel(f[i]) for i in range(n)]),
            "invert": np.stack([oracle.fe_invert(f[i]) for i in range(n)]),
            "soa": f + g}   # limbwise u64 add, wraps, no carry (cuda_field_ops.cu:521)


def _ops(bp):
    return {"add": bp.cuda_batch_field_add, "sub": bp.cuda_batch_field_sub, "mul": bp.cuda_batch_field_mul,
            "karatsuba": bp.cuda_batch_field_mul_karatsuba, "square": bp.cuda_batch_field_square,
            "invert": bp.cuda_batch_field_invert, "soa": bp.cuda_soa_field_add}


UNARY = ("square", "invert")


@pytest.mark.parametrize("count", COUNTS)
def test_field_ops_every_element(bp, ab, field_want, count):
    a, b = ab
    f, g = a[:count], b[:count]
    bad = []
    for name, op in _ops(bp).items():
        got = op(f) if name in UNARY else op(f, g)
        want = field_want["mul" if name == "karatsuba" else name][:count]
        if not np.array_equal(got, want):
            bad.append((name, np.flatnonzero((got != want).any(axis=1))[:8].tolist()))
    assert not bad, bad


def test_field_binary_ops_edge_pool_squared(bp, oracle):
    """Every pool value against every pool value, through add, sub, mul, mul_karatsuba and soa add."""
    pool = ref.edge_pool()
    k = len(pool)
    f, g = np.repeat(pool, k, axis=0), np.tile(pool, (k, 1))
    assert f.shape == (k * k, 4) and k >= 12
    ops = _ops(bp)
    for name, fn in (("add", oracle.fe_add), ("sub", oracle.fe_sub), ("mul", oracle.fe_mul), ("karatsuba", oracle.fe_mul)):
        want = np.stack([fn(f[i], g[i]) for i in range(k * k)])
        got = ops[name](f, g)
        assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1))[:8].tolist())
    assert np.array_equal(ops["soa"](f, g), f + g)
    for name, fn in (("square", oracle.fe_square_kernel), ("invert", oracle.fe_invert)):
        assert np.array_equal(ops[name](pool), np.stack([fn(x) for x in pool])), name


def square_kernel_int(limbs):
    """field_square_kernel (cuda_field_ops.cu:147-216) on four Python-integer limbs -> (limbs, branch):
    branch is "carry" (the fold's last carry, :203), "gt" (t[3] > p[3]), "eq" (t[3] == p[3]: the
    compare chain at :204-206 decides) or "none" (no reduction, :213-217)."""
    a = [int(x) for x in limbs]
    t = [0] * 8
    for i in range(4):
        diag = a[i] * a[i]                                   # :173
        t[i + i] = (t[i + i] + (diag & M64)) & M64           # :174, no carry out
        if i + i + 1 < 8:
            t[i + i + 1] = (t[i + i + 1] + (diag >> 64)) & M64   # :175
        for j in range(i + 1, 4):
            m = (2 * (a[i] * a[j])) & (2**128 - 1)           # :179, the doubling's top bit is dropped
            t[i + j] = (t[i + j] + (m & M64)) & M64          # :180
            if i + j + 1 < 8:
                t[i + j + 1] = (t[i + j + 1] + (m >> 64)) & M64   # :181
    p = [P >> (64 * i) & M64 for i in range(4)]
    c = (t[4] * 19) & M64                                    # :192
    t[0] = (t[0] + c) & M64
    carry = 1 if t[0] < c else 0                             # :194
    for i in range(1, 4):
        c = (t[i + 4] * 19 + carry) & M64                    # :197
        t[i] = (t[i] + c) & M64
        carry = 1 if t[i] < c else 0                         # :199
    if carry:
        branch = "carry"
    elif t[3] > p[3]:
        branch = "gt"
    elif t[3] == p[3]:
        branch = "eq"
    else:
        branch = "none"
    if carry or t[3] > p[3] or (t[3] == p[3] and (t[2] > p[2] or (t[2] == p[2] and (
            t[1] > p[1] or (t[1] == p[1] and t[0] >= p[0]))))):   # :203-206
        carry, out = 0, []
        for i in range(4):
            out.append((t[i] - p[i] - carry) & M64)          # :209
            carry = 1 if t[i] < ((p[i] + carry) & M64) else 0    # :210, p[i] + carry wraps to 0
        return out, branch
    return t[:4], branch


def t3_equals_p3_inputs():
    """Two-limb inputs (a0, 0, 0, a3) on which the fold leaves t[3] == p[3] with no carry.  With only
    limbs 0 and 3 set, t[3] = lo(2 a0 a3) + 19 hi(a3^2) (t[2]'s step cannot carry), so for an odd a3
    whose hi(a3^2) is odd and below 2^63 / 19, a0 = (2^63 - 1 - 19 hi(a3^2)) / 2 / a3 mod 2^63."""
    out, a3 = [], 2**61 + 12345
    while len(out) < 4:
        a3 += 2
        hi = (a3 * a3) >> 64
        if hi % 2 == 0:
            continue
        assert 19 * hi < 2**63
        a0 = (2**63 - 1 - 19 * hi) // 2 * pow(a3, -1, 2**63) % 2**63
        out.append([a0, 0, 0, a3])
        out.append([a0 + 2**63, 0, 0, a3])                   # (2 a0 a3 mod 2^64 is the same)
    return np.array(out, np.uint64)


def test_square_kernel_structured_inputs(bp, oracle):
    """cuda_batch_field_square on limbs from {0, 1, 2^63, 2^64 - 1} in every combination (256 inputs:
    the 2 a_i a_j doubling overflows 128 bits, the inter-limb carries are dropped), on constructed
    inputs that leave t[3] == p[3], and on random ones.  A Python-integer restatement of
    cuda_field_ops.cu:147-216 names the branch each input takes: the set reaches the reduction's
    carry branch, t[3] > p[3], t[3] == p[3] and the no-reduction branch, and plain random inputs
    meet the first, second and last on at least 10 % each.  t[3] == p[3] with the chain deciding
    for the reduction (t[2] = t[1] = 2^64 - 1, t[0] >= 2^64 - 19) was not constructed: the inputs
    here take the chain's first comparison and leave unreduced."""
    vals = (0, 1, 2**63, 2**64 - 1)
    structured = np.array(list(itertools.product(vals, repeat=4)), np.uint64)
    assert structured.shape == (256, 4)
    eq = t3_equals_p3_inputs()
    rnd = np.random.default_rng(147).integers(0, 2**64, size=(3000, 4), dtype=np.uint64)
    x = np.concatenate([structured, eq, rnd])
    model = [square_kernel_int(r) for r in x]
    want = np.stack([oracle.fe_square_kernel(r) for r in x])
    assert np.array_equal(np.array([m[0] for m in model], np.uint64), want)   # the restatements agree
    br = np.array([m[1] for m in model])
    assert {"carry", "gt", "none"} <= set(br[:256])
    assert (br[256:256 + len(eq)] == "eq").all() and len(eq) >= 4
    for name in ("carry", "gt", "none"):
        assert (br[-3000:] == name).mean() >= 0.10, name
    # the doubling's dropped bit: 2 a_i a_j >= 2^128 somewhere in the structured set
    assert any(2 * int(r[i]) * int(r[j]) >= 2**128 for r in structured for i in range(4) for j in range(i + 1, 4))
    got = bp.cuda_batch_field_square(x)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8].tolist()


def test_field_ops_results_alias_a(bp, ab, field_want):
    """One call per op with `results` the same host buffer as `a`."""
    a, b = ab
    n = 257
    L = bp.lib()
    for name in ("add", "sub", "mul", "karatsuba", "square", "invert", "soa"):
        buf, g = a[:n].copy(), b[:n].copy()
        fn = getattr(L, "cuda_soa_field_add" if name == "soa" else
                     "cuda_batch_field_mul_karatsuba" if name == "karatsuba" else "cuda_batch_field_" + name)
        pb = ctypes.c_void_p(buf.ctypes.data)
        if name in UNARY:
            fn(pb, pb, ctypes.c_size_t(n))
        else:
            fn(pb, pb, ctypes.c_void_p(g.ctypes.data), ctypes.c_size_t(n))
        assert np.array_equal(buf, field_want["mul" if name == "karatsuba" else name][:n]), name
        assert np.array_equal(g, b[:n])


# ------------------------------------------------------------------ e. the MSM's chain-length sort
def msm_scalars(m, seed):
    """m scalars of shuffled classes: zero (bin 0), 2^256 - 1 (bin 512), single bits 0, 63, 64 and
    255, one-limb, random, one value repeated more than 1024 times (a bin wider than a scatter
    block), and values whose chain length occurs once."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2**64, size=(m, 4), dtype=np.uint64)
    rep = ref.fe_int(0x0123456789ABCDEF_0F1E2D3C4B5A6978_1122334455667788_99AABBCCDDEEFF01)
    fixed = [ref.fe_int(1 << k) for k in (0, 63, 64, 255)]
    fixed += [ref.fe_int((1 << k) - 1) for k in (2, 9, 77, 130, 201)]   # chain lengths met once
    fixed += [ref.fe_int(2**256 - 1)] * 3
    order = rng.permutation(m)
    nrep = 1100 if m >= 4000 else m // 4
    s[order[:nrep]] = rep
    k = nrep
    s[order[k:k + m // 16]] = 0
    k += m // 16
    s[order[k:k + m // 16], 1:] = 0                                      # one limb
    k += m // 16
    s[order[k:k + len(fixed)]] = np.stack(fixed)
    assert k + len(fixed) < m // 2
    return s


@pytest.fixture(scope="module")
def msm_points(oracle):
    return oracle.base_points(5000, 29)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 5000])
def test_msm_sort_threshold_and_bins(bp, oracle, msm_points, n):
    """cuda_point_vector_multi_scalar_mul just below, at and above MSM_SORT_MIN = 4096."""
    P_, s = msm_points[:n], msm_scalars(n, n)
    if n >= 4096:
        cnt = np.unique(s, axis=0, return_counts=True)[1]
        assert cnt.max() > 1024 and (s == 0).all(axis=1).any() and (s == np.uint64(M64)).all(axis=1).any()
    assert np.array_equal(bp.cuda_point_vector_multi_scalar_mul(s, P_), oracle.msm_canon(s, P_))


@pytest.mark.parametrize("n,count", [(1024, 4), (1365, 3), (1366, 3), (4097, 2)])
def test_msm_batch_across_sort_threshold(bp, oracle, msm_points, n, count):
    """hipbp_msm_batch with count * n at 4096, just below (4095) and above (4098, 8194): item i of
    the sorted order takes point perm[i] % n."""
    import torch
    P_, s = msm_points[:n], msm_scalars(n * count, 7 * n + count)
    dev = torch.device("cuda:0")
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.uint64).view(np.int64)).to(dev)
    out = torch.zeros(count, 16, dtype=torch.int64, device=dev)
    bp.msm_batch(out, T(s), T(P_))
    torch.cuda.synchronize()
    out = out.cpu().numpy().view(np.uint64)
    bad = [k for k in range(count) if not np.array_equal(out[k], oracle.msm_canon(s[k * n:(k + 1) * n], P_))]
    assert not bad, bad

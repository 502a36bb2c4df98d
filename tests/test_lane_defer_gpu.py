"""The lane loops' deferred rare-edge and gate tests on the device (ge25519_dev.h *_d forms,
fe25519_dev.h LAT 3), bit for bit against the CPU restatement.

* Field hooks (bp.field_op *_acc): four waves of 63 common lanes, near-edge words among them, and one
  lane on an edge each; the element's running words must report the edge and the gated form's result
  must come out.
* Forced recovery (bp.sm_probe): the deferred pass made to report a hit after its first chunk, so
  ordinary inputs take the rerun with the gated forms: the same bits as the normal pass.
* Gate failure through the MSM: one lane per wave has a base whose T, Z or Y+X has a top word above
  MUL_BOUNDED_WORD, so the product gate fails at that lane's every add.
"""
import numpy as np
import pytest

from test_fixup_forms_gpu import INV19, M32, _flagged, _lanes, _limbs, _w

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
BOUND = 0xFFFFFFEF   # mul512_asm.h MUL_BOUNDED_WORD


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda:0")


def _field(bp, kind, a, b=None):
    import torch
    r = torch.empty(len(a), 4, dtype=torch.int64, device="cuda:0")
    bp.field_op(kind, r, _T(a), _T(b) if b is not None else None)
    torch.cuda.synchronize()
    return r.cpu().numpy().view(np.uint64)


def _int(f):
    return sum(int(f[i]) << (64 * i) for i in range(4))


# kind -> (the generator's kind for tests/test_fixup_forms_gpu._lanes, the oracle's operation)
EDGE_KINDS = {"add_acc": ("add", "add"), "fold_acc": ("fold", "fold"), "addsub_acc_add": ("addsub_add", "add"),
              "addsub_acc_sub": ("addsub_sub", "sub"), "sub_acc": ("addsub_sub", "sub")}


def _want(oracle, op, a, b):
    from test_gpu_parity import _ref_fold
    if op == "fold":
        return _ref_fold([int(x) for x in a] + [int(x) for x in b])
    return [int(x) for x in getattr(oracle, "fe_" + op)(a, b)]


@pytest.mark.parametrize("kind", list(EDGE_KINDS))
def test_deferred_field_forms_on_the_add_side_edges(bp, oracle, kind):
    """h1 or h4 == 2^32-1 in one lane of each wave; the common lanes carry 0 and 2^32-2 there."""
    gen, op = EDGE_KINDS[kind]
    lanes = _lanes(gen, np.random.default_rng(300 + list(EDGE_KINDS).index(kind)))[1024:]
    assert len(lanes) == 256
    flags = [_flagged(gen, a, b) for a, b, _, _ in lanes]
    assert [sum(flags[64 * k:64 * k + 64]) for k in range(4)] == [1, 1, 1, 1]
    assert any(M32 - 1 in (_w(h, 1), _w(h, 4)) for _, _, _, h in lanes)   # near-edge words that must not flag
    a = np.array([_limbs(x) for x, _, _, _ in lanes], dtype=np.uint64)
    if op == "fold":   # the device forms x_i = lo64(19 t_hi_i) itself
        b = np.array([[(v * INV19) & M64 for v in _limbs(x)] for _, x, _, _ in lanes], dtype=np.uint64)
    else:
        b = np.array([_limbs(x) for _, x, _, _ in lanes], dtype=np.uint64)
    got = _field(bp, kind, a, b)
    for i in range(256):
        assert [int(x) for x in got[i]] == _want(oracle, op, a[i], b[i]), (kind, i)


@pytest.mark.parametrize("kind", ["addsub_acc_add", "addsub_acc_sub", "sub_acc"])
def test_deferred_field_forms_on_the_sub_side_edges(bp, oracle, kind):
    """One lane per wave on one of fe25519_sub's edges: g_1's low word all ones, t0 < 19 under a final
    borrow (t's word 1 is 0), t1 or t2 with an all-ones low word."""
    gen, op = EDGE_KINDS[kind]
    rng = np.random.default_rng(400 + len(kind))
    common = _lanes(gen, rng)[:256]
    assert not any(_flagged(gen, a, b) for a, b, _, _ in common)
    pairs = [(a, b) for a, b, _, _ in common]
    R = lambda: int.from_bytes(rng.bytes(32), "little")
    edges = []
    b = R() | (M32 << 64)                                    # g_1's low word (word 2) all ones
    edges.append((R(), b))
    t = (R() & ~((1 << 64) - 1)) | 7                         # t0 = 7 < 19, word 1 = 0
    b = R() | (1 << 255)
    edges.append(((t + b) % 2**256, b))
    for word in (2, 4):                                      # t's word 2 / word 4 all ones
        t = R() | (M32 << (32 * word))
        b = R()
        edges.append(((t + b) % 2**256, b))
    for wv, e in enumerate(edges):
        assert _flagged("addsub", *e)
        pairs[64 * wv + (wv * 29 + 3) % 64] = e
    a = np.array([_limbs(x) for x, _ in pairs], dtype=np.uint64)
    b = np.array([_limbs(x) for _, x in pairs], dtype=np.uint64)
    got = _field(bp, kind, a, b)
    for i in range(256):
        assert [int(x) for x in got[i]] == _want(oracle, op, a[i], b[i]), (kind, i)


@pytest.mark.parametrize("kind", ["mul_acc", "sq_acc"])
def test_deferred_products_on_the_gate(bp, oracle, kind):
    """a0 / b7 (the square: a0 / a7) at MUL_BOUNDED_WORD and just below in the common lanes, above it in
    one lane per wave: that element's gacc reports the failed gate and the counting product runs."""
    rng = np.random.default_rng(500 + len(kind))
    a = rng.integers(0, 2**64, size=(256, 4), dtype=np.uint64)
    b = rng.integers(0, 2**64, size=(256, 4), dtype=np.uint64)
    near = [BOUND, BOUND - 1, 0, 0x7FFFFFFF]
    lo = lambda f, v: (f & np.uint64(0xFFFFFFFF00000000)) | np.uint64(v)          # word 0 of a limb
    hi = lambda f, v: (f & np.uint64(0x00000000FFFFFFFF)) | np.uint64(v << 32)    # word 1 of a limb
    top = a if kind == "sq_acc" else b
    for i in range(256):
        a[i, 0] = lo(a[i, 0], near[i % 4] if i % 3 == 0 else int(a[i, 0]) & 0xFFFFFFFF & BOUND)
        top[i, 3] = hi(top[i, 3], near[(i // 4) % 4] if i % 5 == 0 else (int(top[i, 3]) >> 32) & BOUND)
    for wv, (w0, w7) in enumerate([(BOUND + 1, None), (None, 0xFFFFFFF0), (M32, None), (None, M32)]):
        i = 64 * wv + (wv * 23 + 9) % 64
        if w0 is not None:
            a[i, 0] = lo(a[i, 0], w0)
        else:
            top[i, 3] = hi(top[i, 3], w7)
    fails = [max(int(a[i, 0]) & M32, int(top[i, 3]) >> 32) > BOUND for i in range(256)]
    assert [sum(fails[64 * k:64 * k + 64]) for k in range(4)] == [1, 1, 1, 1]
    got = _field(bp, kind, a, None if kind == "sq_acc" else b)
    for i in range(256):
        want = oracle.fe_mul(a[i], a[i] if kind == "sq_acc" else b[i])
        assert [int(x) for x in got[i]] == [int(x) for x in want], (kind, i)


# ----------------------------------------------------------------------------- the loops
def _points(rng, n, affine):
    P = rng.integers(0, 2**64, size=(n, 16), dtype=np.uint64)
    if affine:
        P[:, 8:12] = 0
        P[:, 8] = 1
    return P


def _probe(bp, force, s, P):
    import torch
    out = torch.zeros(len(s), 16, dtype=torch.int64, device="cuda:0")
    bp.sm_probe(force, out, _T(s), _T(P))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _sm_oracle(oracle, s, P):
    return np.stack([np.asarray(oracle.ge_scalarmult(np.ascontiguousarray(s[i]).view(np.uint8), P[i]), np.uint64)
                     for i in range(len(s))])


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("affine", [True, False])
def test_forced_recovery_gives_the_same_bits(bp, oracle, shared, affine):
    """128 random (scalar, point) pairs, two waves: per-lane scalars (sm_lane_loop_d) or one scalar for
    all (sm_uniform_d), Z = 1 (the zone forms) or Z != 1."""
    rng = np.random.default_rng(600 + 2 * shared + affine)
    s = rng.integers(0, 2**64, size=(128, 4), dtype=np.uint64)
    if shared:
        s[:] = s[0]
    else:
        s[5] = 0                      # no step at all
        s[70, 1:] = 0                 # a short scalar in a wave of long ones
    P = _points(rng, 128, affine)
    normal, forced = _probe(bp, 0, s, P), _probe(bp, 1, s, P)
    assert np.array_equal(normal, forced)
    assert np.array_equal(normal, _sm_oracle(oracle, s, P))


def _with_top_word(rng, oracle, coord, word):
    """A point whose T, Z or Y + X (the prepared operand, fe25519_add's result) has top word `word`."""
    P = _points(rng, 1, coord != "Z")[0]
    if coord in ("T", "Z"):
        col = 12 if coord == "T" else 8
        P[col + 3] = (P[col + 3] & np.uint64(0xFFFFFFFF)) | np.uint64(word << 32)
        return P
    # Y + X = h + 2^256 with h's top word = word - 2^31: the sum carries out, so the fix-up adds 2^63
    h = (int.from_bytes(rng.bytes(32), "little") & ((1 << 224) - 1)) | ((word - 0x80000000) << 224)
    h &= ~(M32 << 32) & ~(M32 << 128)          # off the fix-up's own edges (h1, h4 not all ones)
    Y = h + 1 + int.from_bytes(rng.bytes(32), "little") % (2**256 - h - 1)
    X = h + 2**256 - Y
    P[0:4], P[4:8] = _limbs(X), _limbs(Y)
    assert int(oracle.fe_add(P[4:8], P[0:4])[3]) >> 32 == word
    return P


@pytest.mark.parametrize("affine", [True, False])
def test_gate_failure_through_the_msm(bp, oracle, affine):
    """128 points, two waves; lanes 9 and 64 + 40 carry a base whose gate word is above the bound."""
    import torch
    rng = np.random.default_rng(700 + affine)
    s = rng.integers(0, 2**64, size=(128, 4), dtype=np.uint64)
    plain = _points(rng, 128, affine)
    quirk = plain.copy()
    lanes = (9, 64 + 40)
    specs = [("T", 0xFFFFFFF0), ("Y+X", M32)] if affine else [("Z", M32), ("Y+X", 0xFFFFFFF0)]
    for lane, (coord, word) in zip(lanes, specs):
        quirk[lane] = _with_top_word(rng, oracle, coord, word)
    out = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    bp.msm(out, _T(s), _T(quirk))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), oracle.msm_canon(s, quirk))
    # per lane (the raw scalar multiplications): the quirk lanes against the oracle, and every other
    # lane keeps the bits it has without the quirk
    got, ref = _probe(bp, 0, s, quirk), _probe(bp, 0, s, plain)
    other = [i for i in range(128) if i not in lanes]
    assert np.array_equal(got[other], ref[other])
    assert np.array_equal(got, _sm_oracle(oracle, s, quirk))

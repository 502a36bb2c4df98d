"""The fast fix-up of the field asm (field_asm.h: m1, then limb 0 += 19 m as one 64-bit multiply-add,
h4 += m, h7 += m << 31) on the device, through bp.field_op: 16 waves whose every lane is a common
one, so the fast statements are what runs, with sums on the fix-up's word patterns; then 4 waves
with one rare lane each (h4 or h1 == 2^32-1), which must take the exact form and still match."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M32, M64 = 2**32 - 1, 2**64 - 1
INV19 = pow(19, -1, 2**64)
H0 = (0, 2**32 - 20, 2**32 - 19, 2**32 - 1)
H1 = (0, 2**32 - 2)
H4 = (0, 2**32 - 2)
H7 = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
KINDS = ["add", "fold", "addsub_add", "addsub_sub", "add_lat", "fold_lat", "addsub_lat_add", "add_defer", "fold_defer"]


def _w(x, i):
    return (x >> (32 * i)) & M32


def _flagged(kind, a, b):
    """The rare-edge test of the block that `kind` runs (tools/gen_field_asm.py), on the operands:
    add / fold: h1 or h4 all ones (fold: or a low word of x_1..x_3); add/sub: also sub's tests."""
    h = (a + b) % 2**256
    f = _w(h, 1) == M32 or _w(h, 4) == M32
    if kind.startswith("fold"):
        f = f or M32 in (_w(b, 2), _w(b, 4), _w(b, 6))
    if kind.startswith("addsub"):
        t = (a - b) % 2**256
        f = f or M32 in (_w(b, 2), _w(b, 4), _w(b, 6), _w(t, 2), _w(t, 4)) or _w(t, 1) == 0
    return f


def _operands(kind, rng, h, carry, want_flag):
    """a, b < 2^256 with a + b = h + carry 2^256 (fold: b = x, the words of lo64(19 t_hi))."""
    for _ in range(64):
        lo, hi = (h + 1, 2**256) if carry else (0, h + 1)
        a = lo + int.from_bytes(rng.bytes(32), "little") % (hi - lo)
        b = h + (carry << 256) - a
        assert 0 <= a < 2**256 and 0 <= b < 2**256
        if _flagged(kind, a, b) == want_flag:
            return a, b
    raise AssertionError("no operands found")


def _limbs(x):
    return [(x >> (64 * k)) & M64 for k in range(4)]


def _lanes(kind, rng):
    """[(a, b, carry, h)]: 16 common waves over the cross product of the edge words, 8 lanes each, then
    4 waves of 63 common lanes and one rare lane at a rotating position."""
    common = []
    for rep in range(8):
        for h0 in H0:
            for h1 in H1:
                for h4 in H4:
                    for h7 in H7:
                        for carry in (0, 1):
                            w = [h0, h1, int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), h4,
                                 int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), h7]
                            h = sum(x << (32 * i) for i, x in enumerate(w))
                            common.append(_operands(kind, rng, h, carry, False) + (carry, h))
    assert len(common) == 16 * 64
    lanes = list(common)
    for wv, (h1, h4) in enumerate([(0, M32), (M32, 0), (2**32 - 2, M32), (M32, 2**32 - 2)]):
        wave = common[64 * wv + 1:64 * wv + 64]
        w = [H0[wv], h1, int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), h4,
             int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), H7[wv]]
        h = sum(x << (32 * i) for i, x in enumerate(w))
        wave.insert((wv * 37 + 5) % 64, _operands(kind, rng, h, wv & 1, True) + (wv & 1, h))
        lanes += wave
    return lanes


@pytest.mark.parametrize("kind", KINDS)
def test_fast_fixup_forms(bp, oracle, kind):
    import torch
    from test_gpu_parity import _ref_fold
    rng = np.random.default_rng(100 + KINDS.index(kind))
    lanes = _lanes(kind, rng)
    N = len(lanes)
    assert N == 20 * 64
    # no rare lane in the first 16 waves, exactly one in each of the last 4; every combination of
    # carry-out and bit 255 among the common lanes
    flags = [_flagged(kind, a, b) for a, b, _, _ in lanes]
    assert not any(flags[:1024]) and [sum(flags[1024 + 64 * k:1088 + 64 * k]) for k in range(4)] == [1, 1, 1, 1]
    assert {(c, h >> 255) for _, _, c, h in lanes[:1024]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for a, b, c, h in lanes:
        assert a + b == h + (c << 256)
    a = np.array([_limbs(x) for x, _, _, _ in lanes], dtype=np.uint64)
    if kind.startswith("fold"):   # the device forms x_i = lo64(19 t_hi_i) itself
        b = np.array([[(v * INV19) & M64 for v in _limbs(x)] for _, x, _, _ in lanes], dtype=np.uint64)
    else:
        b = np.array([_limbs(x) for _, x, _, _ in lanes], dtype=np.uint64)
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    r = torch.empty(N, 4, dtype=torch.int64, device=dev)
    bp.field_op(kind, r, T(a), T(b))
    torch.cuda.synchronize()
    got = r.cpu().numpy().view(np.uint64)
    op = kind.replace("_lat", "").replace("_defer", "")
    for i in range(N):
        if op == "fold":
            want = _ref_fold([int(x) for x in a[i]] + [int(x) for x in b[i]])
        else:
            want = [int(x) for x in getattr(oracle, "fe_" + op.replace("addsub_", ""))(a[i], b[i])]
        assert [int(x) for x in got[i]] == want, (kind, i, [hex(int(x)) for x in a[i]], [hex(int(x)) for x in b[i]])

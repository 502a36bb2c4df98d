"""CPU model of one scalar-multiplication chain of the drain-tick forms (ge25519_quad.h sm_quad / sm_pair /
sm_row), saying at which in-loop steps a field block's rare-edge test or a product's gate fires.  Not a
test file: tests/test_sm_forms_gpu.py uses it to prove, on the CPU, that each constructed case reaches the
path it is named for; tests/test_sm_forms_ref.py checks the model itself.

The chain is walked the way sm_start and the loops walk it: the start state is the identity doubled once
per leading zero bit of the scalar (dtab[lz], outside the loop), the first in-loop step is the doubling at
the top set bit, and every later step is one ge25519_add(r, q) with q = r (a doubling) or q = P (the add
after a doubling at a set bit).  One step, in operand order, over the oracle's fe_add / fe_sub / fe_mul:

  stage 1   A = (Y1-X1)(Y2-X2), B = (Y1+X1)(Y2+X2), CT = T1 T2, D0 = Z1 Z2    (products: gate words)
  C, D      C = CT k (fe_mul_k / fe_mul_q4_k: no gate), D = D0 + D0            (add block)
  E .. H    H = B + A, E = B - A; G = D + C, F = D - C                         (two add/sub blocks)
  stage 3   X3 = E F, Y3 = G H, Z3 = G F, T3 = E H                             (products: gate words)
  next      Y3 - X3, Y3 + X3, the next step's operands; not after the last step (one add/sub block)

A product's gate reads, in the quad and pair steps (fe_mul(x, y)), x's word 0 and y's word 7, and in the row
step (fe_mul_q4(x, y): x's rows split over the quad) x's words 0, 2, 4 and 6; it fails above
MUL_BOUNDED_WORD.  In every step the running point's operand is the first factor and q's the second.
The row step's deferred recompute looks at the blocks inside the step (D and the two add/sub blocks; its
`next` block runs in the latency form), the quad and pair steps run every block gated.
"""
import ctypes

from test_fixup_forms_gpu import _flagged

M32, M64 = 2**32 - 1, 2**64 - 1
MUL_BOUNDED_WORD = 0xFFFFFFEF   # mul512_asm.h
K = int.from_bytes(bytes([0xA3, 0x78, 0x59, 0x13, 0xCA, 0x4D, 0xEB, 0x75, 0xAB, 0xD8, 0x41, 0x41, 0x4D, 0x0A, 0x70, 0x00,
                          0x98, 0xE8, 0x79, 0x77, 0x79, 0x40, 0xC7, 0x8C, 0x73, 0xFE, 0x6F, 0x2B, 0xEE, 0x6C, 0x03, 0x52]),
                   "little")   # ge25519_add's constant (curve25519_ops.cu:326-378)
EDGE_BLOCKS = ("add_D", "addsub_BA", "addsub_DC", "addsub_next")
ROW_BLOCKS = ("add_D", "addsub_BA", "addsub_DC")   # what sm_row's one ballot per step sees of these


def _w(x, i):
    return (x >> (32 * i)) & M32


class _Field:
    """oracle.fe_add / fe_sub / fe_mul on Python integers (the raw 256-bit limb value)."""

    def __init__(self, oracle):
        self._f = {n: oracle.f("fe_" + n) for n in ("add", "sub", "mul")}
        self._a, self._b, self._r = ((ctypes.c_uint64 * 4)() for _ in range(3))

    def _op(self, name, x, y):
        for i in range(4):
            self._a[i] = (x >> (64 * i)) & M64
            self._b[i] = (y >> (64 * i)) & M64
        self._f[name](self._r, self._a, self._b)
        return self._r[0] | (self._r[1] << 64) | (self._r[2] << 128) | (self._r[3] << 192)

    def add(self, x, y):
        return self._op("add", x, y)

    def sub(self, x, y):
        return self._op("sub", x, y)

    def mul(self, x, y):
        return self._op("mul", x, y)


def _gates(pairs):
    """(plain, q4): does some product x y of `pairs` fail the lane forms' gate, the quad-split form's gate."""
    plain = any(max(_w(x, 0), _w(y, 7)) > MUL_BOUNDED_WORD for x, y in pairs)
    q4 = any(max(_w(x, 0), _w(x, 2), _w(x, 4), _w(x, 6)) > MUL_BOUNDED_WORD for x, _ in pairs)
    return plain, q4


def _operands(F, p):
    X, Y, Z, T = p
    return F.sub(Y, X), F.add(Y, X), T, Z


def point_step(F, o, q, last):
    """One ge25519_add from the running point's operands o = (Y1-X1, Y1+X1, T1, Z1) and q's, in operand
    order.  Returns the result (X3, Y3, Z3, T3), the next operands (None after the last step) and the
    step's flags: one bool per block of EDGE_BLOCKS, and gate_st1 / gate_st3 (fe_mul's gate) and
    gate_q4_st1 / gate_q4_st3 (fe_mul_q4's) for the two product stages."""
    st1 = list(zip(o, q))
    A, B, CT, D0 = (F.mul(x, y) for x, y in st1)
    C = F.mul(CT, K)
    fl = {"add_D": _flagged("add", D0, D0)}
    D = F.add(D0, D0)
    fl["addsub_BA"] = _flagged("addsub", B, A)
    H, E = F.add(B, A), F.sub(B, A)
    fl["addsub_DC"] = _flagged("addsub", D, C)
    G, Fm = F.add(D, C), F.sub(D, C)
    st3 = [(E, Fm), (G, H), (G, Fm), (E, H)]
    X3, Y3, Z3, T3 = (F.mul(x, y) for x, y in st3)
    fl["gate_st1"], fl["gate_q4_st1"] = _gates(st1)
    fl["gate_st3"], fl["gate_q4_st3"] = _gates(st3)
    nxt = None
    fl["addsub_next"] = False
    if not last:
        fl["addsub_next"] = _flagged("addsub", Y3, X3)
        nxt = (F.sub(Y3, X3), F.add(Y3, X3), T3, Z3)
    return (X3, Y3, Z3, T3), nxt, fl


def _int(limbs):
    return sum(int(v) << (64 * i) for i, v in enumerate(limbs))


def chain(oracle, scalar, point):
    """The chain of scalar (4 limbs or an int) times point (16 limbs, X | Y | Z | T).  Returns
    (result as 16 ints' worth of four coordinates, steps): steps[j] = dict(op="dbl" | "add", bit=the
    scalar bit the step belongs to, and point_step's flags) for in-loop step j.  Asserts that the result
    is oracle.ge_scalarmult's, limb for limb."""
    import numpy as np
    F = _Field(oracle)
    s = scalar if isinstance(scalar, int) else _int(scalar)
    P = tuple(_int(point[4 * c:4 * c + 4]) for c in range(4))
    qP = _operands(F, P)
    r = (0, 1, 1, 0)
    top = s.bit_length() - 1                   # sm_start: i = 255 - lz, -1 for the zero scalar
    for _ in range(255 - top):                 # dtab[lz]: the identity doubled lz times, outside the loop
        o = _operands(F, r)
        r, _, _ = point_step(F, o, o, True)
    steps = []
    o = _operands(F, r) if top >= 0 else None
    for i in range(top, -1, -1):
        bit = (s >> i) & 1
        r, o, fl = point_step(F, o, o, i == 0 and not bit)
        steps.append(dict(op="dbl", bit=i, **fl))
        if bit:
            r, o, fl = point_step(F, o, qP, i == 0)
            steps.append(dict(op="add", bit=i, **fl))
    got = np.array([(c >> (64 * k)) & M64 for c in r for k in range(4)], dtype=np.uint64)
    s32 = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
    want = np.asarray(oracle.ge_scalarmult(s32, np.ascontiguousarray(point, np.uint64)), np.uint64)
    assert np.array_equal(got, want), "the model's chain is not oracle.ge_scalarmult's"
    return got, steps


def edge_steps(steps, blocks=EDGE_BLOCKS):
    """Indices of the in-loop steps at which a rare-edge test of `blocks` fires."""
    return [j for j, st in enumerate(steps) if any(st[b] for b in blocks)]


def past_first_operation(steps, idx):
    """Those of the step indices `idx` that lie past the chain's first operation, the top set bit's doubling
    and its add.  There every chain sits on small coordinates: the start state is a doubled identity
    (0, y, z, 0), so B - A = 0 in the doubling, and T1 = 0 gives C = 0 in the add, where a base with Z = 1
    leaves D - C = D small; word 1 of the difference is 0, fe25519_sub's rare edge.  After that add the
    state is an ordinary point (the lane loops run these two steps gated for the same reason, DEFER_WARM)."""
    return [j for j in idx if steps[j]["bit"] < steps[0]["bit"]]


def gate_steps(steps, q4=False):
    """Indices of the in-loop steps with a failed product gate: fe_mul's, or (q4) fe_mul_q4's."""
    a, b = ("gate_q4_st1", "gate_q4_st3") if q4 else ("gate_st1", "gate_st3")
    return [j for j, st in enumerate(steps) if st[a] or st[b]]

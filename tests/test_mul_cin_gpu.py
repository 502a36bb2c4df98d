"""The lane forms' products on the *_cin_asm statements (fe25519_dev.h BP_MUL_CIN, mul512_asm.h) on the
device, bit for bit against the CPU restatement.

* Field hooks: the product, the square and the product by k, gated (LAT 0) and deferred (LAT 3), on 256
  elements: four waves of common lanes, gate words at and just below MUL_BOUNDED_WORD among them, one
  lane per wave with a failing gate and, for the product, one lane per wave whose fold sits on an edge
  (h1 or h4 all ones, t0 >= p0, an x_i = 2^64 - 1 under a carry), steered through the second operand
  (1, or 2^192 + 1).  A square's and k's folds cannot be steered; they take the gate lanes and edge words.
* The scalar-mult loops (bp.sm_probe), plain and with the forced recovery pass: one wave of per-lane
  scalars and one of a uniform scalar, with bases whose gate fails at every add among them.
* The pipeline at B = 4, n = 16, K = 8 in its three modes against the oracle's verdicts, P and check
  points.
"""
import numpy as np
import pytest

from test_gpu_parity import P_LIMBS, WRAP19, _check_std_vs_oracle, rand_fe
from test_lane_defer_gpu import BOUND, _field, _points, _probe, _sm_oracle, _with_top_word

pytestmark = pytest.mark.gpu

M32, M64 = 2**32 - 1, 2**64 - 1
K_LIMBS = [0x75EB4DCA135978A3, 0x00700A4D4141D8AB, 0x8CC740797779E898, 0x52036CEE2B6FFE73]


def _limbs(x):
    return [(x >> (64 * i)) & M64 for i in range(4)]


def _fold_edge_pairs(rng):
    """(a, b) whose exact product's fold sits on one edge each; every gate word within the bound."""
    r = lambda: int(rng.integers(0, 2**64, dtype=np.uint64)) & ~0x10
    one = [1, 0, 0, 0]
    # a = 1: the fold is b itself (b's top word is within the bound: the gate words are a0 and b7)
    out = [(one, [r(), r(), (r() & ~M32) | M32, r() >> 1]),              # h4 all ones
           (one, [(r() & M32) | (M32 << 32), r(), r(), r() >> 1]),       # h1 all ones
           (one, [P_LIMBS[0] + 3, M64, M64, P_LIMBS[3]])]                # t0 >= p0 under p's upper limbs
    while True:   # b = 2^192 + 1: t_hi = (a1 + c, a2, a3, 0); a2 = WRAP19 makes x_1 = 2^64 - 1, under limb 0's carry
        a = [r(), r(), WRAP19, r() >> 1]
        t = sum(v << (64 * i) for i, v in enumerate(a)) * ((1 << 192) + 1)
        tl = _limbs(t) + _limbs(t >> 256)
        if (19 * tl[5]) & M64 == M64 and tl[0] + ((19 * tl[4]) & M64) > M64:
            out.append((a, [1, 0, 0, 1]))
            return out


@pytest.mark.parametrize("kind", ["mul", "mul_acc", "sq", "sq_acc", "mul_k"])
def test_products_on_gates_and_fold_edges(bp, oracle, kind):
    rng = np.random.default_rng(800 + len(kind) + kind.count("_"))
    a = rand_fe(rng, 256, top=True)
    b = rand_fe(rng, 256, top=True)
    square, byk = kind.startswith("sq"), kind == "mul_k"
    top = a if square or byk else b
    near = [BOUND, BOUND - 1, 0, M32 >> 1]
    for i in range(256):   # the gate words of the common lanes: within the bound, at it and just below it often
        w0 = near[i % 4] if i % 3 == 0 else int(a[i, 0]) & BOUND
        w7 = near[(i // 4) % 4] if i % 5 == 0 else (int(top[i, 3]) >> 32) & BOUND
        a[i, 0] = np.uint64((int(a[i, 0]) & ~M32) | w0)
        top[i, 3] = np.uint64((int(top[i, 3]) & M32) | (w7 << 32))
    if kind in ("mul", "mul_acc"):
        for wv, (x, y) in enumerate(_fold_edge_pairs(rng)):
            i = 64 * wv + (wv * 19 + 5) % 64
            a[i], b[i] = np.array(x, np.uint64), np.array(y, np.uint64)
    for wv, (w0, w7) in enumerate([(BOUND + 1, None), (None, 0xFFFFFFF0), (M32, None), (None, M32)]):
        i = 64 * wv + (wv * 23 + 9) % 64
        if w0 is not None:
            a[i, 0] = np.uint64((int(a[i, 0]) & ~M32) | w0)
        else:
            top[i, 3] = np.uint64((int(top[i, 3]) & M32) | (w7 << 32))
    fails = [max(int(a[i, 0]) & M32, int(top[i, 3]) >> 32) > BOUND for i in range(256)]
    assert [sum(fails[64 * k:64 * k + 64]) for k in range(4)] == [1, 1, 1, 1]
    got = _field(bp, kind, a, None if square or byk else b)
    other = a if square else np.tile(np.array(K_LIMBS, np.uint64), (256, 1)) if byk else b
    for i in range(256):
        assert [int(x) for x in got[i]] == [int(x) for x in oracle.fe_mul(a[i], other[i])], (kind, i)


@pytest.mark.parametrize("shared", [False, True])
def test_scalar_mult_loops_plain_and_forced(bp, oracle, shared):
    """64 lanes, one wave: per-lane scalars or one scalar for all; Z = 1 bases, two of them with a gate
    word above the bound (T's top word, and Y + X's), so those lanes' gates fail at every add."""
    rng = np.random.default_rng(900 + shared)
    s = rng.integers(0, 2**64, size=(64, 4), dtype=np.uint64)
    if shared:
        s[:] = s[0]
    P = _points(rng, 64, True)
    P[11] = _with_top_word(rng, oracle, "T", 0xFFFFFFF0)
    P[47] = _with_top_word(rng, oracle, "Y+X", M32)
    want = _sm_oracle(oracle, s, P)
    assert np.array_equal(_probe(bp, 0, s, P), want)
    assert np.array_equal(_probe(bp, 1, s, P), want)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pipeline_small_batch_vs_oracle(bp, oracle, mode):
    import torch
    from cudabulletproof_amd import synth
    n, B, K = 16, 4, 8
    G, H = oracle.base_points(n, 1), oracle.base_points(n, 2)
    g, h = oracle.gh()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    arrays = synth.proofs(B, n, seed=77)
    rng = np.random.default_rng(77)
    arrays["taux"], arrays["mu"] = rand_fe(rng, B, top=False), rand_fe(rng, B, top=False)
    Pg = oracle.base_points(B, 9)
    pipe = bp.VerifyPipeline(B, n, T(G), T(H), T(h), range_mode=mode, g=T(g) if mode == 2 else None)
    pipe.prefix_tables(K)
    batch = bp.RangeProofBatch.from_numpy(n, arrays, dev)
    ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    P, chk = (torch.zeros(B, 16, dtype=torch.int64, device=dev) for _ in range(2))
    fl = torch.zeros(B, dtype=torch.uint8, device=dev)
    poly = torch.zeros(B, 4, 16, dtype=torch.int64, device=dev)
    if mode == 0:
        pipe.push(batch, ok, None, chk, P_in=T(Pg))
    elif mode == 1:
        pipe.push(batch, ok, P, chk)
    else:
        pipe.push(batch, ok, P, chk, flags_out=fl, poly_out=poly)
    pipe.flush()
    torch.cuda.synchronize()
    pipe.close()
    u = lambda t: t.cpu().numpy().view(np.uint64)
    okd = ok.cpu().numpy().astype(bool)
    if mode == 2:
        heads = np.concatenate([arrays[k] for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")], axis=1)
        _check_std_vs_oracle(oracle, n, arrays, heads, G, H, g, h, (okd, u(P), u(chk), fl.cpu().numpy(), u(poly)))
        return
    for p in range(B):
        if mode == 0:
            okr, chkr, _, _ = oracle.cuda_inner_product_verify(n, arrays["a"][p], arrays["b"][p], arrays["c"][p], arrays["L"][p],
                                                               arrays["R"][p], arrays["x"][p], Pg[p], G, H, h)
        else:
            head = np.concatenate([arrays[k][p] for k in ("V", "A", "S", "T1", "T2")] +
                                  [np.zeros(8, np.uint64), arrays["t"][p], arrays["c"][p], arrays["x"][p]])
            okr, Pr, chkr, _, _ = oracle.cuda_range_proof_verify(head, arrays["V"][p], n, arrays["a"][p], arrays["b"][p],
                                                                 arrays["L"][p], arrays["R"][p], G, H, g, h)
            assert np.array_equal(u(P)[p], Pr), p
        assert okd[p] == okr and np.array_equal(u(chk)[p], chkr), (mode, p)

"""The per-lane scalar-mult loop's voted step (ge25519_dev.h ge_add_sel: all lanes doubling, all adding,
or the selected stage 1, then the one tail) on the device, bit for bit against the CPU restatement.

* bp.sm_probe, one block of 256 lanes per case.  The wave under test is built once (64 scalars) and laid
  out four times: waves 0 and 1 on Z = 1 bases (the zone forms), waves 2 and 3 on Z != 1 bases; waves 1
  and 3 with the lanes interleaved, so that equal scalars are not neighbours.  The vote is over the wave,
  not over neighbours, so all four agree on the same steps.
* The verify pipeline at B = 4, n = 16 (the reference's proofs of tests/golden) and n = 8 (synthetic
  proofs against the oracle), the lane form forced on every tick (HIPBP_QUAD=0: k_terms<1>), without
  prefix tables and with K = 4 tables: fold rounds 1-3 hold 2, 4 and 8 distinct scalars per proof.
"""
import numpy as np
import pytest

from test_lane_defer_gpu import M32, _T, _points, _probe, _sm_oracle, _with_top_word

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1


def _limbs(x):
    return [(x >> (64 * i)) & M64 for i in range(4)]


def _rand_scalars(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(k)]


def _groups(rng, k):
    """k distinct scalars, 64 / k neighbouring lanes each (the sorted fold rounds' layout)."""
    return [s for s in _rand_scalars(rng, k) for _ in range(64 // k)]


def _wave(name, rng):
    if name in ("2x32", "force", "gate", "edge"):
        return _groups(rng, 2)
    if name == "4x16":
        return _groups(rng, 4)
    if name == "8x8":
        return _groups(rng, 8)
    if name == "64x1":
        return _rand_scalars(rng, 64)
    if name == "63+1":   # not uniform, so the per-lane loop; agrees wherever the two scalars' phases meet
        a, b = _rand_scalars(rng, 2)
        return [a] * 40 + [b] + [a] * 23
    if name == "short":   # chains that end long before the rest: 200 leading zeros, 255, and no bit at all
        full = _groups(rng, 2)
        for lane, lz in ((3, 200), (17, 200), (40, 255), (41, 256), (63, 130)):
            full[lane] = full[lane] >> lz
        return full
    if name == "runs":
        # long all-doubling runs (few set bits) and all-add steps (the set bits shared): four scalars that
        # differ in a handful of low bits only, on a sparse and on a dense common part
        sparse = (1 << 255) | (1 << 190) | (1 << 189) | (1 << 64) | (1 << 20)
        dense = ((1 << 256) - 1) ^ (1 << 200) ^ (1 << 77)
        out = []
        for base in (sparse, dense):
            out += [base] * 16 + [base ^ 0b1011] * 16
        return out
    raise AssertionError(name)


CASES = ["2x32", "4x16", "8x8", "64x1", "63+1", "short", "runs", "force", "gate", "edge"]


def _block(name, oracle):
    """(scalars (256, 4), points (256, 16)) of one case."""
    rng = np.random.default_rng(1400 + CASES.index(name))
    w = _wave(name, rng)
    assert len(w) == 64 and len(set(w)) > 1          # never the uniform loop
    mixed = [w[(i % 8) * 8 + i // 8] for i in range(64)]
    s = np.array([_limbs(x) for x in w + mixed + w + mixed], dtype=np.uint64)
    P = np.concatenate([_points(rng, 128, True), _points(rng, 128, False)])
    if name == "gate":   # one lane per wave whose base fails the product gate at every add
        specs = [("T", 0xFFFFFFF0), ("Y+X", M32), ("Z", M32), ("Y+X", 0xFFFFFFF0)]
        for wv, (coord, word) in enumerate(specs):
            P[64 * wv + (wv * 23 + 9) % 64] = _with_top_word(rng, oracle, coord, word)
    if name == "edge":
        # one lane per Z = 1 wave on the base (0, 1, 1, 0): its state stays (0, Y, Z, 0) with small Y, so
        # after the gated warm-up steps Y - X has word 1 = 0, fe25519_sub's rare edge, in the deferred pass's
        # first steps: the pass is dropped and the wave reruns gated
        for wv in (0, 1):
            lane = 64 * wv + 21 + wv
            P[lane] = 0
            P[lane, 4] = P[lane, 8] = 1
            assert int(s[lane, 3]) >> 40     # a long chain: the deferred pass is reached
    return s, P


@pytest.mark.parametrize("name", CASES)
def test_voted_step_gives_the_oracles_bits(bp, oracle, name):
    s, P = _block(name, oracle)
    want = _sm_oracle(oracle, s, P)
    got = _probe(bp, 0, s, P)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0]
    if name in ("force", "63+1", "short"):   # the recovery pass (the gated loop, voted too) on the same waves
        forced = _probe(bp, 1, s, P)
        assert np.array_equal(forced, want), np.nonzero((forced != want).any(axis=1))[0]


def _pipeline(bp, n, B, arrays, G, H, g, h, bits):
    import torch
    dev = torch.device("cuda:0")
    pipe = bp.VerifyPipeline(B, n, _T(G), _T(H), _T(h))
    if bits:
        pipe.prefix_tables(bits)
    batch = bp.RangeProofBatch.from_numpy(n, arrays, dev)
    ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    P, chk = (torch.zeros(B, 16, dtype=torch.int64, device=dev) for _ in range(2))
    pipe.push(batch, ok, P, chk)
    pipe.flush()
    torch.cuda.synchronize()
    pipe.close()
    u = lambda t: t.cpu().numpy().view(np.uint64)
    return ok.cpu().numpy().astype(bool), u(P), u(chk)


@pytest.mark.parametrize("bits", [0, 4])
def test_small_pipeline_n16_against_the_reference(bp, golden, monkeypatch, bits):
    """B = 4 of the reference's n = 16 proofs through k_terms<1>: verdicts, P and check points as the
    reference emitted them."""
    from test_gpu_parity import _batch_from_golden
    monkeypatch.setenv("HIPBP_QUAD", "0")
    d = golden("proofs_n16")
    B = 4
    arrays = {k: np.ascontiguousarray(v[:B]) for k, v in _batch_from_golden(bp, d, None).items()}
    ok, P, chk = _pipeline(bp, 16, B, arrays, d["G"], d["H"], d["g"], d["h"], bits)
    assert np.array_equal(ok, d["ok_cuda"][:B].astype(bool))
    assert np.array_equal(P, d["P"][:B])
    assert np.array_equal(chk, d["check"][:B])


@pytest.mark.parametrize("bits", [0, 4])
def test_small_pipeline_n8_against_the_oracle(bp, oracle, monkeypatch, bits):
    """B = 4 synthetic n = 8 proofs (tests/golden holds no reference proof of that size) through
    k_terms<1> against the CPU restatement's verdicts, P and check points."""
    from cudabulletproof_amd import synth
    monkeypatch.setenv("HIPBP_QUAD", "0")
    n, B = 8, 4
    G, H = oracle.base_points(n, 1), oracle.base_points(n, 2)
    g, h = oracle.gh()
    arrays = synth.proofs(B, n, seed=141)
    ok, P, chk = _pipeline(bp, n, B, arrays, G, H, g, h, bits)
    for p in range(B):
        head = np.concatenate([arrays[k][p] for k in ("V", "A", "S", "T1", "T2")] +
                              [np.zeros(8, np.uint64), arrays["t"][p], arrays["c"][p], arrays["x"][p]])
        okr, Pr, chkr, _, _ = oracle.cuda_range_proof_verify(head, arrays["V"][p], n, arrays["a"][p], arrays["b"][p],
                                                             arrays["L"][p], arrays["R"][p], G, H, g, h)
        assert ok[p] == okr and np.array_equal(P[p], Pr) and np.array_equal(chk[p], chkr), p

"""Sequences on one verify pipeline (hipbp_pipeline_*; tests/pipeline_seq.py): batches with fewer
fold rounds than log2 n, batches of different B, L_len, ab_len and split setting sharing ticks,
slots that grow and shrink, drain ticks and idle reuse, two pipelines at once, the cached one-shot
pipeline, the host-struct path and the refused push.  Every batch is read after exactly the
planner's retire tick (retire_tick, pinned on the CPU by tests/test_tick_plan.py) into guarded,
sentinel-filled outputs and compared with the CPU oracle, proof by proof, and with the one-shot
call of the same inputs on another stream.  Bit-exact: integer arithmetic.
"""
import numpy as np
import pytest

import pipeline_seq as ps

pytestmark = pytest.mark.gpu


def _streams(k=2):
    import torch
    return [torch.cuda.Stream() for _ in range(k)]


def _run(bp, oracle, n, mode, ops, clobber=False, full=True, oneshot=True):
    """ops on a fresh pipeline, then a flush; guards, oracle and one-shot checks.  Returns the records."""
    st, other = _streams()
    r = ps.Runner(bp, oracle, n, mode, st, clobber=clobber)
    try:
        r.run(list(ops) + [("flush",)])
        r.check_guards()
        assert r.check_oracle(full=full) > 0
        if oneshot:
            r.check_oneshot(other)
    finally:
        r.flight.clear()
        r.close()
        bp.release_stream_workspaces(other)
    return r.done


SHORT = [(4, 1, 3), (4, 1, 70), (16, 0, 3), (16, 0, 70), (16, 2, 3), (16, 2, 70), (64, 3, 3), (64, 5, 3),
         (256, 2, 3),    # above the lane-tree limit: the block-tree path
         (1024, 9, 2)]


@pytest.mark.parametrize("mode", [1, 0, 2])
@pytest.mark.parametrize("n,L_len,B", SHORT)
def test_uniform_short_rounds(bp, oracle, n, L_len, B, mode):
    """L_len < log2 n: final_terms_job's G[0] / H[0] of the unfolded generators, u / uinv by L_len."""
    _run(bp, oracle, n, mode, [("push", B, L_len, 1 + (B + L_len) % 3, 100 * n + L_len)])


MIX_L = [4, 3, 2, 1, 0] + [0, 1, 2, 3, 4] + [4, 0, 3, 1, 2]   # the first five all finish in one tick
MIX_B = [3, 9, 64, 5, 7, 4, 70, 6, 8, 3, 9, 5, 4, 7, 6]
MIX = [("push", B, L, 1 + k % 3, 4000 + k) for k, (B, L) in enumerate(zip(MIX_B, MIX_L))]


@pytest.fixture(scope="module")
def mix_mode1(bp, oracle):
    return _run(bp, oracle, 16, 1, MIX, clobber=True)


def test_mixed_rounds_mode1(mix_mode1):
    """15 pushes at n = 16 with L_len 4 .. 0 (one retire tick for all five), 0 .. 4, then alternating;
    ab_len 1 .. 3; B 3 .. 9, one batch of 64 and one of 70 (the lane sort); inputs overwritten after each push."""
    assert len(mix_mode1) == len(MIX)


@pytest.mark.parametrize("quad", ["0", "1", "2", "3"])
def test_mixed_rounds_forced_tick_forms_same_bits(bp, oracle, monkeypatch, mix_mode1, quad):
    """The same mix with every tick forced to one form (HIPBP_QUAD): the bits of the run by size."""
    monkeypatch.setenv("HIPBP_QUAD", quad)
    st, = _streams(1)
    r = ps.Runner(bp, oracle, 16, 1, st, clobber=True)
    try:
        got = r.run(MIX + [("flush",)])
        r.check_guards()
        key = lambda x: x.seed
        ps.same_bits(sorted(got, key=key), sorted(mix_mode1, key=key))
    finally:
        r.flight.clear()
        r.close()


@pytest.mark.parametrize("mode", [0, 2])
def test_mixed_rounds_other_modes(bp, oracle, mode):
    """The mix in inner-product mode (P_in overwritten right after its push) and in range_proof_verify
    mode (flags and polynomial sides too)."""
    _run(bp, oracle, 16, mode, MIX, clobber=True)


@pytest.mark.parametrize("n,mode,K", [(16, 1, 0), (16, 1, 5), (16, 2, 0), (16, 2, 5), (64, 1, 0), (64, 1, 5),
                                      (64, 2, 0), (64, 2, 5)])
def test_mixed_split_and_unsplit_stage0(bp, oracle, n, mode, K):
    """defer_msm toggled between pushes with L_len mixed (L_len < 2 never splits): split and unsplit
    batches, RK_MSMT chunks of different spans, share ticks; with and without prefix tables."""
    ln = n.bit_length() - 1
    Ls = [ln, 2, ln - 1, 1, ln, 3 % (ln + 1), 0, ln, 2, ln - 1]
    on = [1, 0, 0, 1, 1, 0, 1, 1, 0, 1]
    ops = [("tables", K)] if K else []
    for k, (L, d) in enumerate(zip(Ls, on)):
        ops += [("defer", bool(d)), ("push", 3 if n == 64 else 3 + k % 7, L, 1 + k % 2, 5000 + n + k)]
    _run(bp, oracle, n, mode, ops)


def test_slot_reuse_growing_and_shrinking(bp, oracle):
    """n = 4 (depth 5), 16 pushes, B cycling 3, 130, 1, 64, 65, 2, 257, 5: every slot's workspaces grow
    and shrink while its neighbours are in flight; no row past B is written."""
    Bs = [3, 130, 1, 64, 65, 2, 257, 5]
    ops = [("push", Bs[k % 8], (2, 1, 2, 0)[k % 4], 1 + k % 3, 6000 + k) for k in range(16)]
    _run(bp, oracle, 4, 1, ops)


def test_drain_ticks_and_idle_reuse(bp, oracle):
    push = lambda k, L: ("push", 4, L, 1 + k % 2, 7000 + k)
    ops = [push(0, 4), ("tick",), push(1, 2), ("tick",), ("tick",), push(2, 3), ("tick",), push(3, 0)]
    ops += [("tick",)] * 7                                   # to idle by drain ticks alone
    ops += [("flush",), ("flush",)]                          # flush on the idle pipeline, twice
    ops += [("tables", 5)] + [push(4 + k, (4, 1, 3, 4, 0)[k]) for k in range(5)] + [("flush",)]
    ops += [("tables", 0), ("gens", 4)] + [push(9 + k, (2, 4, 4, 1, 3)[k]) for k in range(5)]
    _run(bp, oracle, 16, 1, ops)


def test_two_pipelines_interleaved(bp, oracle):
    """n = 16 mode 1 and n = 4 mode 2 on two streams, driven alternately from one thread."""
    sa, sb, other = _streams(3)
    ra, rb = ps.Runner(bp, oracle, 16, 1, sa), ps.Runner(bp, oracle, 4, 2, sb)
    try:
        opa = [("push", 3 + k % 5, (4, 1, 3, 0, 2)[k % 5], 1 + k % 3, 8000 + k) for k in range(10)]
        opb = [("push", 2 + k % 7, (2, 0, 1)[k % 3], 1 + k % 2, 8100 + k) for k in range(10)]
        opa[4:4], opb[7:7] = [("tick",)], [("tick",), ("tick",)]
        for k in range(max(len(opa), len(opb))):
            for r, ops in ((ra, opa), (rb, opb)):
                if k < len(ops):
                    r.step(ops[k])
        for r in (ra, rb):
            r.step(("flush",))
            r.check_guards()
            assert r.check_oracle() > 0
            r.check_oneshot(other)
    finally:
        for r in (ra, rb):
            r.flight.clear()
            r.close()
        bp.release_stream_workspaces(other)


def test_one_shot_calls_regrow_the_cached_pipeline(bp, oracle):
    """(B, L_len) = (5, 4), (70, 1), (5, 4), (3, 0) through batch_range_proof_verify on one stream with
    no sync between the calls: the stream's cached pipeline regrows its workspaces in between."""
    import torch
    st, = _streams(1)
    r = ps.Runner(bp, oracle, 16, 1, st)
    try:
        with torch.cuda.stream(st):
            for k, (B, L_len) in enumerate([(5, 4), (70, 1), (5, 4), (3, 0)]):
                rec = ps.Rec(B, L_len, 1, 9000 + k, ps.make_arrays(16, B, L_len, 1, 9000 + k, 1), None)
                rec.out = r.outputs(B)
                rec.keep = bp.RangeProofBatch.from_numpy(16, rec.arrays, r.dev)
                bp.batch_range_proof_verify(rec.keep, r.dG, r.dH, r.dg, r.dh, rec.out["ok"], rec.out["P"],
                                            rec.out["chk"], stream=st)
                r.flight.append(rec)
            r._retire(list(r.flight))
        r.check_guards()
        assert r.check_oracle() == 83
    finally:
        r.flight.clear()
        r.close()


def test_host_structs_with_short_rounds(bp, oracle):
    """batch_range_proof_verify_host over 40 proofs at n = 16, two of them with L_len = 3."""
    from test_gpu_parity import _synth_proof_dicts
    n = 16
    s = ps.make_arrays(n, 40, 4, 1, 9100, 1)
    proofs = _synth_proof_dicts(s, n)
    for i in (7, 31):
        proofs[i]["L"], proofs[i]["R"] = proofs[i]["L"][:3].copy(), proofs[i]["R"][:3].copy()
    G, H = oracle.base_points(n, 1), oracle.base_points(n, 2)
    g, h = oracle.gh()
    got = bp.batch_range_proof_verify_host(proofs, s["V"], n, G, H, g, h, num_gpus=1)
    for i, pr in enumerate(proofs):
        okr = oracle.cuda_range_proof_verify(pr["head"], s["V"][i], n, pr["a"], pr["b"], pr["L"], pr["R"], G, H, g, h)[0]
        assert bool(got[i]) == okr, i


@pytest.mark.parametrize("n,split", [(2048, 0), (256, 1)])
def test_refused_push_is_atomic(bp, oracle, monkeypatch, n, split):
    """Mode 2, B = 1: L_len log2 n .. 2, then full-L batches until the planner refuses one (the push
    the planner model names).  Nothing of the refused batch runs; after the model's drain ticks (one
    at n = 2048, two at n = 256) it is accepted;
    every batch equals its one-shot result, and the oracle's: at n = 2048 the retried batch, at
    n = 256 (split stage 0 under a raised lane-tree limit) every proof."""
    if split:
        monkeypatch.setenv("HIPBP_LANE_TREE_MAX", "4096")
    at, drain = ps.REFUSED_PUSH[(n, 2, split)]
    ops = ps.descending_ops(n)[:at + 1]
    ops = ([("defer", True)] if split else []) + ops[:at] + [("refused",) + ops[at][1:]] + [("tick",)] * drain + \
          [ops[at], ("flush",)]
    st, other = _streams()
    r = ps.Runner(bp, oracle, n, 2, st)
    try:
        r.run(ops)
        assert len(r.done) == at + 1
        r.check_guards()
        retried = [x for x in r.done if x.seed == ops[-2][4]]
        assert len(retried) == 1
        assert r.check_oracle(only=None if split else retried) == (at + 1 if split else 1)
        r.check_oneshot(other)
    finally:
        r.flight.clear()
        r.close()
        bp.release_stream_workspaces(other)


@pytest.mark.parametrize("seed,n,mode", [(1, 4, 2), (2, 16, 1), (3, 16, 0)])
def test_random_sequences(bp, oracle, seed, n, mode):
    rng = np.random.default_rng(seed)
    ln = n.bit_length() - 1
    ops = []
    for k in range(30):
        what = rng.integers(0, 10)
        if what < 6:
            B = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 64, 65], p=[.12, .12, .12, .12, .12, .12, .12, .12, .02, .02]))
            ops.append(("push", B, int(rng.integers(0, ln + 1)), int(rng.integers(1, 4)), 10000 * seed + k))
        elif what < 8:
            ops.append(("tick",))
        elif what == 8:
            ops.append(("flush",))
        elif mode:
            ops.append(("defer", bool(rng.integers(0, 2))))
    _run(bp, oracle, n, mode, ops)

"""TEST INFRASTRUCTURE: sequences of operations on one verify pipeline (hipbp_pipeline_*), every
batch with its own B, L_len and ab_len, checked against the CPU oracle at the exact tick the
planner retires it (tests/test_pipeline_sequences_gpu.py; the planner half in tests/test_tick_plan.py).

An op is a tuple:
  ("push", B, L_len, ab_len, seed)   one batch (("refused", ...): the same, and the push must be refused)
  ("tick",)                          a drain tick, push(NULL)
  ("flush",)
  ("defer", on)                      hipbp_pipeline_defer_msm for the batches pushed from now on
  ("tables", bits)                   hipbp_pipeline_prefix_tables (idle pipeline)
  ("gens", bits)                     hipbp_pipeline_use_gens with a set of that table width (idle pipeline)
"""
import numpy as np

GUARD = 64                       # rows after row B of every output tensor
SENT8, SENT64 = 0xA5, 0x5A5A5A5A5A5A5A5A
HEAD = ("V", "A", "S", "T1", "T2")


def retire_tick(mode, L):
    """The tick, counted from the batch's own push (tick 0), that runs its RK_FINAL region: the
    batch's outputs are complete after that many further ticks (bp_tick_plan.h batch_schedule's fin)."""
    ft = L + 1 if L else 1
    last = ft
    if mode != 0:
        last = max(last, 2)
    if mode == 2:
        last = max(last, max(ft, 3))
    return last + 1


# The descending-round sequence of the refusal tests (round counts log2 n .. 2, then full-L batches):
# the 0-based index of the push the planner refuses and the drain ticks after which it accepts that
# batch, by (n, mode, split stage 0).  Pinned against the planner's replay by tests/test_tick_plan.py.
REFUSED_PUSH = {(2048, 2, 0): (12, 1), (256, 2, 1): (8, 2)}


def descending_ops(n, B=1, fulls=4):
    ln = n.bit_length() - 1
    return [("push", B, L, 1, 3000 + L) for L in range(ln, 1, -1)] + \
           [("push", B, ln, 1, 3100 + k) for k in range(fulls)]


def rand_fe(rng, shape, top=True):
    v = rng.integers(0, 2**64, size=tuple(shape) + (4,), dtype=np.uint64)
    if not top:
        v[..., 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    return v


def make_arrays(n, B, L_len, ab_len, seed, mode):
    """synth.proofs with L / R cut to L_len, a = [t, 0, ..], b = [1, random ..], c = t; one proof with
    t = 0, one with a short x, one with c wrong (the early reject), as many as B has room for."""
    from cudabulletproof_amd import synth
    s = synth.proofs(B, n, seed=seed)
    rng = np.random.default_rng(seed + 77777)
    s["L"] = np.ascontiguousarray(s["L"][:, :L_len])
    s["R"] = np.ascontiguousarray(s["R"][:, :L_len])
    if B >= 3:
        s["t"][B // 2] = 0
        s["x"][0, 1:] = 0
    a = np.zeros((B, ab_len, 4), np.uint64)
    b = rand_fe(rng, (B, ab_len))
    a[:, 0] = s["t"]
    b[:, 0] = 0
    b[:, 0, 0] = 1
    s["a"], s["b"], s["c"] = a, b, s["t"].copy()
    if B >= 2:
        s["c"][B - 1] = rand_fe(rng, (1,))[0]
    if mode == 2:
        s["taux"] = rand_fe(rng, (B,), top=False)
        s["mu"] = rand_fe(rng, (B,), top=False)
        s["Vp"] = s["V"].copy()
    return s


def special_rows(B):
    return sorted({0, B // 2, B - 1})


class Rec:
    """One pushed batch: its inputs, its guarded outputs, and their snapshot at the retire tick."""

    def __init__(self, B, L_len, ab_len, seed, arrays, Pin):
        self.B, self.L_len, self.ab_len, self.seed, self.arrays, self.Pin = B, L_len, ab_len, seed, arrays, Pin
        self.left = None
        self.got = None


class Runner:
    def __init__(self, bp, oracle, n, mode, stream, clobber=False):
        import torch
        self.bp, self.oracle, self.n, self.mode, self.stream, self.clobber = bp, oracle, n, mode, stream, clobber
        self.dev = torch.device("cuda:0")
        self.G, self.H = oracle.base_points(n, 1), oracle.base_points(n, 2)
        self.g, self.h = oracle.gh()
        with torch.cuda.stream(stream):
            self.dG, self.dH, self.dg, self.dh = (self.T(v) for v in (self.G, self.H, self.g, self.h))
            self.pipe = bp.VerifyPipeline(1, n, self.dG, self.dH, self.dh, range_mode=mode,
                                          g=self.dg if mode == 2 else None, stream=stream)
        self.flight, self.done, self.sets = [], [], []

    def T(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(self.dev)

    def outputs(self, B, guard=GUARD):
        import torch
        i64 = lambda *sh: torch.full(sh, SENT64, dtype=torch.int64, device=self.dev)
        u8 = lambda *sh: torch.full(sh, SENT8, dtype=torch.uint8, device=self.dev)
        return dict(ok=u8(B + guard), P=i64(B + guard, 16), chk=i64(B + guard, 16), fl=u8(B + guard),
                    poly=i64(B + guard, 4, 16))

    def _call(self, push, batch, o, Pin):
        if self.mode == 0:
            push(batch, o["ok"], None, o["chk"], P_in=Pin)
        elif self.mode == 1:
            push(batch, o["ok"], o["P"], o["chk"])
        else:
            push(batch, o["ok"], o["P"], o["chk"], flags_out=o["fl"], poly_out=o["poly"])

    def _ticked(self):
        for r in self.flight:
            r.left -= 1
        due = [r for r in self.flight if r.left == 0]
        if due:
            self._retire(due)

    def _retire(self, recs):
        self.stream.synchronize()
        for r in recs:
            r.got = {k: v.cpu().numpy() for k, v in r.out.items()}
            self.flight.remove(r)
            self.done.append(r)

    def run(self, ops):
        for op in ops:
            self.step(op)
        return self.done

    def step(self, op):
        import torch
        bp = self.bp
        with torch.cuda.stream(self.stream):
            if op[0] in ("push", "refused"):
                _, B, L_len, ab_len, seed = op
                arrays = make_arrays(self.n, B, L_len, ab_len, seed, self.mode)
                Pin = self.oracle.base_points(B, 9 + seed % 5) if self.mode == 0 else None
                r = Rec(B, L_len, ab_len, seed, arrays, Pin)
                batch = bp.RangeProofBatch.from_numpy(self.n, arrays, self.dev)
                dPin = self.T(Pin) if Pin is not None else None
                r.out = self.outputs(B)
                if op[0] == "refused":
                    try:
                        self._call(self.pipe.push, batch, r.out, dPin)
                    except bp.BulletproofError as e:
                        assert "push refused" in str(e) and "drain tick" in str(e) and "retry" in str(e), str(e)
                    else:
                        raise AssertionError(f"push {op} was not refused")
                    self.stream.synchronize()   # nothing ran: the refused batch's outputs are untouched
                    for k, v in r.out.items():
                        assert bool((v == (SENT8 if v.dtype == torch.uint8 else SENT64)).all()), k
                    return
                self._call(self.pipe.push, batch, r.out, dPin)
                if dPin is not None:
                    dPin.fill_(0x5A5A)   # consumed by its own push
                if self.clobber:
                    for k in bp.RangeProofBatch.FIELDS + bp.RangeProofBatch.OPTIONAL:
                        if getattr(batch, k) is not None:
                            getattr(batch, k).fill_(0x5A5A)
                r.keep = (batch, dPin)
                self._ticked()
                r.left = retire_tick(self.mode, L_len)
                self.flight.append(r)
            elif op[0] == "tick":
                self.pipe.push(None)
                self._ticked()
            elif op[0] == "flush":
                self.pipe.flush()
                self._retire(list(self.flight))
            elif op[0] == "defer":
                self.pipe.defer_msm(op[1])
            elif op[0] == "tables":
                assert not self.flight
                self.pipe.prefix_tables(op[1])
            elif op[0] == "gens":
                assert not self.flight
                gs = bp.Generators(self.n, self.dG, self.dH, self.dg, self.dh, prefix_bits=op[1])
                self.sets.append(gs)
                self.pipe.use_gens(gs)
            else:
                raise ValueError(op)

    def close(self):
        assert not self.flight, "batches left in flight"
        self.pipe.close()
        for gs in self.sets:
            gs.close()
        self.bp.release_stream_workspaces(self.stream)

    # ------------------------------------------------------------------ checks
    def check_guards(self):
        for r in self.done:
            for k, v in r.got.items():
                used = k in ("ok", "chk") or (k == "P" and self.mode) or (k in ("fl", "poly") and self.mode == 2)
                tail = v[r.B:] if used else v
                sent = SENT8 if v.dtype == np.uint8 else SENT64
                assert (tail == sent).all(), (r.seed, r.B, k, "write past row B")

    def check_oracle(self, full=True, only=None):
        """Rows of every batch (`only`: of those records) against the oracle at the snapshot taken at
        the retire tick: every proof, or the first, the last and the three special proofs."""
        from test_gpu_parity import _check_std_vs_oracle
        O, n = self.oracle, self.n
        u = lambda a: np.ascontiguousarray(a).view(np.uint64)
        count = 0
        for r in (self.done if only is None else only):
            s, got = r.arrays, r.got
            rows = list(range(r.B)) if full else special_rows(r.B)
            ok, chk = got["ok"][:r.B].astype(bool), u(got["chk"][:r.B])
            assert ((got["ok"][:r.B] == 0) | (got["ok"][:r.B] == 1)).all(), (r.seed, "ok not written")
            count += len(rows)
            if self.mode == 2:
                sub = {k: v[rows] for k, v in s.items()}
                heads = np.concatenate([sub[k] for k in ("Vp", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")], axis=1)
                res = (ok[rows], u(got["P"][:r.B])[rows], chk[rows], got["fl"][:r.B][rows], u(got["poly"][:r.B])[rows])
                _check_std_vs_oracle(O, n, sub, heads, self.G, self.H, self.g, self.h, res)
                continue
            for p in rows:
                if self.mode == 0:
                    okr, chkr, _, _ = O.cuda_inner_product_verify(n, s["a"][p], s["b"][p], s["c"][p], s["L"][p], s["R"][p],
                                                                  s["x"][p], r.Pin[p], self.G, self.H, self.h)
                else:
                    head = np.concatenate([s[k][p] for k in HEAD] + [np.zeros(8, np.uint64), s["t"][p], s["c"][p], s["x"][p]])
                    okr, Pr, chkr, _, _ = O.cuda_range_proof_verify(head, s["V"][p], n, s["a"][p], s["b"][p], s["L"][p],
                                                                    s["R"][p], self.G, self.H, self.g, self.h)
                    assert np.array_equal(u(got["P"][:r.B])[p], Pr), (r.seed, r.B, r.L_len, p, "P")
                assert ok[p] == okr, (r.seed, r.B, r.L_len, p, "ok")
                if okr or not np.array_equal(chkr, np.zeros(16, np.uint64)):
                    assert np.array_equal(chk[p], chkr), (r.seed, r.B, r.L_len, p, "check")
        return count

    def oneshot(self, r, stream):
        """The batch through the one-shot call of the pipeline's mode on `stream`: the outputs' rows."""
        import torch
        bp = self.bp
        with torch.cuda.stream(stream):
            batch = bp.RangeProofBatch.from_numpy(self.n, r.arrays, self.dev)
            o = self.outputs(r.B, 0)
            G, H, g, h = self.T(self.G), self.T(self.H), self.T(self.g), self.T(self.h)
            if self.mode == 0:
                bp.batch_inner_product_verify(batch, self.T(r.Pin), G, H, h, o["ok"], o["chk"], stream=stream)
            elif self.mode == 1:
                bp.batch_range_proof_verify(batch, G, H, g, h, o["ok"], o["P"], o["chk"], stream=stream)
            else:
                bp.batch_range_proof_verify_std(batch, G, H, g, h, o["ok"], o["P"], o["chk"], o["fl"], o["poly"],
                                                stream=stream)
            stream.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def check_oneshot(self, stream):
        for r in self.done:
            one = self.oneshot(r, stream)
            for k, v in one.items():
                assert np.array_equal(v, r.got[k][:r.B]), (r.seed, r.B, r.L_len, k, "differs from the one-shot call")


def same_bits(recs_a, recs_b):
    assert len(recs_a) == len(recs_b)
    for x, y in zip(recs_a, recs_b):
        for k in x.got:
            assert np.array_equal(x.got[k], y.got[k]), (x.seed, x.B, x.L_len, k)

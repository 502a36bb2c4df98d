"""Throughput of the batched GPU inner_product_prove at n = 4096 (tools/, not a test; bench.py is
the flagship benchmark and does not run this).

  python tools/bench_ipa_prove.py --cpu                     CPU leg only: the reference's prover, one proof
  python tools/bench_ipa_prove.py [--B 256,16] [--bits 0,8] [--out FILE.json]

Shape: n = 4096 on the reference's generators (base points {1}, {2}, Q = h), B proofs per call, the
plain form (prefix bits 0) and a generator set with prefix tables.  Per configuration: one warm-up
call, then the median of 5 calls timed with HIP events on the calling stream.  The proofs are checked
outside the timed region: proofs 0 and 1 are the fixture's two n = 4096 instances and must equal it
bit for bit; all of them go through P = msm_batch(a || b, G || H) and batch_inner_product_verify with
c_final.  The reference's verifier does not accept every honest proof (its accept rule and its
non-associative arithmetic): the verdicts of proofs 0..15 must equal the reference's
recorded ones (the fixture's and tests/golden/ipa_prove_bench_verdicts.json); for the rest the
accepted count is reported.

Roof: a proof is 4(n - 1) + 2 log2 n = 16,404 scalar multiplications on fixed bases.  The same run
measures the canonical MSM's scalar-mult rate (msm_batch / msm_batch_gens over G || H, random 255-bit
scalars, the per-point terms dominate) and prints rate / 16,404 as the scalar-mult-bound ceiling and
the achieved fraction of it.  The prover's scalars are as heavy as the MSM's, so the ceiling is fair;
it leaves out the order-bound chains (4(n - 1) dependent add + normalize steps per proof on one lane
each), which the two-workspace schedule is meant to hide at large B and cannot hide at small B.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

N = 4096
SM_PER_PROOF = 4 * (N - 1) + 2 * 12


def cpu_leg():
    """The reference's inner_product_prove on one core: seconds per proof (None without the reference build)."""
    from make_ipa_prove import case_inputs, generators
    from oracle import pyoracle as po
    if not po.have_reference():
        return None
    R = po.Reference()
    a, b, tr, _ = case_inputs(23, N, 0)
    G, H, Q = generators(R, N)
    c = po.fe()
    R.f("inner_product")(po._p(c), po._p(a), po._p(b), po._sz(N))
    t0 = time.perf_counter()
    R.ipa_prove(a, b, G, H, Q, c, tr)
    return time.perf_counter() - t0


def timed(torch, fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="CPU leg only")
    ap.add_argument("--B", default="256,16")
    ap.add_argument("--bits", default="0,8")
    ap.add_argument("--cores", type=int, default=16, help="CPU cores the reference's prover is credited with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"n": N, "sm_per_proof": SM_PER_PROOF}
    cpu_s = cpu_leg()
    res["cpu_ref_s_per_proof"] = cpu_s
    res["cpu_ref_proofs_per_s_all_cores"] = args.cores / cpu_s if cpu_s else None
    print(json.dumps({k: res[k] for k in ("cpu_ref_s_per_proof", "cpu_ref_proofs_per_s_all_cores")}), flush=True)
    if args.cpu:
        return

    import torch

    import cudabulletproof_amd as bp
    from make_ipa_prove import case_inputs, generators
    from oracle import pyoracle as po
    bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    O = po.Oracle()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    Gn, Hn, Qn = generators(O, N)
    G, H, Q, g = T(Gn), T(Hn), T(Qn), T(O.gh()[0])
    GH = torch.cat([G, H]).contiguous()
    fix = dict(np.load(os.path.join(ROOT, "tests", "golden", "ipa_prove.npz")))
    Bs = [int(x) for x in args.B.split(",")]
    Bmax = max(Bs)
    cases = [23, 24] + [1000 + k for k in range(Bmax - 2)]
    with open(os.path.join(ROOT, "tests", "golden", "ipa_prove_bench_verdicts.json")) as f:
        rec = json.load(f)
    assert rec["cases"] == cases[2:2 + len(rec["cases"])]
    want_ok = np.array(fix["ok_final"][23:25].tolist() + rec["ok_final"], bool)
    ins = [case_inputs(k, N, 0) for k in cases[:Bmax]]
    a_all, b_all = np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins])
    c_all = np.stack([O.inner_product(i[0], i[1]) for i in ins])
    assert np.array_equal(c_all[:2], fix["c_in"][23:25])
    res["runs"] = []
    for bits in [int(x) for x in args.bits.split(",")]:
        gens = bp.Generators(N, G, H, g, Q, prefix_bits=bits) if bits else None
        # roof: the canonical MSM's scalar-mult rate over the same bases (32 MSMs of 2n points)
        M = 32
        sc = T(np.concatenate([a_all[:M], b_all[:M]], axis=1))
        Pm = torch.zeros(M, 16, dtype=torch.int64, device=dev)
        msm = (lambda: bp.msm_batch_gens(Pm, sc, gens)) if gens else (lambda: bp.msm_batch(Pm, sc, GH))
        msm_ms, _, _ = timed(torch, msm)
        sm_rate = M * 2 * N / (msm_ms * 1e-3)
        for B in Bs:
            a, b, c = T(a_all[:B]), T(b_all[:B]), T(c_all[:B])
            ms, all_ms, out = timed(torch, lambda: bp.batch_inner_product_prove(N, a, b, c, G, H, Q, gens=gens))
            torch.cuda.synchronize()
            # checks, outside the timed region
            lo = fix["L_off"]
            k = min(B, 2)
            same = all(np.array_equal(out[key][:k].cpu().numpy().view(np.uint64).reshape(k, -1),
                                      np.stack([fix[src][23 + p] if src not in ("L", "R") else
                                                fix[src][lo[23 + p]:lo[24 + p]].reshape(-1) for p in range(k)]).reshape(k, -1))
                       for key, src in (("a", "a"), ("b", "b"), ("c", "c_in"), ("x", "x"), ("c_final", "c_final"),
                                        ("L", "L"), ("R", "R")))
            P = torch.zeros(B, 16, dtype=torch.int64, device=dev)
            bp.msm_batch(P, torch.cat([a, b], dim=1).contiguous(), GH)
            ok = torch.zeros(B, dtype=torch.uint8, device=dev)
            bp.batch_inner_product_verify(bp.ipa_proof_batch(N, out, c="c_final"), P, G, H, Q, ok)
            torch.cuda.synchronize()
            okh = ok.cpu().numpy().astype(bool)
            k = min(B, len(want_ok))
            verdicts = bool(np.array_equal(okh[:k], want_ok[:k]))
            rate = B / (ms * 1e-3)
            ceiling = sm_rate / SM_PER_PROOF
            run = dict(B=B, prefix_bits=bits, ms_median=ms, ms_all=all_ms, proofs_per_s=rate,
                       msm_sm_per_s=sm_rate, ceiling_proofs_per_s=ceiling, fraction_of_ceiling=rate / ceiling,
                       fixture_bits_equal=bool(same), verdicts_equal_reference=verdicts,
                       verdicts_checked=k, roundtrip_accepted=int(okh.sum()),
                       speedup_vs_cpu_all_cores=rate / res["cpu_ref_proofs_per_s_all_cores"]
                       if res["cpu_ref_proofs_per_s_all_cores"] else None)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        if gens:
            gens.close()
    res["ok"] = all(r["fixture_bits_equal"] and r["verdicts_equal_reference"] for r in res["runs"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"ok": res["ok"]}))
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

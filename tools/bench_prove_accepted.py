"""What an accepted batch costs beside the seeded prover followed by a verify (tools/, not a test;
bench.py is the flagship benchmark and does not run this).

  python tools/bench_prove_accepted.py [--B 65536] [--n 64] [--reps 5] [--prefix-bits 8] [--out FILE.json]

Shape: B proofs of n bits per call with a generator set (tools/bench_prove_seeded.py's generators,
values and blindings).  Three legs, each one warm-up call, then `reps` calls timed with a host clock
around the call and a device synchronise, taken in turn (a, b, b1, a, b, b1, ...) in one session:

  (a)  batch_generate_range_proof_seeded(gens) followed by batch_range_proof_verify_gens on its
       output: the existing paths, the yardstick;
  (b)  batch_generate_range_proof_accepted(gens, max_attempts = 8, check = 1);
  (b1) the same with max_attempts = 1: round 1 alone, so (b) - (b1) is what rounds >= 2 cost.

Then, outside the timed region: the proofs proved per round (accepted_last_stats), the three new
kernels' HIP-event times over one call with HIPBP_ACCEPT_TIMING=1, and a verify of (b)'s output,
which must accept exactly the proofs with attempts > 0.

Expectation, stated beside the measurement and no pass mark: (b) ~ (a) x (1 + the retried share)
plus the latency-bound small rounds; the new kernels a fraction of a per cent of (b).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_prove_seeded import generators  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prefix-bits", type=int, default=8)
    ap.add_argument("--max-attempts", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n = args.B, args.n

    import torch
    sys.path.insert(0, ROOT)
    import cudabulletproof_amd as bp
    bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    G, H, g, h = (T(x) for x in generators(n))
    gens = bp.Generators(n, G, H, g, h, prefix_bits=args.prefix_bits)
    rng = np.random.default_rng(1)
    v = np.zeros((B, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << min(n, 62), B, dtype=np.uint64)
    gam = rng.integers(0, 1 << 62, (B, 4), dtype=np.uint64)
    vd, gd = T(v), T(gam)
    seed = bytes(range(32))
    ok = torch.zeros(B, dtype=torch.uint8, device=dev)

    def verify(o):
        bp.batch_range_proof_verify_gens(bp.RangeProofBatch(n, **{k: o[k] for k in bp.RangeProofBatch.FIELDS}), gens, ok)

    def leg_a():
        o = bp.batch_generate_range_proof_seeded(n, vd, gd, seed, G, H, g, h, gens=gens)
        verify(o)
        return o

    accepted = lambda k: bp.batch_generate_range_proof_accepted(n, vd, gd, seed, G, H, g, h, max_attempts=k, gens=gens)
    legs = dict(a=leg_a, b=lambda: accepted(args.max_attempts), b1=lambda: accepted(1))
    ms = {k: [] for k in legs}
    out = {}
    for k, fn in legs.items():   # warm-up
        fn()
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            out[k] = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(x) for k, x in ms.items()}
    res = dict(B=B, n=n, reps=args.reps, prefix_bits=args.prefix_bits, max_attempts=args.max_attempts)
    for k in legs:
        res[f"{k}_ms_median"], res[f"{k}_ms_all"] = med[k], ms[k]
    res.update(b_over_a=med["b"] / med["a"], b1_over_a=med["b1"] / med["a"],
               rounds_ge2_ms=med["b"] - med["b1"], rounds_ge2_share_of_b=(med["b"] - med["b1"]) / med["b"])

    # one more call with the loop's kernels between HIP events; the per-round sizes
    os.environ["HIPBP_ACCEPT_TIMING"] = "1"
    ob = accepted(args.max_attempts)
    os.environ.pop("HIPBP_ACCEPT_TIMING")
    st = bp.accepted_last_stats()
    att = ob["attempts"].cpu().numpy()
    valid = ob["valid"].cpu().numpy()
    kms = st["kernel_ms"]
    res.update(rounds=st["rounds"], proved_per_round=st["proved"], retried_share=sum(st["proved"][1:]) / B,
               attempts_histogram=np.bincount(att, minlength=2).tolist(), valid=int(valid.sum()),
               kernel_ms=kms, kernel_ms_total=sum(kms.values()), kernel_share_of_b=sum(kms.values()) / med["b"],
               expected_b_ms=med["a"] * (1 + sum(st["proved"][1:]) / B))
    res["b_accepted_proofs_per_s"] = int((att > 0).sum()) / (med["b"] * 1e-3)
    # the result verifies: ok exactly where attempts > 0 (no refused value in this batch), and the
    # timed call gave the same bits
    verify(ob)
    torch.cuda.synchronize()
    res["verify_agrees"] = bool(np.array_equal(ok.cpu().numpy() != 0, att > 0)) and int(valid.sum()) == B
    res["same_bits"] = all(bool(torch.equal(ob[k], out["b"][k])) for k in ob if k != "_keep")
    res["ok"] = res["verify_agrees"] and res["same_bits"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

"""What feeding the batched prover costs, and what the seeded prover saves (tools/, not a test;
bench.py is the flagship benchmark and does not run this).

  python tools/bench_prove_seeded.py [--B 65536] [--n 64] [--reps 5] [--out FILE.json]
  python tools/bench_prove_seeded.py --only-a [--root OTHER_CHECKOUT] --out A.json
  python tools/bench_prove_seeded.py --parent-a A1.json,A2.json --out FILE.json

Shape: B proofs of n bits per call on the golden generators (tests/golden/proofs_n{n}.npz; other n:
the reference's base points {1}, {2}).  Three ways to one batch of proofs, each one warm-up call
then `reps` calls timed with a host clock around the call and a device synchronise:

  (a) batch_generate_range_proof with its 2n + 4 scalars per proof already resident on the device
      (what bench.py and the tests do; numpy scalars with generate_random_scalar's masks, so this
      leg runs unchanged on a checkout from before the seeded prover: --only-a --root);
  (b) batch_generate_range_proof_seeded: v, gamma resident, the scalars derived on the GPU;
  (c) batch_generate_range_proof fed as a caller without (b) must: the scalars drawn on the host
      (os.urandom + the masks in numpy, `--threads` threads, into pinned memory), one H2D copy, the call.

Also the derive kernels alone (derive_prover_scalars between HIP events).  Outside the timed region
(b)'s proofs are compared with the explicit prover's on the derived scalars, every tensor.

--parent-a: (a) results of --only-a runs on the parent checkout, taken in the same session and
alternated with this one; their individual call times give the parent's own run-to-run spread, and
a_within_parent_spread says whether this checkout's (a) median lies inside it.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R", "valid")


def generators(n):
    f = os.path.join(ROOT, "tests", "golden", f"proofs_n{n}.npz")
    if os.path.exists(f):
        d = np.load(f)
        return d["G"], d["H"], d["g"], d["h"]
    sys.path.insert(0, ROOT)
    from oracle import pyoracle as po
    O = po.Oracle()
    g, h = O.gh()
    return O.base_points(n, 1), O.base_points(n, 2), g, h


def mask(flat_u8):
    """generate_random_scalar's masks (rp.cu:153-159) on (..., 32) bytes, in place."""
    s = flat_u8.reshape(-1, 32)
    s[:, 0] &= 0xF8
    s[:, 31] &= 0x7F
    s[:, 31] |= 0x40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of leg (c)")
    ap.add_argument("--root", default=ROOT, help="import cudabulletproof_amd from this checkout (built there)")
    ap.add_argument("--only-a", action="store_true", help="leg (a) alone (any checkout with the batched prover)")
    ap.add_argument("--parent-a", default=None, help="comma list of --only-a results from the parent checkout")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n = args.B, args.n

    import torch
    sys.path.insert(0, os.path.abspath(args.root))
    import cudabulletproof_amd as bp
    bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    G, H, g, h = (T(x) for x in generators(n))
    rng = np.random.default_rng(1)
    v = np.zeros((B, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << min(n, 62), B, dtype=np.uint64)
    gam = rng.integers(0, 1 << 62, (B, 4), dtype=np.uint64)
    vd, gd = T(v), T(gam)
    S = 2 * n + 4
    seed = bytes(range(32))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), ms, out

    res = dict(B=B, n=n, reps=args.reps, root=os.path.relpath(os.path.abspath(args.root), ROOT), scalars_per_batch=B * S,
               scalar_bytes_per_batch=B * S * 32)

    # (a) resident scalars
    sc = rng.integers(0, 1 << 63, (B * S, 4), dtype=np.uint64)
    mask(sc.view(np.uint8))
    scd = T(sc)
    rnd_a, sL_a, sR_a = scd[:4 * B].view(B, 4, 4), scd[4 * B:(4 + n) * B].view(B, n, 4), scd[(4 + n) * B:].view(B, n, 4)
    a_ms, a_all, oa = timed(lambda: bp.batch_generate_range_proof(n, vd, gd, sL_a, sR_a, rnd_a, G, H, g, h))
    res.update(a_ms_median=a_ms, a_ms_all=a_all, a_proofs_per_s=B / (a_ms * 1e-3), a_valid=int(oa["valid"].sum()))
    print(json.dumps({k: res[k] for k in ("a_ms_median", "a_ms_all", "a_proofs_per_s")}), flush=True)

    if not args.only_a:
        # (b) seeded
        b_ms, b_all, ob = timed(lambda: bp.batch_generate_range_proof_seeded(n, vd, gd, seed, G, H, g, h))
        res.update(b_ms_median=b_ms, b_ms_all=b_all, b_proofs_per_s=B / (b_ms * 1e-3))
        # the derive kernels alone, HIP events
        bp.derive_prover_scalars(n, vd, gd, seed)
        torch.cuda.synchronize()
        d_all = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            der = bp.derive_prover_scalars(n, vd, gd, seed)
            e1.record()
            e1.synchronize()
            d_all.append(e0.elapsed_time(e1))
        d_ms = statistics.median(d_all)
        res.update(derive_ms_median=d_ms, derive_ms_all=d_all, derive_scalars_per_s=B * S / (d_ms * 1e-3),
                   derive_fraction_of_b=d_ms / b_ms)
        # (b) against the explicit prover on the derived scalars, outside the timed region
        oe = bp.batch_generate_range_proof(n, vd, gd, der["sL"], der["sR"], der["rnd"], G, H, g, h)
        torch.cuda.synchronize()
        res["b_equals_explicit"] = all(bool(torch.equal(ob[k], oe[k])) for k in KEYS)

        # (c) host-generated scalars: urandom + masks in `threads` threads into pinned memory, H2D, call
        pin = torch.empty(B * S, 4, dtype=torch.int64).pin_memory()
        pin8 = pin.numpy().view(np.uint8).reshape(-1)
        dst = torch.empty(B * S, 4, dtype=torch.int64, device=dev)
        nb = B * S * 32
        cuts = [nb * k // args.threads // 32 * 32 for k in range(args.threads + 1)]
        pool = ThreadPoolExecutor(args.threads)

        def fill(k):
            lo, hi = cuts[k], cuts[k + 1]
            pin8[lo:hi] = np.frombuffer(os.urandom(hi - lo), np.uint8)
            mask(pin8[lo:hi])

        def leg_c():
            list(pool.map(fill, range(args.threads)))
            dst.copy_(pin, non_blocking=True)
            return bp.batch_generate_range_proof(n, vd, gd, dst[4 * B:(4 + n) * B].view(B, n, 4),
                                                 dst[(4 + n) * B:].view(B, n, 4), dst[:4 * B].view(B, 4, 4), G, H, g, h)
        c_ms, c_all, _ = timed(leg_c)
        t0 = time.perf_counter()
        list(pool.map(fill, range(args.threads)))
        res.update(c_ms_median=c_ms, c_ms_all=c_all, c_proofs_per_s=B / (c_ms * 1e-3),
                   c_host_generation_ms=(time.perf_counter() - t0) * 1e3, c_threads=args.threads)
        pool.shutdown()

    if args.parent_a:
        runs = [json.load(open(f)) for f in args.parent_a.split(",")]
        allp = [x for r in runs for x in r["a_ms_all"]]
        res.update(parent_a_ms_medians=[r["a_ms_median"] for r in runs], parent_a_ms_all=allp,
                   parent_a_spread_ms=[min(allp), max(allp)],
                   a_within_parent_spread=bool(min(allp) <= res["a_ms_median"] <= max(allp)))
    res["ok"] = bool(res.get("b_equals_explicit", True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

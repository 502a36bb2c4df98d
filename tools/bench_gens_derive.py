"""What deriving generators from seeds costs, against what a caller did before (tools/, not
a test; bench.py is the flagship benchmark and does not run this).  One session on one GPU.

  python tools/bench_gens_derive.py [--reps 5] [--out profiles/bench/gens_derive_p01.json]

The legs are alternated in one session, `reps` rounds after a warm-up round; medians and min-max:
  derive_131072, derive_2p20   hipbp_derive_base_points into a device buffer (HIP events around the
                               call), with the GB/s of its 128-byte stores
  today_131072, today_2p20     the same points the earlier way: synth.base_points_xy (hashlib) and
                               synth.fill_T (upload X and Y, field_op("mul"), download); wall clock
  seeded_64, seeded_65536      Generators.from_seeds(n), no tables; wall clock (the call is synchronous)
  upload_64, upload_65536      hipbp_derive_base_points_host for G, H, g, h, upload, Generators(...); wall clock
  host_2p20                    hipbp_derive_base_points_host for 2^20 points, one thread; wall clock
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = args.reps

    import torch

    import cudabulletproof_amd as bp
    from cudabulletproof_amd import synth
    bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    sizes = {"131072": 131072, "2p20": 1 << 20}
    bufs = {k: torch.zeros(c, 16, dtype=torch.int64, device=dev) for k, c in sizes.items()}
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    keep = {}

    def event_ms(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep["last"] = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def today(k):
        keep["today_" + k] = synth.fill_T(synth.base_points_xy(sizes[k], 5), dev)

    def seeded(n):
        bp.Generators.from_seeds(n).close()

    def upload(n):
        G, H = bp.derive_base_points_host(1, n), bp.derive_base_points_host(2, n)
        g, h = bp.derive_single_point_host(3), bp.derive_single_point_host(4)
        bp.Generators(n, T(G), T(H), T(g), T(h)).close()

    def host(k):
        keep["host_" + k] = bp.derive_base_points_host(5, sizes[k])

    legs = {}
    for k in sizes:
        legs["derive_" + k] = lambda k=k: event_ms(lambda: bp.derive_base_points(5, sizes[k], out=bufs[k]))
        legs["today_" + k] = lambda k=k: wall_ms(lambda: today(k))
    for n in (64, 65536):
        legs[f"seeded_{n}"] = lambda n=n: wall_ms(lambda: seeded(n))
        legs[f"upload_{n}"] = lambda n=n: wall_ms(lambda: upload(n))
    legs["host_2p20"] = lambda: wall_ms(lambda: host("2p20"))
    ms = {k: [] for k in legs}
    for r in range(reps + 1):   # round 0 warms up
        for k, fn in legs.items():
            t = fn()
            if r:
                ms[k].append(t)

    def stat(x):
        return dict(ms_median=statistics.median(x), ms_all=x, ms_spread=[min(x), max(x)])
    res = dict(reps=reps, device=torch.cuda.get_device_name(0), **{k: stat(x) for k, x in ms.items()})
    for k, c in sizes.items():
        res["derive_" + k]["points"] = c
        res["derive_" + k]["store_GBps"] = c * 128 / (res["derive_" + k]["ms_median"] * 1e-3) / 1e9
    res["host_2p20"]["us_per_point"] = res["host_2p20"]["ms_median"] * 1e3 / sizes["2p20"]
    same = all(np.array_equal(bufs[k].cpu().numpy().view(np.uint64), keep["today_" + k]) for k in sizes)
    same = same and np.array_equal(keep["host_2p20"], keep["today_2p20"])
    res["ok"] = bool(same)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()

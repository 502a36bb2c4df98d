"""What the batched Pedersen commitments cost (tools/, not a test; bench.py is the flagship benchmark
and does not run this).  One session on one GPU, every rate from a host clock around calls that end
in a device synchronise, one warm-up call per shape first.

  python tools/bench_commit.py [--log2 20] [--reps 5] [--out FILE.json] [--ab-out FILE.json]

  (a) commitments/s at count = 2^log2, values uniform in [0, 2^64), blindings masked as
      generate_random_scalar masks them: the plain call, and with a K = 16 generator set (n = 1, so
      the tables are 32 MB).  Median of `reps`, with the spread.
  (b) the canonical MSM (hipbp_msm) on 2^log2 points in the same session, as the yardstick: points/s,
      and from it point operations per second, an "operation" being one ge25519_add of a scalar
      multiplication's chain (sm_ops: 256 - leading zeros doublings + popcount adds) plus the MSM
      tree's m - 1 adds.  (a) is reported as a fraction of that rate over the operations per
      commitment (both chains + the one add), counted on the actual scalars of both workloads.  The
      count leaves out the normalisations: the MSM's are the device form (no inversion), a commitment
      has three host ge25519_normalize, each a field inversion when Z != 1, so the fraction is
      expected below 1.
  (c) the prover's proofs/s at n = 64 (batch_generate_range_proof, scalars resident), the cost of
      obtaining V the only way there was before.
  (d) the chain-length sort A/B (HIPBP_COMMIT_SORT 0 / 1): `reps` alternating calls each, for the
      uniform workload and for values of log-uniform magnitude (2^8 .. 2^63), with the bytes compared;
      written to --ab-out.
  (e) the host call (batch_pedersen_commit_host, one GPU) at the same count, and the share of its
      time spent outside the device call's kernels (1 - device call time / host call time).
  (f) the smallest count at which the warm device call beats count x the CPU time of one restatement
      commitment (the C restatement's fe_tobytes, 2 ge_scalarmult, 3 ge_normalize_host, ge_add through
      ctypes, measured here): bisection between powers of two, each point the median of `reps` calls.

The multi-GPU rate of the host form is not measured here (a one-GPU session).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def masked(rng, count):
    b = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    b[:, 31] &= 0x7F
    b[:, 0] &= 0xF8
    b[:, 31] |= 0x40
    return np.ascontiguousarray(b).view("<u8").astype(np.uint64).reshape(count, 4)


def sm_ops_sum(s):
    """Sum over the (count,4) uint64 scalars of ge25519_dev.h's sm_ops: bit length + popcount."""
    total = 0
    for lo in range(0, len(s), 1 << 16):
        bits = np.unpackbits(np.ascontiguousarray(s[lo:lo + (1 << 16)]).view(np.uint8), axis=1, bitorder="little")
        anyb = bits.any(axis=1)
        length = np.where(anyb, 256 - np.argmax(bits[:, ::-1], axis=1), 0)
        total += int(length.sum()) + int(bits.sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prove-batch", type=int, default=16384)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-out", default=None)
    args = ap.parse_args()
    count, reps = 1 << args.log2, args.reps

    import torch

    import cudabulletproof_amd as bp
    import commit_ref as cr
    from oracle import pyoracle
    bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    d = np.load(os.path.join(ROOT, "tests", "golden", "proofs_n64.npz"))
    g, h = d["g"], d["h"]
    gd, hd = T(g), T(h)
    rng = np.random.default_rng(1)
    v = np.zeros((count, 4), np.uint64)
    v[:, 0] = rng.integers(0, 2**64, count, dtype=np.uint64)
    vlog = np.zeros((count, 4), np.uint64)   # log-uniform magnitudes: a uniform bit length in 9 .. 64
    nbits = rng.integers(9, 65, count)
    vlog[:, 0] = (rng.integers(0, 2**64, count, dtype=np.uint64) >> (64 - nbits).astype(np.uint64)) | \
        (np.uint64(1) << (nbits - 1).astype(np.uint64))
    gamma = masked(rng, count)
    vd, vlogd, gamd = T(v), T(vlog), T(gamma)
    out = torch.empty(count, 16, dtype=torch.int64, device=dev)

    def timed(fn, n=reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def stat(ms, items):
        med = statistics.median(ms)
        return dict(ms_median=med, ms_all=ms, ms_spread=[min(ms), max(ms)], per_s=items / (med * 1e-3))

    res = dict(count=count, reps=reps, sort_default=os.environ.get("HIPBP_COMMIT_SORT", "unset"))

    # (a) plain and K = 16 tables
    res["a_plain"] = stat(timed(lambda: bp.batch_pedersen_commit(vd, gamd, gd, hd, out=out)), count)
    plain = out.clone()
    gens = bp.Generators(1, T(d["G"][:1]), T(d["H"][:1]), gd, hd, prefix_bits=16)
    res["a_gens16"] = stat(timed(lambda: bp.batch_pedersen_commit(vd, gamd, None, None, out=out, gens=gens)), count)
    res["a_gens16"]["table_bytes"] = gens.nbytes_tables()
    res["a_gens16_equals_plain"] = bool(torch.equal(out, plain))
    gens.close()
    print(json.dumps({k: res[k] for k in ("a_plain", "a_gens16")}), flush=True)

    # (b) the canonical MSM on the commitments just made (count valid normalized points), random 255-bit scalars
    ms_scal = rng.integers(0, 2**64, (count, 4), dtype=np.uint64)
    ms_scal[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    msd, root = T(ms_scal), torch.empty(16, dtype=torch.int64, device=dev)
    res["b_msm"] = stat(timed(lambda: bp.msm(root, msd, plain)), count)
    ops_msm = sm_ops_sum(ms_scal) + count - 1
    ops_commit = sm_ops_sum(v) + sm_ops_sum(gamma) + count
    ops_per_s = ops_msm / (res["b_msm"]["ms_median"] * 1e-3)
    predicted = ops_per_s / (ops_commit / count)
    res["b_model"] = dict(msm_point_ops=ops_msm, commit_point_ops=ops_commit, ops_per_commit=ops_commit / count,
                          msm_ops_per_s=ops_per_s, predicted_commits_per_s=predicted,
                          a_plain_fraction_of_predicted=res["a_plain"]["per_s"] / predicted)
    print(json.dumps({k: res[k] for k in ("b_msm", "b_model")}), flush=True)

    # (c) the prover at n = 64
    B, n = args.prove_batch, 64
    S = 2 * n + 4
    sc = masked(rng, B * S)
    scd = T(sc)
    rnd_a, sL_a, sR_a = scd[:4 * B].view(B, 4, 4), scd[4 * B:(4 + n) * B].view(B, n, 4), scd[(4 + n) * B:].view(B, n, 4)
    pv = np.zeros((B, 4), np.uint64)
    pv[:, 0] = rng.integers(0, 1 << 62, B, dtype=np.uint64)
    pvd, pgd, G, H = T(pv), T(gamma[:B]), T(d["G"]), T(d["H"])
    keep = {}

    def prove():
        keep["o"] = bp.batch_generate_range_proof(n, pvd, pgd, sL_a, sR_a, rnd_a, G, H, gd, hd)
    res["c_prover"] = stat(timed(prove, 3), B)
    res["c_prover"].update(B=B, n=n)
    cv = bp.batch_pedersen_commit(pvd, pgd, gd, hd)
    torch.cuda.synchronize()
    res["c_prover"]["V_equals_commit"] = bool(torch.equal(cv, keep["o"]["V"])) and bool(keep["o"]["valid"].all())
    res["c_prover"]["commit_speedup_per_V"] = res["a_plain"]["per_s"] / res["c_prover"]["per_s"]
    keep.clear()
    print(json.dumps({"c_prover": res["c_prover"]}), flush=True)

    # (d) sort A/B, alternating
    ab = dict(count=count, reps=reps, workloads={})
    for name, vv in (("uniform", vd), ("log_uniform", vlogd)):
        ms = {"0": [], "1": []}
        outs = {}
        for sw in ("0", "1"):   # warm both
            os.environ["HIPBP_COMMIT_SORT"] = sw
            bp.batch_pedersen_commit(vv, gamd, gd, hd, out=out)
            torch.cuda.synchronize()
            outs[sw] = out.clone()
        for _ in range(reps):
            for sw in ("0", "1"):
                os.environ["HIPBP_COMMIT_SORT"] = sw
                t0 = time.perf_counter()
                bp.batch_pedersen_commit(vv, gamd, gd, hd, out=out)
                torch.cuda.synchronize()
                ms[sw].append((time.perf_counter() - t0) * 1e3)
        off, on = stat(ms["0"], count), stat(ms["1"], count)
        gain = off["ms_median"] / on["ms_median"] - 1
        spread = (max(ms["0"]) - min(ms["0"])) / off["ms_median"]
        ab["workloads"][name] = dict(sort_off=off, sort_on=on, same_bytes=bool(torch.equal(outs["0"], outs["1"])),
                                     gain=gain, unsorted_spread=spread, gain_exceeds_spread=bool(gain > spread))
    del os.environ["HIPBP_COMMIT_SORT"]
    res["d_sort_ab"] = {k: dict(gain=w["gain"], unsorted_spread=w["unsorted_spread"],
                                gain_exceeds_spread=w["gain_exceeds_spread"]) for k, w in ab["workloads"].items()}
    print(json.dumps({"d_sort_ab": ab}), flush=True)

    # (e) the host call on one GPU
    host_ms = timed(lambda: bp.batch_pedersen_commit_host(v, gamma, g, h, num_gpus=1), 3)
    res["e_host"] = stat(host_ms, count)
    res["e_host"]["share_outside_kernels"] = 1 - res["a_plain"]["ms_median"] / res["e_host"]["ms_median"]
    res["e_host"]["equals_device"] = bool(np.array_equal(bp.batch_pedersen_commit_host(v, gamma, g, h, num_gpus=1),
                                                         plain.cpu().numpy().view(np.uint64)))
    print(json.dumps({"e_host": res["e_host"]}), flush=True)

    # (f) the crossover against one CPU commitment
    O = pyoracle.Oracle()
    cr.restate(O, v[0], gamma[0], g, h)
    t0 = time.perf_counter()
    for i in range(200):
        cr.restate(O, v[i], gamma[i], g, h)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / 200

    def dev_ms(c):
        return statistics.median(timed(lambda: bp.batch_pedersen_commit(vd[:c], gamd[:c], gd, hd, out=out[:c])))
    points = {}
    hi = 1
    while hi < count:
        points[hi] = dev_ms(hi)
        if points[hi] < hi * cpu_ms:
            break
        hi *= 2
    if hi not in points:
        points[hi] = dev_ms(hi)
    lo = hi // 2  # the device call loses at lo (or hi = 1 wins at once), wins at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        points[mid] = dev_ms(mid)
        if points[mid] < mid * cpu_ms:
            hi = mid
        else:
            lo = mid
    res["f_crossover"] = dict(cpu_ms_per_commit=cpu_ms, device_ms_at={str(k): points[k] for k in sorted(points)},
                              smallest_winning_count=hi, device_wins_there=bool(points[hi] < hi * cpu_ms))
    print(json.dumps({"f_crossover": res["f_crossover"]}), flush=True)

    res["multi_gpu_rate"] = "not measured (one-GPU session)"
    res["ok"] = bool(res["a_gens16_equals_plain"] and res["e_host"]["equals_device"] and
                     res["c_prover"]["V_equals_commit"] and all(w["same_bytes"] for w in ab["workloads"].values()))
    for path, obj in ((args.out, res), (args.ab_out, ab)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(obj, f, indent=1)
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

"""What the provers on host structs cost beside the device call (tools/, not a test; bench.py is the
flagship benchmark and does not run this).  DESIGN §15 holds the expectation and the results.

  python tools/bench_prove_host.py [--B 65536] [--n 64] [--reps 5] [--parent-d P1.json,P2.json]
                                   [--this-d T1.json,T2.json] [--out FILE.json]
  python tools/bench_prove_host.py --only-d [--root OTHER_CHECKOUT] [--calls 5] --out D.json

Shape: B proofs of n bits per call on tools/bench_prove_seeded.py's generators, values and blindings,
check 1, max_attempts 8, one device.  Each leg one warm-up call, then `reps` calls, the legs taken in
turn in one session.  The host legs are timed by tools/bench_prove_host_shim.c: the monotonic clock
around the C call and the freeing of every vector it handed out.

  (a)  batch_generate_range_proof_accepted on device tensors, no generator set (no prefix tables, as
       the host path): host clock around call + synchronise;
  (b)  hipbp_batch_generate_range_proof_accepted_host, num_gpus = 1.  (b) - (a) is the host path:
       staging, the D2H of 2401 bytes per proof, unpacking into malloc'ed vectors, freeing them;
  (bs) the same with HIPBP_PROVE_HOST_CHUNK = B: the chunk comes back as ONE piece, so no copy runs
       under any unpacking; 1 - ((b) - (a)) / ((bs) - (a)) is the share of the host path that the
       pieces' overlap hides;
  (c)  the same as (b) with HIPBP_PROVE_HOST_ACCEPT_CHUNK = 16384: the retry loop once per 16384
       proofs, what the chunk rule avoids; per extra retry round (from the attempts: a chunk runs as
       many rounds as its largest attempts value) beside DESIGN §14's 20 ms;
  (d)  hipbp_batch_generate_range_proof_host (the seeded prover, one device), `--only-d`: run for the
       parent checkout (`--root`, built there) and for this one in alternating processes of one
       session; the main run merges the files (--parent-d, --this-d) and says whether this
       checkout's median lies inside the parent's own min-max spread.

Outside the timed region (b)'s structs are compared with (a)'s tensors (every head field of every
proof, valid, attempts; a, b, L, R of 64 proofs spread over the batch)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from bench_prove_seeded import generators  # noqa: E402


def build_shim():
    """Compile the timing shim into build/ (gcc, a second)."""
    src = os.path.join(HERE, "bench_prove_host_shim.c")
    out = os.path.join(ROOT, "build", "bench_prove_host_shim.so")
    hdr = os.path.join(ROOT, "include", "cudabulletproof_hip.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", out])
    S = ctypes.CDLL(out)
    S.shim_seeded_host.restype = ctypes.c_double
    S.shim_accepted_host.restype = ctypes.c_double
    S.shim_free.restype = None
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="--only-d: timed calls")
    ap.add_argument("--root", default=ROOT, help="--only-d: import cudabulletproof_amd from this checkout (built there)")
    ap.add_argument("--only-d", action="store_true", help="leg (d) alone (any checkout with the host prover)")
    ap.add_argument("--parent-d", default=None, help="comma list of --only-d results from the parent checkout")
    ap.add_argument("--this-d", default=None, help="comma list of --only-d results from this checkout")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n = args.B, args.n

    import torch
    sys.path.insert(0, os.path.abspath(args.root))
    import cudabulletproof_amd as bp
    L = bp.lib()
    bp.require_gpu()
    S = build_shim()
    dev = torch.device("cuda:0")
    Gn, Hn, gn, hn = (np.ascontiguousarray(x, np.uint64) for x in generators(n))
    rng = np.random.default_rng(1)
    v = np.zeros((B, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << min(n, 62), B, dtype=np.uint64)
    gam = rng.integers(0, 1 << 62, (B, 4), dtype=np.uint64)
    seed = bytes(range(32))
    sd = (ctypes.c_uint8 * 32).from_buffer_copy(seed)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    fn = lambda f: ctypes.cast(f, ctypes.c_void_p)
    gv, hv = bp.PointVector(p(Gn).value, n), bp.PointVector(p(Hn).value, n)
    arr = (bp.RangeProofC * B)()
    valid, attempts = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    rc, call_ms = ctypes.c_int(0), ctypes.c_double(0)
    common = (p(v), p(gam), ctypes.c_size_t(B), ctypes.c_size_t(n), ctypes.byref(gv), ctypes.byref(hv), p(gn), p(hn), sd,
              ctypes.c_uint64(0))

    def seeded_host():
        ms = S.shim_seeded_host(fn(L.hipbp_batch_generate_range_proof_host), arr, p(valid), *common, ctypes.byref(rc),
                                ctypes.byref(call_ms))
        assert rc.value == 0, L.hipbp_last_error()
        return ms

    def emit(res):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))

    if args.only_d:
        seeded_host()
        ms = [seeded_host() for _ in range(args.calls)]
        emit(dict(B=B, n=n, root=os.path.relpath(os.path.abspath(args.root), ROOT), d_ms_all=ms,
                  d_ms_median=statistics.median(ms), valid=int(valid.sum())))
        return

    def accepted_host(keep=0, env=None):
        for k, val in (env or {}).items():
            os.environ[k] = str(val)
        ms = S.shim_accepted_host(fn(L.hipbp_batch_generate_range_proof_accepted_host), arr, p(valid), p(attempts), *common,
                                  ctypes.c_int(8), ctypes.c_int(1), ctypes.c_int(1), ctypes.c_int(keep), ctypes.byref(rc),
                                  ctypes.byref(call_ms))
        for k in env or {}:
            os.environ.pop(k)
        assert rc.value == 0, L.hipbp_last_error()
        return ms

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
    G, H, g, h = T(Gn), T(Hn), T(gn), T(hn)
    vd, gd = T(v), T(gam)
    out = {}

    def leg_a():
        t0 = time.perf_counter()
        out["a"] = bp.batch_generate_range_proof_accepted(n, vd, gd, seed, G, H, g, h, max_attempts=8, check=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = dict(a=leg_a, b=accepted_host, bs=lambda: accepted_host(env=dict(HIPBP_PROVE_HOST_CHUNK=B)),
                c=lambda: accepted_host(env=dict(HIPBP_PROVE_HOST_ACCEPT_CHUNK=16384)))
    ms = {k: [] for k in legs}
    for k, f in legs.items():   # warm-up
        f()
    for _ in range(args.reps):
        for k, f in legs.items():
            ms[k].append(f())
    med = {k: statistics.median(x) for k, x in ms.items()}
    res = dict(B=B, n=n, reps=args.reps, max_attempts=8, check=1, bytes_per_proof=5 * 128 + 7 * 32 + 2 * (n.bit_length() - 1) * 128 + 2)
    for k in legs:
        res[f"{k}_ms_median"], res[f"{k}_ms_all"] = med[k], ms[k]
    host, host_serial = med["b"] - med["a"], med["bs"] - med["a"]
    res.update(host_path_ms=host, host_path_share_of_b=host / med["b"], host_path_one_piece_ms=host_serial,
               overlap_share=1 - host / host_serial if host_serial > 0 else None,
               b_accepted_proofs_per_s=B / (med["b"] * 1e-3))

    # (b) once more with the vectors kept: the bits against (a)'s tensors, the stats, the rounds per chunk
    accepted_host(keep=1)
    st = bp.accepted_last_stats()
    o = out["a"]
    raw = np.frombuffer(arr, np.uint8).reshape(B, 880)
    d = {k: o[k].cpu().numpy() for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R")}
    same = np.array_equal(valid, o["valid"].cpu().numpy()) and np.array_equal(attempts, o["attempts"].cpu().numpy())
    for i, k in enumerate(("V", "A", "S", "T1", "T2")):
        same = same and np.array_equal(raw[:, 128 * i:128 * i + 128], d[k].view(np.uint8).reshape(B, 128))
    for k, off in (("taux", 640), ("mu", 672), ("t", 704), ("c", 776), ("x", 848)):
        same = same and np.array_equal(raw[:, off:off + 32], d[k].view(np.uint8).reshape(B, 32))
    Lr = n.bit_length() - 1
    for i in range(0, B, max(B // 64, 1)):
        ip = arr[i].ip_proof
        same = same and ip.n == n and ip.L_len == Lr
        for vec, k, size in ((ip.a, "a", 32), (ip.b, "b", 32), (ip.L, "L", 128 * Lr), (ip.R, "R", 128 * Lr)):
            same = same and ctypes.string_at(vec.elements, size) == d[k][i].tobytes()
    S.shim_free(arr, ctypes.c_size_t(B))
    rounds_in = lambda ch: [int(max(attempts[c0:c0 + ch].max(), 1)) for c0 in range(0, B, ch)]
    extra = sum(r - 1 for r in rounds_in(16384)) - sum(r - 1 for r in rounds_in(B))
    res.update(same_bits=bool(same), valid=int(valid.sum()), accepted=int((attempts > 0).sum()), rounds=st["rounds"],
               proved_per_round=st["proved"], rounds_per_16384_chunk=rounds_in(16384), extra_retry_rounds_c=extra,
               c_minus_b_ms=med["c"] - med["b"], c_minus_b_ms_per_extra_round=(med["c"] - med["b"]) / extra if extra else None)

    # (d): the seeded host prover here against the parent, from --only-d runs alternated in this session
    if args.parent_d and args.this_d:
        load = lambda files: [x for f in files.split(",") for x in json.load(open(f))["d_ms_all"]]
        par, this = load(args.parent_d), load(args.this_d)
        res.update(d_parent_ms_all=par, d_this_ms_all=this, d_parent_ms_median=statistics.median(par),
                   d_this_ms_median=statistics.median(this), d_parent_ms_min=min(par), d_parent_ms_max=max(par),
                   d_within_parent_spread=bool(min(par) <= statistics.median(this) <= max(par)))
    res["ok"] = res["same_bits"] and res["accepted"] == B
    emit(res)
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

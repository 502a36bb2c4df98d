"""What proof ids and a batch Merkle root cost on the GPU, against fingerprinting on the host (tools/,
not a test; bench.py is the flagship benchmark and does not run this).  One session on one GPU; one
accepted batch of `count` proofs at n = 64 with taux and mu (f = 1), made once by
hipbp_batch_generate_range_proof_accepted_host (check 1).

  python tools/bench_proof_ids.py [--log2 16] [--reps 5] [--out profiles/bench/proof_ids_p01.json]

The legs are alternated in one session, `reps` rounds after a warm-up round; medians and min-max:
  flat     hipbp_batch_proof_ids on the flat device batch              (HIP events around the call)
  blob     hipbp_blob_proof_ids on the encoded device blob             (HIP events)
  root     hipbp_merkle_root over the count ids                        (HIP events)
  host     what a caller does without them: the device blob copied to the host, then
           hipbp_blob_proof_ids_host (HIPBP_HOST_THREADS threads, by default the job's 16 CPUs) and
           hipbp_merkle_root_host (one thread); wall clock, the three parts also apart
"""
import argparse
import ctypes
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
    ap.add_argument("--log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    count, reps, n, f = 1 << args.log2, args.reps, 64, 1

    import torch

    import cudabulletproof_amd as bp
    L = bp.lib()
    bp.require_gpu()
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(ROOT, "tests", "golden", "proofs_n64.npz"))
    u = lambda a, w: np.ascontiguousarray(a, np.uint64).reshape(-1, w)
    G, H, g, h = u(d["G"], 16), u(d["H"], 16), u(d["g"], 16), u(d["h"], 16)
    gv, hv = bp.PointVector(G.ctypes.data, n), bp.PointVector(H.ctypes.data, n)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    sz, cv = ctypes.c_size_t, ctypes.c_void_p
    rng = np.random.default_rng(7)
    v = np.zeros((count, 4), np.uint64)
    v[:, 0] = rng.integers(0, 1 << 62, count, dtype=np.uint64)
    b = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    b[:, 31] &= 0x7F
    b[:, 0] &= 0xF8
    b[:, 31] |= 0x40
    gamma = np.ascontiguousarray(b).view("<u8").astype(np.uint64).reshape(count, 4)
    seed = (ctypes.c_uint8 * 32)(*range(32))

    def chk(rc):
        if rc != 0:
            raise SystemExit("error: " + L.hipbp_last_error().decode())

    arr = (bp.RangeProofC * count)()
    valid, attempts = np.zeros(count, np.uint8), np.zeros(count, np.uint8)
    chk(L.hipbp_batch_generate_range_proof_accepted_host(arr, p(valid), p(attempts), p(v), p(gamma), sz(count), sz(n),
                                                         ctypes.byref(gv), ctypes.byref(hv), p(g), p(h), seed,
                                                         ctypes.c_uint64(0), 8, 1, 1))
    cap = L.hipbp_proof_blob_bound(sz(count), sz(1), sz(6), ctypes.c_uint(f))
    blob = np.zeros(cap, np.uint8)
    nb = sz(0)
    chk(L.hipbp_proofs_encode_host(arr, sz(count), sz(n), f, p(blob), sz(cap), ctypes.byref(nb)))
    blob = np.ascontiguousarray(blob[:nb.value])
    info = bp.proof_blob_info(blob)
    del arr
    blob_t = torch.from_numpy(blob).to(dev)
    batch = bp.decode_proofs(blob_t)
    ic = bp.ProofBlobInfoC(info["count"], info["n"], info["ab_len"], info["L_len"], info["flags"], info["raw_count"], info["bytes"])
    bs = batch.c_struct()
    st = bp._stream_ptr(None)
    ids_a = torch.zeros(count, 32, dtype=torch.uint8, device=dev)
    ids_b = torch.zeros(count, 32, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    root = torch.zeros(32, dtype=torch.uint8, device=dev)
    host_blob = np.zeros(len(blob), np.uint8)
    host_ids = np.zeros(32 * count, np.uint8)
    host_root = np.zeros(32, np.uint8)
    parts = dict(d2h=[], ids=[], root=[])

    def event_ms(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    def leg_host():
        t0 = time.perf_counter()
        host_blob[:] = blob_t.cpu().numpy()
        t1 = time.perf_counter()
        chk(L.hipbp_blob_proof_ids_host(p(host_blob), sz(len(host_blob)), p(host_ids)))
        t2 = time.perf_counter()
        chk(L.hipbp_merkle_root_host(p(host_ids), sz(count), p(host_root)))
        t3 = time.perf_counter()
        parts["d2h"].append((t1 - t0) * 1e3); parts["ids"].append((t2 - t1) * 1e3); parts["root"].append((t3 - t2) * 1e3)
        return (t3 - t0) * 1e3

    legs = dict(
        flat=lambda: event_ms(lambda: chk(L.hipbp_batch_proof_ids(ctypes.byref(bs), f, cv(ids_a.data_ptr()), None, st))),
        blob=lambda: event_ms(lambda: chk(L.hipbp_blob_proof_ids(cv(blob_t.data_ptr()), ctypes.byref(ic), cv(ids_b.data_ptr()),
                                                                 cv(bad.data_ptr()), st))),
        root=lambda: event_ms(lambda: chk(L.hipbp_merkle_root(cv(ids_a.data_ptr()), sz(count), cv(root.data_ptr()), st))),
        host=leg_host)
    ms = {k: [] for k in legs}
    for r in range(reps + 1):   # round 0 warms up
        for k, fn in legs.items():
            t = fn()
            if r:
                ms[k].append(t)
    for k in parts:
        parts[k] = parts[k][1:]

    def stat(x):
        return dict(ms_median=statistics.median(x), ms_all=x, ms_spread=[min(x), max(x)])
    hashed = 32 * count + len(blob) - 32 - ((count + 7) & ~7)   # headers and records
    res = dict(count=count, n=n, f=f, reps=reps, blob_bytes=len(blob), raw_count=info["raw_count"], hashed_bytes=hashed,
               compressions=int((hashed + 64 * count) // 64), host_threads=os.environ.get("HIPBP_HOST_THREADS", "unset (16 at most)"),
               flat=stat(ms["flat"]), blob=stat(ms["blob"]), root=stat(ms["root"]), host=stat(ms["host"]),
               host_parts={k: stat(x) for k, x in parts.items()})
    same = bool(torch.equal(ids_a, ids_b)) and int(bad.item()) == 0
    same = same and ids_a.cpu().numpy().tobytes() == host_ids.tobytes() and root.cpu().numpy().tobytes() == host_root.tobytes()
    res["ok"] = same
    res["root"]["hex"] = host_root.tobytes().hex()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()

"""What the compact proof blobs cost and save (tools/, not a test; bench.py is the flagship benchmark
and does not run this).  One session on one GPU; one accepted batch of `count` proofs at n = 64, made
once by hipbp_batch_generate_range_proof_accepted_host (check 1), so every proof verifies.

  python tools/bench_codec.py [--log2 16] [--reps 5] [--out profiles/bench/codec_p01.json]
  python tools/bench_codec.py --structs-only [--package-root DIR]    # leg (a) alone, e.g. on another build

  size     blob bytes (taux and mu stored) against the 2400 bytes per proof of the structs' content;
           expected 1216 / 2400 plus one byte per proof with no raw proof
  kernels  hipbp_batch_proof_encode / _decode on the device batch, HIP events around the call, `reps`
           warm calls each: ms and GB/s of the bytes moved (the flat arrays' 2400 count bytes plus the
           blob's, each counted once)
  cpu      the host encoder and decoder (one thread), for scale
  verify   (a) hipbp_batch_range_proof_verify_host on the structs, (b)
           hipbp_batch_range_proof_verify_bytes_host (check 1) on the blob of the same proofs: the C
           entry points called directly on arrays built beforehand, `reps` runs each, interleaved in
           one process after a warm call of each, the same HIPBP_HOST_PREFIX_BITS; medians and min-max
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--structs-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose cudabulletproof_amd is measured")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    count, reps, n = 1 << args.log2, args.reps, 64

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
    sz = ctypes.c_size_t
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

    # the batch, as host structs
    arr = (bp.RangeProofC * count)()
    valid, attempts = np.zeros(count, np.uint8), np.zeros(count, np.uint8)
    t0 = time.perf_counter()
    chk(L.hipbp_batch_generate_range_proof_accepted_host(arr, p(valid), p(attempts), p(v), p(gamma), sz(count), sz(n),
                                                         ctypes.byref(gv), ctypes.byref(hv), p(g), p(h), seed,
                                                         ctypes.c_uint64(0), 8, 1, 1))
    res = dict(count=count, n=n, reps=reps, prefix_bits=os.environ.get("HIPBP_HOST_PREFIX_BITS", "unset (16)"),
               prove_s=time.perf_counter() - t0, accepted=int((attempts > 0).sum()),
               package_root=os.path.relpath(args.package_root, ROOT))
    V = np.frombuffer(arr, np.uint8).reshape(count, ctypes.sizeof(bp.RangeProofC))[:, :128].copy()
    ok_a, ok_b = np.zeros(count, np.uint8), np.zeros(count, np.uint8)

    def run_a():
        chk(L.hipbp_batch_range_proof_verify_host(arr, p(V), sz(count), sz(n), ctypes.byref(gv), ctypes.byref(hv), p(g),
                                                  p(h), 1, p(ok_a)))

    def stat(ms, items):
        med = statistics.median(ms)
        return dict(ms_median=med, ms_all=ms, ms_spread=[min(ms), max(ms)], per_s=items / (med * 1e-3),
                    per_s_spread=[items / (max(ms) * 1e-3), items / (min(ms) * 1e-3)])

    def clock(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    if args.structs_only:
        run_a()
        res["a_structs"] = stat([clock(run_a) for _ in range(reps)], count)
        res["ok"] = bool(np.array_equal(ok_a != 0, attempts > 0))
        return finish(args, res)

    # size, and the CPU codec
    f = 1
    cap = L.hipbp_proof_blob_bound(sz(count), sz(1), sz(6), ctypes.c_uint(f))
    blob = np.zeros(cap, np.uint8)
    nb = sz(0)
    t0 = time.perf_counter()
    chk(L.hipbp_proofs_encode_host(arr, sz(count), sz(n), f, p(blob), sz(cap), ctypes.byref(nb)))
    enc_cpu = time.perf_counter() - t0
    blob = np.ascontiguousarray(blob[:nb.value])
    info = bp.proof_blob_info(blob)
    back = (bp.RangeProofC * count)()
    t0 = time.perf_counter()
    chk(L.hipbp_proofs_decode_host(p(blob), sz(len(blob)), back))
    dec_cpu = time.perf_counter() - t0
    flat = 2400 * count
    res["size"] = dict(blob_bytes=len(blob), struct_content_bytes=flat, ratio=len(blob) / flat, raw_count=info["raw_count"],
                       expected_ratio=(1216 + 1) / 2400)
    res["cpu"] = dict(encode_s=enc_cpu, decode_s=dec_cpu, encode_MBps=flat / enc_cpu / 1e6, decode_MBps=flat / dec_cpu / 1e6)
    # (the decoded structs hold what went in: the parts outside ip_proof compared here, the rest by the tests)
    fixed = lambda a: np.frombuffer(a, np.uint8).reshape(count, ctypes.sizeof(bp.RangeProofC))[:, :736]   # up to ip_proof
    same = bool(np.array_equal(fixed(back), fixed(arr)))
    bp._take_proofs(back, count)   # frees the decoder's vectors
    print(json.dumps({k: res[k] for k in ("size", "cpu")}), flush=True)

    # the kernels
    blob_t = torch.from_numpy(blob).to(dev)
    batch = bp.decode_proofs(blob_t)
    ic = bp.ProofBlobInfoC(info["count"], info["n"], info["ab_len"], info["L_len"], info["flags"], info["raw_count"], info["bytes"])
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    oc = bp.ProofOutC(*[getattr(batch, k).data_ptr() if k != "valid" and getattr(batch, k).numel() else None
                        for k in bp._PROOF_KEYS])
    enc_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    nbd = torch.zeros(1, dtype=torch.int64, device=dev)
    bs = batch.c_struct()
    st = bp._stream_ptr(None)
    cv = ctypes.c_void_p

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            ms.append(a.elapsed_time(z))
        return ms
    moved = flat + len(blob)
    enc_ms = events(lambda: chk(L.hipbp_batch_proof_encode(ctypes.byref(bs), f, cv(enc_out.data_ptr()), sz(cap),
                                                           cv(nbd.data_ptr()), st)))
    dec_ms = events(lambda: chk(L.hipbp_batch_proof_decode(cv(blob_t.data_ptr()), ctypes.byref(ic), ctypes.byref(oc),
                                                           cv(bad.data_ptr()), st)))
    gpu_same = int(nbd.item()) == len(blob) and bool(torch.equal(enc_out[:len(blob)], blob_t)) and int(bad.item()) == 0
    res["kernels"] = dict(bytes_moved=moved, encode=stat(enc_ms, count), decode=stat(dec_ms, count),
                          encode_GBps=moved / (statistics.median(enc_ms) * 1e-3) / 1e9,
                          decode_GBps=moved / (statistics.median(dec_ms) * 1e-3) / 1e9, gpu_blob_equals_cpu_blob=gpu_same)
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    del batch, enc_out, blob_t
    torch.cuda.empty_cache()

    # host verify, structs against bytes
    def run_b():
        chk(L.hipbp_batch_range_proof_verify_bytes_host(p(blob), sz(len(blob)), p(V), sz(n), ctypes.byref(gv),
                                                        ctypes.byref(hv), p(g), p(h), 1, 1, p(ok_b)))
    run_a()
    run_b()
    ms_a, ms_b = [], []
    for _ in range(reps):
        ms_a.append(clock(run_a))
        ms_b.append(clock(run_b))
    res["a_structs"], res["b_bytes"] = stat(ms_a, count), stat(ms_b, count)
    res["b_median_below_a_minimum"] = bool(res["b_bytes"]["per_s"] < res["a_structs"]["per_s_spread"][0])
    res["ok"] = bool(same and gpu_same and np.array_equal(ok_a, ok_b) and np.array_equal(ok_a != 0, attempts > 0))
    finish(args, res)


def finish(args, res):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

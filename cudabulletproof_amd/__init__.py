"""cudabulletproof_amd — MI355X (gfx950) engine for the MSM / inner-product-argument hot path
of ronantakizawa/cudabulletproof.

The compute path is libcudabulletproof_hip.so (hand-written HIP in csrc/, C ABI in
include/cudabulletproof_hip.h).  This module is a thin ctypes layer over that ABI:

* reference-named entry points (``cuda_point_vector_multi_scalar_mul``,
  ``cuda_range_proof_verify`` ...) that take numpy arrays in the reference's layouts
  and behave like the reference's C functions (cuda_bulletproof.h:13-84);
* a batched, device-resident verify (``RangeProofBatch`` + ``batch_range_proof_verify``)
  on torch CUDA tensors, used by bench.py.

There is no CPU fallback: if the library is missing or no GPU is present the calls
raise.  Layouts (numpy uint64): fe25519 (..., 4), ge25519 (..., 16) = X|Y|Z|T.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libcudabulletproof_hip.so")
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["bp_terms1.hip", "bp_terms2.hip", "bp_terms4.hip", "bp_terms16.hip", "bp_kernels.hip", "bp_prove.hip",
           "bp_prove_seed.hip", "bp_ipa_prove.hip", "bp_pippenger.hip", "bp_commit.hip", "bp_codec.hip", "bp_ids.hip",
           "bp_gens_derive.hip",
           "bp_api_engine.hip", "bp_api_prove.hip", "bp_api_host.hip", "bp_api_blob.hip", "bp_api_ref.hip"]

_lib = None


class BulletproofError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 into LIB_PATH (in-tree, travels with the repo)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps.append(os.path.join(ROOT, "include", "cudabulletproof_hip.h"))
    if not force and os.path.exists(LIB_PATH):
        t = os.path.getmtime(LIB_PATH)
        if all(os.path.getmtime(d) <= t for d in deps):
            return LIB_PATH
    import tempfile
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
    flags += os.environ.get("HIPBP_EXTRA_CFLAGS", "").split()   # A/B builds (e.g. -DBP_TERMS_OCC=3)
    with tempfile.TemporaryDirectory() as tmp:   # one hipcc per source, in parallel, then link
        objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in srcs]
        procs = []
        for s, o in zip(srcs, objs):
            cmd = ["hipcc"] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, subprocess.Popen(cmd)))
        for cmd, p in procs:
            if p.wait() != 0:
                raise subprocess.CalledProcessError(p.returncode, cmd)
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


_c = ctypes.c_void_p
_sz = ctypes.c_size_t


class FieldVector(ctypes.Structure):
    _fields_ = [("elements", _c), ("length", _sz)]


PointVector = FieldVector


class InnerProductProof(ctypes.Structure):   # bulletproof_vectors.h:65-74 (144 bytes)
    _fields_ = [("n", _sz), ("a", FieldVector), ("b", FieldVector), ("c", ctypes.c_uint64 * 4),
                ("L", PointVector), ("R", PointVector), ("L_len", _sz), ("x", ctypes.c_uint64 * 4)]


class RangeProofC(ctypes.Structure):   # bulletproof_range_proof.h:7-18 (880 bytes)
    _fields_ = [("V", ctypes.c_uint64 * 16), ("A", ctypes.c_uint64 * 16), ("S", ctypes.c_uint64 * 16),
                ("T1", ctypes.c_uint64 * 16), ("T2", ctypes.c_uint64 * 16), ("taux", ctypes.c_uint64 * 4),
                ("mu", ctypes.c_uint64 * 4), ("t", ctypes.c_uint64 * 4), ("ip_proof", InnerProductProof)]


class ProofBatchC(ctypes.Structure):   # hipbp_proof_batch
    _fields_ = [("count", _sz), ("n", _sz), ("ab_len", _sz), ("L_len", _sz)] + \
               [(k, _c) for k in ("V", "A", "S", "T1", "T2", "t", "a", "b", "c", "x", "L", "R", "taux", "mu", "Vp")]


class ProveInputC(ctypes.Structure):   # hipbp_prove_input
    _fields_ = [("count", _sz), ("n", _sz)] + [(k, _c) for k in ("v", "gamma", "sL", "sR", "rnd")]


class ProofOutC(ctypes.Structure):   # hipbp_proof_out
    _fields_ = [(k, _c) for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R", "valid")]


class ProofBlobInfoC(ctypes.Structure):   # hipbp_proof_blob_info
    _fields_ = [("count", _sz), ("n", _sz), ("ab_len", _sz), ("L_len", _sz), ("flags", ctypes.c_uint),
                ("raw_count", _sz), ("bytes", _sz)]


class ProveIpaInputC(ctypes.Structure):   # hipbp_ipa_prove_input
    _fields_ = [("count", _sz), ("n", _sz)] + [(k, _c) for k in ("a", "b", "c", "transcript")]


class IpaProofOutC(ctypes.Structure):   # hipbp_ipa_proof_out
    _fields_ = [(k, _c) for k in ("a", "b", "c", "x", "c_final", "L", "R")]


assert ctypes.sizeof(InnerProductProof) == 144 and ctypes.sizeof(RangeProofC) == 880

EXPORTS = [
    "cuda_point_vector_multi_scalar_mul", "cuda_point_vector_multi_scalar_mul_shared",
    "cuda_field_vector_inner_product", "cuda_field_vector_inner_product_shared",
    "cuda_batch_field_vector_inner_product", "cuda_batch_field_add", "cuda_batch_field_sub",
    "cuda_batch_field_mul", "cuda_batch_field_mul_karatsuba", "cuda_batch_field_square",
    "cuda_batch_field_invert", "cuda_soa_field_add", "cuda_range_proof_verify", "cuda_inner_product_verify",
    "cuda_benchmark_multi_scalar_mul", "cuda_benchmark_inner_product", "cuda_benchmark_field_operations",
    "cuda_benchmark_range_proof", "hipbp_last_error", "hipbp_device_count", "hipbp_batch_range_proof_verify",
    "hipbp_batch_range_proof_verify_std", "hipbp_batch_range_proof_verify_gens", "hipbp_batch_inner_product_verify", "hipbp_batch_generate_range_proof", "hipbp_msm",
    "hipbp_msm_pippenger", "hipbp_msm_pippenger_batch", "hipbp_msm_pippenger_windows",
    "hipbp_msm_pippenger_horner", "hipbp_msm_batch", "hipbp_msm_batch_gens", "hipbp_point_tree", "hipbp_field_op",
    "hipbp_sha_probe", "hipbp_sm_probe", "hipbp_sm_form_probe", "hipbp_sync", "hipbp_timing_enable",
    "hipbp_timing_collect", "hipbp_kernel_count", "hipbp_kernel_name", "hipbp_pipeline_create",
    "hipbp_pipeline_push", "hipbp_pipeline_flush", "hipbp_pipeline_depth", "hipbp_pipeline_destroy",
    "hipbp_pipeline_defer_msm",
    "hipbp_release_stream_workspaces",
    "hipbp_batch_inner_product_prove", "hipbp_batch_inner_product_prove_gens", "hipbp_inner_product_prove_host",
    "hipbp_derive_prover_scalars", "hipbp_batch_generate_range_proof_seeded",
    "hipbp_batch_generate_range_proof_seeded_gens", "hipbp_batch_generate_range_proof_host",
    "hipbp_batch_generate_range_proof_accepted", "hipbp_batch_generate_range_proof_accepted_gens",
    "hipbp_derive_prover_scalars_at", "hipbp_accepted_last_stats",
    "hipbp_batch_generate_range_proof_host_sharded", "hipbp_batch_generate_range_proof_accepted_host",
    "hipbp_batch_pedersen_commit", "hipbp_batch_pedersen_commit_gens", "hipbp_batch_pedersen_open",
    "hipbp_batch_pedersen_commit_host",
    "hipbp_proof_blob_bound", "hipbp_proof_blob_header", "hipbp_proof_blob_parse", "hipbp_batch_proof_encode",
    "hipbp_batch_proof_decode", "hipbp_proofs_encode_host", "hipbp_proofs_decode_host",
    "hipbp_batch_range_proof_verify_bytes_host",
    "hipbp_batch_proof_ids", "hipbp_blob_proof_ids", "hipbp_merkle_root", "hipbp_proof_ids_host",
    "hipbp_blob_proof_ids_host", "hipbp_merkle_root_host", "hipbp_merkle_path_host", "hipbp_merkle_verify_host",
    "hipbp_derive_base_points", "hipbp_derive_single_point", "hipbp_derive_base_points_host",
    "hipbp_derive_single_point_host", "hipbp_gens_create_seeded", "hipbp_gens_copy_points",
]


def lib():
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BulletproofError(f"{LIB_PATH} missing: run cudabulletproof_amd.build() (hipcc, gfx950)")
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as
        # /opt/rocm's).  Importing torch first makes the dynamic loader bind this library to the
        # runtime torch uses, so device pointers, streams and torch.distributed interoperate.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.hipbp_last_error.restype = ctypes.c_char_p
        for f in ("cuda_range_proof_verify", "cuda_inner_product_verify"):
            getattr(L, f).restype = ctypes.c_bool
        for f in ("hipbp_batch_range_proof_verify", "hipbp_batch_range_proof_verify_host",
                  "hipbp_batch_range_proof_verify_std", "hipbp_batch_range_proof_verify_gens",
                  "hipbp_batch_inner_product_verify", "hipbp_batch_generate_range_proof", "hipbp_msm",
                  "hipbp_msm_pippenger", "hipbp_msm_pippenger_batch", "hipbp_msm_pippenger_windows",
                  "hipbp_msm_pippenger_horner", "hipbp_msm_batch", "hipbp_msm_batch_gens", "hipbp_point_tree",
                  "hipbp_field_op", "hipbp_sha_probe", "hipbp_sm_probe", "hipbp_sm_form_probe", "hipbp_sync",
                  "hipbp_device_count",
                  "hipbp_release_stream_workspaces", "hipbp_batch_inner_product_prove",
                  "hipbp_batch_inner_product_prove_gens", "hipbp_inner_product_prove_host",
                  "hipbp_derive_prover_scalars", "hipbp_batch_generate_range_proof_seeded",
                  "hipbp_batch_generate_range_proof_seeded_gens", "hipbp_batch_generate_range_proof_host",
                  "hipbp_batch_generate_range_proof_accepted", "hipbp_batch_generate_range_proof_accepted_gens",
                  "hipbp_derive_prover_scalars_at", "hipbp_accepted_last_stats",
                  "hipbp_batch_generate_range_proof_host_sharded", "hipbp_batch_generate_range_proof_accepted_host",
                  "hipbp_batch_pedersen_commit", "hipbp_batch_pedersen_commit_gens", "hipbp_batch_pedersen_open",
                  "hipbp_batch_pedersen_commit_host", "hipbp_proof_blob_header", "hipbp_proof_blob_parse",
                  "hipbp_batch_proof_encode", "hipbp_batch_proof_decode", "hipbp_proofs_encode_host",
                  "hipbp_proofs_decode_host", "hipbp_batch_range_proof_verify_bytes_host",
                  "hipbp_batch_proof_ids", "hipbp_blob_proof_ids", "hipbp_merkle_root", "hipbp_proof_ids_host",
                  "hipbp_blob_proof_ids_host", "hipbp_merkle_root_host", "hipbp_merkle_path_host",
                  "hipbp_merkle_verify_host", "hipbp_derive_base_points", "hipbp_derive_single_point",
                  "hipbp_derive_base_points_host", "hipbp_derive_single_point_host", "hipbp_gens_copy_points"):
            getattr(L, f).restype = ctypes.c_int
        L.hipbp_proof_blob_bound.restype = ctypes.c_size_t
        L.hipbp_gens_create_seeded.restype = ctypes.c_void_p
        _lib = L
    return _lib


def require_gpu():
    n = lib().hipbp_device_count()
    if n < 1:
        raise BulletproofError("no HIP device visible: the engine has no CPU fallback")
    return n


def _chk(rc):
    if rc != 0:
        raise BulletproofError(lib().hipbp_last_error().decode())


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _u64(a, last):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.shape[-1] != last:
        raise ValueError(f"expected trailing dimension {last}, got {a.shape}")
    return a


# ====================================================================== reference-named host API
def cuda_point_vector_multi_scalar_mul(scalars, points, shared=False):
    """cuda_bulletproof.h:13 (shared: :17, cuda_point_vector_multi_scalar_mul_shared) — canonical-tree
    MSM of device-normalized terms; both entry points compute the same tree."""
    require_gpu()
    s, P = _u64(scalars, 4), _u64(points, 16)
    if len(s) != len(P):
        raise ValueError("Vector lengths must match for multi-scalar multiplication")
    out = np.zeros(16, np.uint64)
    sv, pv = FieldVector(_p(s).value, len(s)), PointVector(_p(P).value, len(P))
    f = lib().cuda_point_vector_multi_scalar_mul_shared if shared else lib().cuda_point_vector_multi_scalar_mul
    f(_p(out), ctypes.byref(sv), ctypes.byref(pv))
    return out


def cuda_field_vector_inner_product(a, b, shared=False):
    """cuda_bulletproof.h:22/:26 — the reference's GPU reduction order."""
    require_gpu()
    a, b = _u64(a, 4), _u64(b, 4)
    out = np.zeros(4, np.uint64)
    av, bv = FieldVector(_p(a).value, len(a)), FieldVector(_p(b).value, len(b))
    f = lib().cuda_field_vector_inner_product_shared if shared else lib().cuda_field_vector_inner_product
    f(_p(out), ctypes.byref(av), ctypes.byref(bv))
    return out


def cuda_batch_field_vector_inner_product(a_vectors, b_vectors):
    require_gpu()
    a, b = _u64(a_vectors, 4), _u64(b_vectors, 4)
    nv, n = a.shape[0], a.shape[1]
    av = (FieldVector * nv)(*[FieldVector(_p(a).value + i * n * 32, n) for i in range(nv)])
    bv = (FieldVector * nv)(*[FieldVector(_p(b).value + i * n * 32, n) for i in range(nv)])
    out = np.zeros((nv, 4), np.uint64)
    lib().cuda_batch_field_vector_inner_product(_p(out), av, bv, _sz(nv))
    return out


def _field(name, a, b=None):
    require_gpu()
    a = _u64(a, 4).reshape(-1, 4)
    out = np.zeros_like(a)
    if b is None:
        getattr(lib(), name)(_p(out), _p(a), _sz(len(a)))
    else:
        b = _u64(b, 4).reshape(-1, 4)
        if len(b) != len(a):
            raise ValueError("length mismatch")
        getattr(lib(), name)(_p(out), _p(a), _p(b), _sz(len(a)))
    return out


def cuda_batch_field_add(a, b):
    return _field("cuda_batch_field_add", a, b)


def cuda_batch_field_sub(a, b):
    return _field("cuda_batch_field_sub", a, b)


def cuda_batch_field_mul(a, b):
    return _field("cuda_batch_field_mul", a, b)


def cuda_batch_field_mul_karatsuba(a, b):
    return _field("cuda_batch_field_mul_karatsuba", a, b)


def cuda_batch_field_square(a):
    return _field("cuda_batch_field_square", a)


def cuda_batch_field_invert(a):
    return _field("cuda_batch_field_invert", a)


def cuda_soa_field_add(a, b):
    return _field("cuda_soa_field_add", a, b)


def _range_proof_struct(proof, n, keep):
    """proof: dict(head (100,) u64 = V,A,S,T1,T2 | taux,mu,t,c,x ; a, b (k,4); L, R (m,16))."""
    head = np.asarray(proof["head"], np.uint64)
    a, b = _u64(proof["a"], 4), _u64(proof["b"], 4)
    L, R = _u64(proof["L"], 16).reshape(-1, 16), _u64(proof["R"], 16).reshape(-1, 16)
    keep += [a, b, L, R]
    rp = RangeProofC()
    for i, k in enumerate(("V", "A", "S", "T1", "T2")):
        getattr(rp, k)[:] = [int(v) for v in head[16 * i:16 * i + 16]]
    for i, k in enumerate(("taux", "mu", "t")):
        getattr(rp, k)[:] = [int(v) for v in head[80 + 4 * i:84 + 4 * i]]
    ip = rp.ip_proof
    ip.n = n
    ip.a = FieldVector(_p(a).value, len(a))
    ip.b = FieldVector(_p(b).value, len(b))
    ip.c[:] = [int(v) for v in head[92:96]]
    ip.L = PointVector(_p(L).value, len(L))
    ip.R = PointVector(_p(R).value, len(R))
    ip.L_len = len(L)
    ip.x[:] = [int(v) for v in head[96:100]]
    return rp


def cuda_range_proof_verify(proof, V, n, G, H, g, h):
    """cuda_bulletproof.h:61 — one proof, host arrays, returns bool (crv:82 semantics)."""
    require_gpu()
    keep = []
    rp = _range_proof_struct(proof, n, keep)
    V, g, h = _u64(V, 16), _u64(g, 16), _u64(h, 16)
    G, H = _u64(G, 16), _u64(H, 16)
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    return bool(lib().cuda_range_proof_verify(ctypes.byref(rp), _p(V), _sz(n), ctypes.byref(gv), ctypes.byref(hv),
                                              _p(g), _p(h)))


def batch_range_proof_verify_host(proofs, V, n, G, H, g, h, num_gpus=0):
    """hipbp_batch_range_proof_verify_host: cuda_range_proof_verify over a list of proofs (the
    dicts cuda_range_proof_verify takes) packed as an array of the reference's RangeProof structs,
    sharded over num_gpus devices (0: all) from the current device on.  Host arrays in, (count,) bool
    verdicts out."""
    require_gpu()
    keep = []
    count = len(proofs)
    arr = (RangeProofC * max(count, 1))()
    for i, pr in enumerate(proofs):
        arr[i] = _range_proof_struct(pr, n, keep)
    V = _u64(V, 16).reshape(-1, 16)
    g, h = _u64(g, 16), _u64(h, 16)
    G, H = _u64(G, 16), _u64(H, 16)
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    ok = np.zeros(max(count, 1), np.uint8)
    _chk(lib().hipbp_batch_range_proof_verify_host(arr, _p(V), _sz(count), _sz(n), ctypes.byref(gv), ctypes.byref(hv),
                                                   _p(g), _p(h), ctypes.c_int(num_gpus), _p(ok)))
    return ok[:count].astype(bool)


def cuda_inner_product_verify(proof, P, G, H, Q):
    """cuda_bulletproof.h:72 — the IPA check alone (crv:130 semantics)."""
    require_gpu()
    keep = []
    G, H = _u64(G, 16), _u64(H, 16)
    rp = _range_proof_struct(proof, len(G), keep)
    P, Q = _u64(P, 16), _u64(Q, 16)
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    return bool(lib().cuda_inner_product_verify(ctypes.byref(rp.ip_proof), _p(P), ctypes.byref(gv), ctypes.byref(hv),
                                                _p(Q)))


# ====================================================================== batched device API (torch)
class RangeProofBatch:
    """A batch of proofs in the flat wire format, resident on a torch CUDA device.

    Tensors are int64 views of the u64 limbs: V/A/S/T1/T2 (B,16), t/c/x (B,4),
    a/b (B,ab_len,4), L/R (B,L_len,16).  Optional (range_proof_verify semantics only):
    taux/mu (B,4) and Vp (B,16), the proof's own V (default: V).
    """

    FIELDS = ("V", "A", "S", "T1", "T2", "t", "a", "b", "c", "x", "L", "R")
    OPTIONAL = ("taux", "mu", "Vp")

    def __init__(self, n, **tensors):
        self.n = int(n)
        for k in self.FIELDS:
            setattr(self, k, tensors[k].contiguous())
        for k in self.OPTIONAL:
            v = tensors.get(k)
            setattr(self, k, v.contiguous() if v is not None else None)
        self.count = int(self.V.shape[0])
        self.ab_len = int(self.a.shape[1])
        self.L_len = int(self.L.shape[1])

    @classmethod
    def from_numpy(cls, n, arrays, device):
        import torch
        t = {k: torch.from_numpy(np.ascontiguousarray(arrays[k]).view(np.int64)).to(device)
             for k in cls.FIELDS + cls.OPTIONAL if arrays.get(k) is not None}
        return cls(n, **t)

    def c_struct(self):
        s = ProofBatchC(self.count, self.n, self.ab_len, self.L_len)
        for k in self.FIELDS:
            setattr(s, k, getattr(self, k).data_ptr())
        for k in self.OPTIONAL:
            v = getattr(self, k)
            setattr(s, k, v.data_ptr() if v is not None else None)
        return s

    def nbytes(self):
        return sum(getattr(self, k).numel() * 8 for k in self.FIELDS)


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def batch_range_proof_verify(batch, G, H, g, h, ok, P_out=None, check_out=None, stream=None):
    """Enqueue cuda_range_proof_verify over the whole batch on `stream` (asynchronous).

    G/H: (n,16) int64 CUDA tensors, g/h: (16,), ok: (B,) uint8, P_out/check_out: (B,16) or None.
    """
    s = batch.c_struct()
    _chk(lib().hipbp_batch_range_proof_verify(
        ctypes.byref(s), _c(G.data_ptr()), _c(H.data_ptr()), _c(g.data_ptr()), _c(h.data_ptr()), _c(ok.data_ptr()),
        _c(P_out.data_ptr()) if P_out is not None else None,
        _c(check_out.data_ptr()) if check_out is not None else None, _stream_ptr(stream)))


def batch_range_proof_verify_gens(batch, gens, ok, P_out=None, check_out=None, stream=None):
    """batch_range_proof_verify with a Generators set's generators and prefix tables
    (hipbp_batch_range_proof_verify_gens): same bits, the table-started scalar multiplications."""
    s = batch.c_struct()
    _chk(lib().hipbp_batch_range_proof_verify_gens(
        ctypes.byref(s), _c(gens.h), _c(ok.data_ptr()), _c(P_out.data_ptr()) if P_out is not None else None,
        _c(check_out.data_ptr()) if check_out is not None else None, _stream_ptr(stream)))


def batch_range_proof_verify_std(batch, G, H, g, h, ok, P_out=None, check_out=None, flags_out=None, poly_out=None,
                                 stream=None):
    """Enqueue range_proof_verify semantics (bulletproof_range_proof.cu:1717) over the
    batch (needs batch.taux/mu).  flags_out (B,) uint8: bit0 V match, bit1 range check, bit2
    polynomial identity methods 1|2, bit3 method 3, bit4 method 4, bit5 inner_product_verify;
    poly_out (B,4,16): left, right, chal*left, chal*right."""
    s = batch.c_struct()
    opt = lambda t: _c(t.data_ptr()) if t is not None else None
    _chk(lib().hipbp_batch_range_proof_verify_std(
        ctypes.byref(s), _c(G.data_ptr()), _c(H.data_ptr()), _c(g.data_ptr()), _c(h.data_ptr()), _c(ok.data_ptr()),
        opt(P_out), opt(check_out), opt(flags_out), opt(poly_out), _stream_ptr(stream)))


def batch_inner_product_verify(batch, P, G, H, Q, ok, check_out=None, stream=None):
    s = batch.c_struct()
    _chk(lib().hipbp_batch_inner_product_verify(
        ctypes.byref(s), _c(P.data_ptr()), _c(G.data_ptr()), _c(H.data_ptr()), _c(Q.data_ptr()), _c(ok.data_ptr()),
        _c(check_out.data_ptr()) if check_out is not None else None, _stream_ptr(stream)))


class Generators:
    """hipbp_gens_create: a device snapshot of the generators G (n,16), H (n,16), g, h (16,) and,
    with prefix_bits > 0, their fixed-base prefix tables ((2n + 2) * 2^bits * 128 bytes).  Pass it
    to batch_generate_range_proof(gens=...) and VerifyPipeline.use_gens(); results keep their bits."""

    def __init__(self, n, G, H, g, h, prefix_bits=0, stream=None):
        L = lib()
        L.hipbp_gens_create.restype = ctypes.c_void_p
        self.n, self.bits = int(n), int(prefix_bits)
        self.h = L.hipbp_gens_create(_sz(n), _c(G.data_ptr()), _c(H.data_ptr()), _c(g.data_ptr()), _c(h.data_ptr()),
                                     ctypes.c_int(self.bits), _stream_ptr(stream))
        if not self.h:
            raise BulletproofError(L.hipbp_last_error().decode())

    @classmethod
    def from_seeds(cls, n, seed_G=None, seed_H=None, seed_g=None, seed_h=None, prefix_bits=0, stream=None):
        """hipbp_gens_create_seeded: the set whose G, H are derive_base_points(seed_G / seed_H, n) and
        whose g, h are derive_single_point(seed_g / seed_h), derived in place on the GPU.
        The defaults are REFERENCE_SEEDS, the reference test driver's generators.  points() hands the
        arrays out for the entry points that take them."""
        L = lib()
        seeds = [_gen_seed(REFERENCE_SEEDS[k] if s is None else s)
                 for k, s in zip(("G", "H", "g", "h"), (seed_G, seed_H, seed_g, seed_h))]
        self = cls.__new__(cls)
        self.n, self.bits = int(n), int(prefix_bits)
        self.h = L.hipbp_gens_create_seeded(_sz(n), *seeds, ctypes.c_int(self.bits), _stream_ptr(stream))
        if not self.h:
            raise BulletproofError(L.hipbp_last_error().decode())
        return self

    def points(self, stream=None):
        """hipbp_gens_copy_points: (G (n,16), H (n,16), g (16,), h (16,)) as new int64 CUDA tensors on
        the current device, copies of the set's snapshot.  Asynchronous on `stream`."""
        import contextlib

        import torch
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device="cuda")
            G, H, g, h = z(self.n, 16), z(self.n, 16), z(16), z(16)
        _chk(lib().hipbp_gens_copy_points(_c(self.h), _c(G.data_ptr()), _c(H.data_ptr()), _c(g.data_ptr()),
                                          _c(h.data_ptr()), None, None, _stream_ptr(stream)))
        return G, H, g, h

    def nbytes_tables(self):
        return (2 * self.n + 2) * (1 << self.bits) * 128 if self.bits else 0

    def close(self):
        if self.h:
            lib().hipbp_gens_destroy(_c(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_PROOF_KEYS = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R", "valid")


def _proof_out(B, n, dev, stream):
    """The prover's fifteen output tensors (_PROOF_KEYS) and the hipbp_proof_out over them.  Every
    output element is written by the prover (refused proofs get the reference's zeroed proof), so the
    buffers are allocated uninitialised on the stream the prover runs on."""
    import contextlib

    import torch
    Lr = max(int(n).bit_length() - 1, 0)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
        out = dict(V=z(B, 16), A=z(B, 16), S=z(B, 16), T1=z(B, 16), T2=z(B, 16), taux=z(B, 4), mu=z(B, 4),
                   t=z(B, 4), c=z(B, 4), x=z(B, 4), a=z(B, 1, 4), b=z(B, 1, 4), L=z(B, Lr, 16), R=z(B, Lr, 16),
                   valid=torch.empty(B, dtype=torch.uint8, device=dev))
    return out, ProofOutC(*[out[k].data_ptr() if out[k].numel() else None for k in _PROOF_KEYS])


def batch_generate_range_proof(n, v, gamma, sL, sR, rnd, G, H, g, h, stream=None, gens=None):
    """generate_range_proof (bulletproof_range_proof.cu:1159) over a batch, on the GPU.

    v, gamma (B,4); sL, sR (B,n,4); rnd (B,4,4) = alpha, rho, tau1, tau2: int64 CUDA tensors of the
    u64 limbs (the random scalars exactly as generate_random_scalar produced them).  Returns a dict
    of CUDA tensors in RangeProofBatch layout (V, A, S, T1, T2, t, a, b, c, x, L, R, taux, mu) plus
    "valid" (B,) uint8; RangeProofBatch(n, **out) verifies it directly."""
    B = int(v.shape[0])
    out, oc = _proof_out(B, n, v.device, stream)
    ins = [t.contiguous() for t in (v, gamma, sL, sR, rnd)]
    ic = ProveInputC(B, int(n), *[t.data_ptr() for t in ins])
    if gens is not None:   # the set's generators and prefix tables (G, H, g, h are not read)
        _chk(lib().hipbp_batch_generate_range_proof_gens(ctypes.byref(ic), _c(gens.h), ctypes.byref(oc),
                                                         _stream_ptr(stream)))
    else:
        _chk(lib().hipbp_batch_generate_range_proof(ctypes.byref(ic), _c(G.data_ptr()), _c(H.data_ptr()),
                                                    _c(g.data_ptr()), _c(h.data_ptr()), ctypes.byref(oc),
                                                    _stream_ptr(stream)))
    out["_keep"] = ins
    return out


# ---------------------------------------------------------------------- seeded prover
def _seed_arg(seed):
    """The 32 secret seed bytes as a ctypes buffer (the C ABI reads them during the call)."""
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError(f"seed must be 32 bytes, got {len(seed)}")
    return (ctypes.c_uint8 * 32).from_buffer_copy(seed)


def derive_prover_scalars(n, v, gamma, seed, index_base=0, stream=None):
    """hipbp_derive_prover_scalars: the seeded prover's derivation alone, on the GPU.

    v, gamma (B,4) int64 CUDA tensors of the u64 limbs; seed: 32 secret bytes; proof p of the call
    has the global index index_base + p (mod 2^64).  Returns dict(sL (B,n,4), sR (B,n,4), rnd (B,4,4))
    of int64 CUDA tensors: what batch_generate_range_proof takes and what
    batch_generate_range_proof_seeded proves with."""
    import contextlib

    import torch
    sd = _seed_arg(seed)
    B, n = int(v.shape[0]), int(n)
    ins = [v.contiguous(), gamma.contiguous()]
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=v.device)
        out = dict(sL=z(B, n, 4), sR=z(B, n, 4), rnd=z(B, 4, 4))
    _chk(lib().hipbp_derive_prover_scalars(sd, _c(ins[0].data_ptr()), _c(ins[1].data_ptr()),
                                           ctypes.c_uint64(int(index_base) & (2**64 - 1)), _sz(B), _sz(n),
                                           _c(out["sL"].data_ptr()), _c(out["sR"].data_ptr()),
                                           _c(out["rnd"].data_ptr()), _stream_ptr(stream)))
    out["_keep"] = ins
    return out


def batch_generate_range_proof_seeded(n, v, gamma, seed, G, H, g, h, index_base=0, stream=None, gens=None):
    """batch_generate_range_proof with its random scalars derived on the GPU from a 32-byte secret
    seed (hipbp_batch_generate_range_proof_seeded; derivation: DESIGN §13): the proofs of
    batch_generate_range_proof(n, v, gamma, **derive_prover_scalars(n, v, gamma, seed, index_base)),
    bit for bit, without the scalars ever being the caller's.  v, gamma (B,4) int64 CUDA tensors;
    proof p has the global index index_base + p, so a batch cut into several calls gives the proofs
    of the single call.  Returns batch_generate_range_proof's dict."""
    sd = _seed_arg(seed)
    B = int(v.shape[0])
    out, oc = _proof_out(B, n, v.device, stream)
    ins = [v.contiguous(), gamma.contiguous()]
    ic = ProveInputC(B, int(n), ins[0].data_ptr(), ins[1].data_ptr(), None, None, None)
    ib = ctypes.c_uint64(int(index_base) & (2**64 - 1))
    if gens is not None:   # the set's generators and prefix tables (G, H, g, h are not read)
        _chk(lib().hipbp_batch_generate_range_proof_seeded_gens(ctypes.byref(ic), sd, ib, _c(gens.h), ctypes.byref(oc),
                                                                _stream_ptr(stream)))
    else:
        _chk(lib().hipbp_batch_generate_range_proof_seeded(ctypes.byref(ic), sd, ib, _c(G.data_ptr()), _c(H.data_ptr()),
                                                           _c(g.data_ptr()), _c(h.data_ptr()), ctypes.byref(oc),
                                                           _stream_ptr(stream)))
    out["_keep"] = ins
    return out


# ---------------------------------------------------------------------- generators from seeds
# the reference test driver's seeds (complete_bulletproof_test.cu:66-109): byte k, then 31 zeros
REFERENCE_SEEDS = {k: bytes([b]) + bytes(31) for k, b in (("G", 1), ("H", 2), ("g", 3), ("h", 4))}


def _gen_seed(seed):
    """A generator seed for the C ABI: 32 bytes, or an int 0..255 for that byte followed by 31 zeros
    (None stays None: the C ABI's null seed)."""
    if seed is None:
        return None
    if isinstance(seed, (int, np.integer)):
        if not 0 <= int(seed) <= 255:
            raise ValueError(f"an int seed must be 0..255, got {seed}")
        seed = bytes([int(seed)]) + bytes(31)
    return _seed_arg(seed)


def derive_base_points(seed, count, first=0, out=None, stream=None):
    """hipbp_derive_base_points: points first .. first + count - 1 of the seed's generator
    vector, derived on the GPU: X = SHA-256(seed | BE32(i)), Y = SHA-256(X's bytes), Z = 1, T = X * Y
    in the reference's arithmetic, the reference test driver's rule bit for bit.  first + count <= 2^32.
    out: a contiguous (count,16) int64 CUDA tensor to write, or None for a new one on the current
    device.  Asynchronous on `stream`.  Returns the (count,16) tensor."""
    import contextlib

    import torch
    count = int(count)
    if out is None:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            out = torch.empty(count, 16, dtype=torch.int64, device="cuda")
    elif out.dtype != torch.int64 or tuple(out.shape) != (count, 16) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({count}, 16) int64 tensor")
    sd = _gen_seed(seed)
    if count:   # (an empty tensor has no address to pass)
        _chk(lib().hipbp_derive_base_points(_c(out.data_ptr()), sd, ctypes.c_uint64(int(first)), _sz(count),
                                            _stream_ptr(stream)))
    return out


def derive_single_point(seed, stream=None):
    """hipbp_derive_single_point: the seed's single generator (the reference driver's g, h rule):
    X = SHA-256(seed), Y = Z = 1, T = X * 1 in the reference's arithmetic.  Returns a (16,) int64 CUDA
    tensor on the current device.  Asynchronous on `stream`."""
    import contextlib

    import torch
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        out = torch.empty(16, dtype=torch.int64, device="cuda")
    _chk(lib().hipbp_derive_single_point(_c(out.data_ptr()), _gen_seed(seed), _stream_ptr(stream)))
    return out


def derive_base_points_host(seed, count, first=0):
    """hipbp_derive_base_points_host: derive_base_points on the CPU; a (count,16) uint64 array with the
    device call's bytes.  Needs no GPU."""
    out = np.zeros((int(count), 16), np.uint64)
    _chk(lib().hipbp_derive_base_points_host(_p(out), _gen_seed(seed), ctypes.c_uint64(int(first)), _sz(int(count))))
    return out


def derive_single_point_host(seed):
    """hipbp_derive_single_point_host: derive_single_point on the CPU; a (16,) uint64 array.  Needs no GPU."""
    out = np.zeros(16, np.uint64)
    _chk(lib().hipbp_derive_single_point_host(_p(out), _gen_seed(seed)))
    return out


# ---------------------------------------------------------------------- accepted prover
def derive_prover_scalars_at(n, v, gamma, seed, attempt=None, index_base=0, stream=None):
    """hipbp_derive_prover_scalars_at: derive_prover_scalars for chosen attempts.

    attempt: (B,) uint8 CUDA tensor, proof p's 0-based attempt index (its scalars come from the try
    key key_{p, attempt[p]}); None: every proof's attempt 0, derive_prover_scalars itself.  With
    attempt = max(attempts, 1) - 1 of a batch_generate_range_proof_accepted result these are the
    scalars its proofs were proved with.  Returns derive_prover_scalars' dict."""
    import contextlib

    import torch
    sd = _seed_arg(seed)
    B, n = int(v.shape[0]), int(n)
    ins = [v.contiguous(), gamma.contiguous()]
    if attempt is not None:
        if attempt.dtype != torch.uint8 or tuple(attempt.shape) != (B,):
            raise ValueError(f"attempt must be a ({B},) uint8 tensor")
        ins.append(attempt.contiguous())
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=v.device)
        out = dict(sL=z(B, n, 4), sR=z(B, n, 4), rnd=z(B, 4, 4))
    _chk(lib().hipbp_derive_prover_scalars_at(sd, _c(ins[0].data_ptr()), _c(ins[1].data_ptr()),
                                              ctypes.c_uint64(int(index_base) & (2**64 - 1)),
                                              _c(ins[2].data_ptr()) if attempt is not None else None, _sz(B), _sz(n),
                                              _c(out["sL"].data_ptr()), _c(out["sR"].data_ptr()),
                                              _c(out["rnd"].data_ptr()), _stream_ptr(stream)))
    out["_keep"] = ins
    return out


def batch_generate_range_proof_accepted(n, v, gamma, seed, G, H, g, h, index_base=0, max_attempts=8, check=1,
                                        stream=None, gens=None):
    """batch_generate_range_proof_seeded whose proofs the library's own verifier accepts
    (hipbp_batch_generate_range_proof_accepted): the seeded proofs are verified on the
    GPU (check 1: batch_range_proof_verify's semantics, check 2: batch_range_proof_verify_std's) and
    each rejected one is proved again, up to max_attempts (1..16) attempts in all, with the scalars
    of its next try key.  SYNCHRONOUS: the outputs are complete on return.

    Returns the prover's dict plus "attempts" (B,) uint8: k >= 1, accepted at the k-th attempt (the
    proof of derive_prover_scalars_at(attempt = k - 1)); 0, refused (valid 0) or not accepted
    within max_attempts (valid 1; the last attempt's proof)."""
    import contextlib

    import torch
    sd = _seed_arg(seed)
    B = int(v.shape[0])
    out, oc = _proof_out(B, n, v.device, stream)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        out["attempts"] = torch.empty(B, dtype=torch.uint8, device=v.device)
    ins = [v.contiguous(), gamma.contiguous()]
    ic = ProveInputC(B, int(n), ins[0].data_ptr(), ins[1].data_ptr(), None, None, None)
    ib = ctypes.c_uint64(int(index_base) & (2**64 - 1))
    tail = (ctypes.byref(oc), _c(out["attempts"].data_ptr()), _stream_ptr(stream))
    if gens is not None:   # the set's generators and prefix tables (G, H, g, h are not read)
        _chk(lib().hipbp_batch_generate_range_proof_accepted_gens(ctypes.byref(ic), sd, ib, ctypes.c_int(max_attempts),
                                                                  ctypes.c_int(check), _c(gens.h), *tail))
    else:
        _chk(lib().hipbp_batch_generate_range_proof_accepted(ctypes.byref(ic), sd, ib, ctypes.c_int(max_attempts),
                                                             ctypes.c_int(check), _c(G.data_ptr()), _c(H.data_ptr()),
                                                             _c(g.data_ptr()), _c(h.data_ptr()), *tail))
    out["_keep"] = ins
    return out


def accepted_last_stats():
    """hipbp_accepted_last_stats: the calling thread's last accepted call as dict(rounds, proved (the
    proofs proved in each round), kernel_ms (try_keys, select, scatter; zeros unless
    HIPBP_ACCEPT_TIMING=1 was set when the call ran))."""
    r = ctypes.c_int(0)
    m = (ctypes.c_uint32 * 16)()
    ms = (ctypes.c_float * 3)()
    _chk(lib().hipbp_accepted_last_stats(ctypes.byref(r), m, ms))
    return dict(rounds=r.value, proved=list(m)[:r.value],
                kernel_ms=dict(zip(("try_keys", "select", "scatter"), (float(x) for x in ms))))


def _take(vec, words):
    """A malloc'ed FieldVector / PointVector the library handed out, as a (length, words) uint64
    array; the C vector is freed."""
    if _take.free is None:
        _take.free = ctypes.CDLL(None).free
        _take.free.argtypes = [ctypes.c_void_p]
    out = np.ctypeslib.as_array(ctypes.cast(vec.elements, ctypes.POINTER(ctypes.c_uint64)),
                                shape=(vec.length, words)).copy() if vec.length else np.zeros((0, words), np.uint64)
    _take.free(vec.elements)
    return out


_take.free = None   # libc's free, looked up on first use


def _host_prove_args(v, gamma, G, H, g, h, seed):
    """The host provers' arguments as the C ABI takes them: (seed buffer, v, gamma, G, H, g, h, count)."""
    sd = _seed_arg(seed)
    v, gamma = _u64(v, 4).reshape(-1, 4), _u64(gamma, 4).reshape(-1, 4)
    if len(v) != len(gamma):
        raise ValueError("v and gamma must have the same length")
    G, H, g, h = _u64(G, 16), _u64(H, 16), _u64(g, 16), _u64(h, 16)
    return sd, v, gamma, G, H, g, h, len(v)


def _take_proofs(arr, count):
    """The structs a host prover filled as proof dicts; every vector is freed through _take."""
    proofs = []
    for i in range(count):
        rp = arr[i]
        ip = rp.ip_proof
        head = np.concatenate([np.array(getattr(rp, k), np.uint64) for k in ("V", "A", "S", "T1", "T2", "taux", "mu", "t")] +
                              [np.array(ip.c, np.uint64), np.array(ip.x, np.uint64)])
        proofs.append(dict(head=head, a=_take(ip.a, 4), b=_take(ip.b, 4), L=_take(ip.L, 16), R=_take(ip.R, 16),
                           n=int(ip.n), L_len=int(ip.L_len)))
    return proofs


def batch_generate_range_proof_host(v, gamma, n, G, H, g, h, seed, index_base=0, num_gpus=1):
    """hipbp_batch_generate_range_proof_host_sharded: the seeded prover on host arrays, through the
    reference's own RangeProof structs.  v, gamma (count,4), G, H (n,16), g, h (16,) uint64; seed 32
    secret bytes.  Returns (proofs, valid): a list of the proof dicts cuda_range_proof_verify and
    batch_range_proof_verify_host take (head (100,) = V,A,S,T1,T2 | taux,mu,t,c,x; a, b (1,4); L, R
    (log2 n,16)) and a (count,) bool array.  A refused value (valid False) has the zeroed proof:
    empty a, b, L, R.  Synchronous.  num_gpus: the devices the batch is split over, from the current
    one on (1: the current device alone; 0: all visible); the result does not depend on it."""
    require_gpu()
    sd, v, gamma, G, H, g, h, count = _host_prove_args(v, gamma, G, H, g, h, seed)
    arr = (RangeProofC * max(count, 1))()
    valid = np.zeros(max(count, 1), np.uint8)
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    _chk(lib().hipbp_batch_generate_range_proof_host_sharded(arr, _p(valid), _p(v), _p(gamma), _sz(count), _sz(int(n)),
                                                             ctypes.byref(gv), ctypes.byref(hv), _p(g), _p(h), sd,
                                                             ctypes.c_uint64(int(index_base) & (2**64 - 1)),
                                                             ctypes.c_int(num_gpus)))
    return _take_proofs(arr, count), valid[:count].astype(bool)


def batch_generate_range_proof_accepted_host(v, gamma, n, G, H, g, h, seed, index_base=0, max_attempts=8, check=1,
                                             num_gpus=1):
    """hipbp_batch_generate_range_proof_accepted_host: the accepted prover on host
    arrays; batch_generate_range_proof_host's arguments and proof dicts, batch_generate_range_proof_accepted's
    max_attempts and check.  Returns (proofs, valid, attempts): attempts (count,) uint8, k >= 1 accepted
    at the k-th attempt; 0 refused (valid False, the zeroed proof) or not accepted within max_attempts
    (valid True, the last attempt's proof).  accepted_last_stats() afterwards reports the whole call."""
    require_gpu()
    sd, v, gamma, G, H, g, h, count = _host_prove_args(v, gamma, G, H, g, h, seed)
    arr = (RangeProofC * max(count, 1))()
    valid = np.zeros(max(count, 1), np.uint8)
    attempts = np.zeros(max(count, 1), np.uint8)
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    _chk(lib().hipbp_batch_generate_range_proof_accepted_host(arr, _p(valid), _p(attempts), _p(v), _p(gamma), _sz(count),
                                                              _sz(int(n)), ctypes.byref(gv), ctypes.byref(hv), _p(g),
                                                              _p(h), sd, ctypes.c_uint64(int(index_base) & (2**64 - 1)),
                                                              ctypes.c_int(max_attempts), ctypes.c_int(check),
                                                              ctypes.c_int(num_gpus)))
    return _take_proofs(arr, count), valid[:count].astype(bool), attempts[:count].copy()


# ---------------------------------------------------------------------- Pedersen commitments
def _commit_args(v, gamma, g, h, gens):
    """(count, [v, gamma, g, h] contiguous; g, h None with a generator set) of a commit / open call."""
    if gens is None and (g is None or h is None):
        raise ValueError("g and h are needed without a generator set")
    ins = [v.contiguous(), gamma.contiguous()] + [None if gens is not None else t.contiguous() for t in (g, h)]
    count = int(ins[0].numel() // 4)
    if ins[0].numel() != count * 4 or ins[1].numel() != count * 4:
        raise ValueError("v and gamma must both be (count, 4)")
    return count, ins


def batch_pedersen_commit(v, gamma, g, h, out=None, stream=None, gens=None):
    """pedersen_commit (bulletproof_range_proof.cu:277) over a batch, on the GPU
    (hipbp_batch_pedersen_commit): out[i] = N(add(N(sm(tobytes(v[i]), g)), N(sm(tobytes(gamma[i]), h)))),
    the V batch_generate_range_proof gives where valid = 1, without its range check.

    v, gamma (count,4); g, h (16,): int64 CUDA tensors of the u64 limbs.  gens= a Generators set (any
    n): its g, h and prefix tables are used (g, h are not read and may be None); the same bits.
    out: a (count,16) int64 CUDA tensor to write (it must not overlap the inputs), or None for a new
    one.  Asynchronous on `stream`.  Returns the (count,16) tensor."""
    import contextlib

    import torch
    count, ins = _commit_args(v, gamma, g, h, gens)
    if out is None:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            out = torch.empty(count, 16, dtype=torch.int64, device=v.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (count, 16) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({count}, 16) int64 tensor")
    if gens is not None:
        _chk(lib().hipbp_batch_pedersen_commit_gens(_c(out.data_ptr()), _c(ins[0].data_ptr()), _c(ins[1].data_ptr()),
                                                    _sz(count), _c(gens.h), _stream_ptr(stream)))
    else:
        _chk(lib().hipbp_batch_pedersen_commit(_c(out.data_ptr()), _c(ins[0].data_ptr()), _c(ins[1].data_ptr()),
                                               _sz(count), _c(ins[2].data_ptr()), _c(ins[3].data_ptr()),
                                               _stream_ptr(stream)))
    return out


def batch_pedersen_open(V, v, gamma, g, h, stream=None, gens=None):
    """hipbp_batch_pedersen_open: ok[i] = 1 iff all 16 limbs of V[i] equal batch_pedersen_commit's
    commitment of (v[i], gamma[i]).  V (count,16), v, gamma (count,4), g, h (16,) int64 CUDA tensors;
    gens= as in batch_pedersen_commit.  Asynchronous on `stream`.  Returns a (count,) uint8 CUDA tensor."""
    import contextlib

    import torch
    count, ins = _commit_args(v, gamma, g, h, gens)
    V = V.contiguous()
    if V.numel() != count * 16:
        raise ValueError(f"V must be ({count}, 16)")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        ok = torch.empty(count, dtype=torch.uint8, device=v.device)
    _chk(lib().hipbp_batch_pedersen_open(_c(ok.data_ptr()), _c(V.data_ptr()), _c(ins[0].data_ptr()),
                                         _c(ins[1].data_ptr()), _sz(count),
                                         _c(ins[2].data_ptr()) if ins[2] is not None else None,
                                         _c(ins[3].data_ptr()) if ins[3] is not None else None,
                                         _c(gens.h) if gens is not None else None, _stream_ptr(stream)))
    return ok


def batch_pedersen_commit_host(v, gamma, g, h, num_gpus=1):
    """hipbp_batch_pedersen_commit_host: batch_pedersen_commit on host arrays.  v, gamma (count,4),
    g, h (16,) uint64; returns a (count,16) uint64 array with the device call's bytes.  Synchronous.
    num_gpus: the devices the batch is split over, from the current one on (1: the current device
    alone; 0: all visible); the result does not depend on it."""
    require_gpu()
    v, gamma = _u64(v, 4).reshape(-1, 4), _u64(gamma, 4).reshape(-1, 4)
    if len(v) != len(gamma):
        raise ValueError("v and gamma must have the same length")
    g, h = _u64(g, 16), _u64(h, 16)
    out = np.zeros((len(v), 16), np.uint64)
    _chk(lib().hipbp_batch_pedersen_commit_host(_p(out), _p(v), _p(gamma), _sz(len(v)), _p(g), _p(h),
                                                ctypes.c_int(num_gpus)))
    return out


# ---------------------------------------------------------------------- compact proof blobs
def _blob_info(ic):
    return dict(count=int(ic.count), n=int(ic.n), ab_len=int(ic.ab_len), L_len=int(ic.L_len), flags=int(ic.flags),
                raw_count=int(ic.raw_count), bytes=int(ic.bytes))


def _blob_arg(blob):
    """A host blob (bytes, bytearray, memoryview or a uint8 array) as a contiguous uint8 array."""
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob, np.uint8).reshape(-1)
    return np.frombuffer(bytes(blob), np.uint8)


def proof_blob_info(blob):
    """hipbp_proof_blob_parse: fully validates a host proof blob ("HBPC" version 1) and
    returns dict(count, n, ab_len, L_len, flags (bit 0: taux and mu stored), raw_count, bytes).
    Raises BulletproofError with the reason on a malformed blob.  CPU only: needs no GPU."""
    b = _blob_arg(blob)
    ic = ProofBlobInfoC()
    _chk(lib().hipbp_proof_blob_parse(_p(b), _sz(len(b)), ctypes.byref(ic)))
    return _blob_info(ic)


def proofs_to_bytes(proofs, n, with_blinding=False):
    """hipbp_proofs_encode_host: a list of proof dicts (what cuda_range_proof_verify and
    batch_range_proof_verify_host take: head (100,) = V,A,S,T1,T2 | taux,mu,t,c,x; a, b (k,4); L, R
    (m,16)) as one compact blob, returned as bytes.  A proof whose points are normalized (Z = 1, T = X Y)
    and whose a = [t], b = [1], c = t, limb for limb, takes 64 bytes per point; any other is stored
    verbatim, so proofs_from_bytes returns every limb.  with_blinding: taux and mu are stored.  The
    first proof sets the shape; a proof of another shape raises.  CPU only: needs no GPU; the bytes
    are encode_proofs'."""
    keep = []
    count = len(proofs)
    arr = (RangeProofC * max(count, 1))()
    for i, pr in enumerate(proofs):
        arr[i] = _range_proof_struct(pr, n, keep)
    abl = len(keep[0]) if count else 1
    Lr = len(keep[2]) if count else 0
    cap = lib().hipbp_proof_blob_bound(_sz(count), _sz(abl), _sz(Lr), ctypes.c_uint(1 if with_blinding else 0))
    out = np.zeros(cap, np.uint8)
    nb = _sz(0)
    _chk(lib().hipbp_proofs_encode_host(arr, _sz(count), _sz(int(n)), ctypes.c_int(1 if with_blinding else 0), _p(out),
                                        _sz(cap), ctypes.byref(nb)))
    return out[:nb.value].tobytes()


def proofs_from_bytes(blob):
    """hipbp_proofs_decode_host: the proofs of a host blob as a list of proof dicts (head, a, b, L, R,
    n, L_len; taux and mu zero when the blob does not store them), bit for bit what was encoded.
    Raises BulletproofError on a malformed blob.  CPU only: needs no GPU."""
    b = _blob_arg(blob)
    count = proof_blob_info(b)["count"]
    arr = (RangeProofC * max(count, 1))()
    _chk(lib().hipbp_proofs_decode_host(_p(b), _sz(len(b)), arr))
    return _take_proofs(arr, count)


def encode_proofs(batch, with_blinding=False, stream=None):
    """hipbp_batch_proof_encode: a RangeProofBatch as one compact blob on its device (classify, scan
    and write launches; the bytes are proofs_to_bytes').  with_blinding needs batch.taux / batch.mu.
    The V encoded is batch.Vp when present, else batch.V.  Returns a uint8 CUDA tensor trimmed to the
    written size (the call waits for the stream to read that size)."""
    import contextlib

    import torch
    f = 1 if with_blinding else 0
    cap = lib().hipbp_proof_blob_bound(_sz(batch.count), _sz(batch.ab_len), _sz(batch.L_len), ctypes.c_uint(f))
    dev = batch.V.device
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        blob = torch.empty(cap, dtype=torch.uint8, device=dev)
        nb = torch.zeros(1, dtype=torch.int64, device=dev)
    s = batch.c_struct()
    _chk(lib().hipbp_batch_proof_encode(ctypes.byref(s), ctypes.c_int(f), _c(blob.data_ptr()), _sz(cap),
                                        _c(nb.data_ptr()), _stream_ptr(stream)))
    _chk(lib().hipbp_sync(_stream_ptr(stream)))
    return blob[:int(nb.item())]


def decode_proofs(blob_tensor, stream=None):
    """hipbp_batch_proof_decode: a blob in a uint8 CUDA tensor as a RangeProofBatch on its device
    (taux / mu present when the blob stores them).  The 32 header bytes are read back and validated
    on the host (hipbp_proof_blob_header); the kernels check every index they take from the blob
    and skip what fails: a non-zero count of skipped records raises.  Waits for the stream."""
    import contextlib

    import torch
    blob_tensor = blob_tensor.contiguous()
    if blob_tensor.dtype != torch.uint8 or blob_tensor.dim() != 1:
        raise ValueError("blob_tensor must be a 1-D uint8 tensor")
    head = blob_tensor[:32].cpu().numpy()
    if len(head) < 32:
        raise BulletproofError("proof_blob_header: blob shorter than its header")
    ic = ProofBlobInfoC()
    _chk(lib().hipbp_proof_blob_header(_p(head), _sz(blob_tensor.numel()), ctypes.byref(ic)))
    B, n, abl, Lr, f = int(ic.count), int(ic.n), int(ic.ab_len), int(ic.L_len), int(ic.flags) & 1
    dev = blob_tensor.device
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
        out = dict(V=z(B, 16), A=z(B, 16), S=z(B, 16), T1=z(B, 16), T2=z(B, 16), taux=z(B, 4) if f else None,
                   mu=z(B, 4) if f else None, t=z(B, 4), c=z(B, 4), x=z(B, 4), a=z(B, abl, 4), b=z(B, abl, 4),
                   L=z(B, Lr, 16), R=z(B, Lr, 16), valid=None)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    oc = ProofOutC(*[out[k].data_ptr() if out[k] is not None and out[k].numel() else None for k in _PROOF_KEYS])
    _chk(lib().hipbp_batch_proof_decode(_c(blob_tensor.data_ptr()), ctypes.byref(ic), ctypes.byref(oc),
                                        _c(bad.data_ptr()), _stream_ptr(stream)))
    _chk(lib().hipbp_sync(_stream_ptr(stream)))
    if int(bad.item()):
        raise BulletproofError(f"decode_proofs: {int(bad.item())} record(s) failed their checks and were skipped")
    del out["valid"]
    return RangeProofBatch(n, **out)


# ---------------------------------------------------------------------- proof ids and the batch Merkle root
def proof_ids(batch, with_blinding=False, stream=None, return_kinds=False):
    """hipbp_batch_proof_ids: the id of every proof of a RangeProofBatch, on its device: a (B, 32) uint8
    CUDA tensor (SHA-256 of a 32-byte header and the record the compact blob stores for
    the proof).  with_blinding needs batch.taux / batch.mu and gives other ids.  return_kinds: also
    the (B,) uint8 kinds (0 compact, 1 raw).  Asynchronous on `stream`."""
    import contextlib

    import torch
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        ids = torch.empty(batch.count, 32, dtype=torch.uint8, device=batch.V.device)
        kinds = torch.empty(batch.count, dtype=torch.uint8, device=batch.V.device) if return_kinds else None
    s = batch.c_struct()
    _chk(lib().hipbp_batch_proof_ids(ctypes.byref(s), ctypes.c_int(1 if with_blinding else 0), _c(ids.data_ptr()),
                                     _c(kinds.data_ptr()) if return_kinds else None, _stream_ptr(stream)))
    return (ids, kinds) if return_kinds else ids


def blob_proof_ids(blob_tensor, stream=None):
    """hipbp_blob_proof_ids: the ids of the proofs of a blob in a uint8 CUDA tensor -> (ids (B, 32)
    uint8, bad), both on its device.  The 32 header bytes are read back and validated on the host; the
    kernel checks every index it takes from the blob: a record that fails has an all-zero id and is
    counted in bad (a 1-element int32 tensor; 0 for a well-formed blob).  Asynchronous on `stream`
    after the header's read-back."""
    import contextlib

    import torch
    blob_tensor = blob_tensor.contiguous()
    if blob_tensor.dtype != torch.uint8 or blob_tensor.dim() != 1:
        raise ValueError("blob_tensor must be a 1-D uint8 tensor")
    head = blob_tensor[:32].cpu().numpy()
    if len(head) < 32:
        raise BulletproofError("proof_blob_header: blob shorter than its header")
    ic = ProofBlobInfoC()
    _chk(lib().hipbp_proof_blob_header(_p(head), _sz(blob_tensor.numel()), ctypes.byref(ic)))
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        ids = torch.empty(int(ic.count), 32, dtype=torch.uint8, device=blob_tensor.device)
        bad = torch.zeros(1, dtype=torch.int32, device=blob_tensor.device)
    _chk(lib().hipbp_blob_proof_ids(_c(blob_tensor.data_ptr()), ctypes.byref(ic), _c(ids.data_ptr()), _c(bad.data_ptr()),
                                    _stream_ptr(stream)))
    return ids, bad


def merkle_root(ids, stream=None):
    """hipbp_merkle_root: the RFC 6962 Merkle root over a (B, 32) uint8 CUDA tensor of ids (the ids are
    the leaf inputs; B = 0: SHA-256 of the empty string) -> a (32,) uint8 tensor on its device.
    Asynchronous on `stream`."""
    import contextlib

    import torch
    ids = ids.contiguous()
    if ids.dtype != torch.uint8 or ids.dim() != 2 or ids.shape[1] != 32:
        raise ValueError("ids must be a (B, 32) uint8 tensor")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        root = torch.empty(32, dtype=torch.uint8, device=ids.device)
    _chk(lib().hipbp_merkle_root(_c(ids.data_ptr()) if ids.shape[0] else None, _sz(ids.shape[0]), _c(root.data_ptr()),
                                 _stream_ptr(stream)))
    return root


def _ids_arg(ids):
    """A list of 32-byte ids, or a (B, 32) uint8 array, as a contiguous (B, 32) uint8 array."""
    if isinstance(ids, np.ndarray):
        a = np.ascontiguousarray(ids, np.uint8)
    else:
        ids = [bytes(i) for i in ids]
        if any(len(i) != 32 for i in ids):
            raise ValueError("an id is 32 bytes")
        a = np.frombuffer(b"".join(ids), np.uint8)
    return a.reshape(-1, 32)


def _ids_list(a, count):
    return [a[32 * i:32 * i + 32].tobytes() for i in range(count)]


def proof_ids_host(proofs, n, with_blinding=False):
    """hipbp_proof_ids_host: the ids of a list of proof dicts (what proofs_to_bytes takes), as a list of
    32-byte `bytes`: proof_ids' bytes.  CPU only: needs no GPU."""
    keep = []
    count = len(proofs)
    arr = (RangeProofC * max(count, 1))()
    for i, pr in enumerate(proofs):
        arr[i] = _range_proof_struct(pr, n, keep)
    out = np.zeros(32 * max(count, 1), np.uint8)
    _chk(lib().hipbp_proof_ids_host(arr, _sz(count), _sz(int(n)), ctypes.c_int(1 if with_blinding else 0), _p(out)))
    return _ids_list(out, count)


def blob_proof_ids_host(blob):
    """hipbp_blob_proof_ids_host: the ids of the proofs of a host blob (fully parsed first; a malformed
    one raises BulletproofError), as a list of 32-byte `bytes`.  CPU only: needs no GPU."""
    b = _blob_arg(blob)
    count = proof_blob_info(b)["count"]
    out = np.zeros(32 * max(count, 1), np.uint8)
    _chk(lib().hipbp_blob_proof_ids_host(_p(b), _sz(len(b)), _p(out)))
    return _ids_list(out, count)


def merkle_root_host(ids):
    """hipbp_merkle_root_host: the Merkle root over the ids (a list of 32-byte ids or a (B, 32) uint8
    array) as 32 `bytes`.  CPU only."""
    a = _ids_arg(ids)
    root = np.zeros(32, np.uint8)
    _chk(lib().hipbp_merkle_root_host(_p(a) if len(a) else None, _sz(len(a)), _p(root)))
    return root.tobytes()


def merkle_path(ids, index):
    """hipbp_merkle_path_host: the RFC 6962 audit path of ids[index], bottom-up, as a list of 32-byte
    `bytes`.  CPU only."""
    a = _ids_arg(ids)
    path = np.zeros(32 * 22, np.uint8)
    n = _sz(0)
    _chk(lib().hipbp_merkle_path_host(_p(a) if len(a) else None, _sz(len(a)), _sz(int(index)), _p(path), ctypes.byref(n)))
    return _ids_list(path, n.value)


def merkle_verify(id, index, count, path, root):
    """hipbp_merkle_verify_host: True when (id, index, count, path) recomputes `root`, consuming exactly
    the path's entries.  CPU only."""
    i, r = _ids_arg([id]), _ids_arg([root])
    p = _ids_arg(path)
    if index < 0 or count < 0:
        return False
    return bool(lib().hipbp_merkle_verify_host(_p(i), _sz(int(index)), _sz(int(count)), _p(p) if len(p) else None,
                                               _sz(len(p)), _p(r)))


def batch_range_proof_verify_bytes_host(blob, n, G, H, g, h, V=None, check=1, num_gpus=1):
    """hipbp_batch_range_proof_verify_bytes_host: verifies the proofs of a host blob on the GPU(s),
    uploading the blob's bytes (about half the structs').  check 1: cuda_range_proof_verify
    semantics, the verdicts of batch_range_proof_verify_host on proofs_from_bytes(blob); check 2:
    range_proof_verify semantics (batch_range_proof_verify_std's verdicts; the blob must store taux
    and mu).  V (count,16): the verify's V argument; None: each proof's own V.  G, H (n,16), g, h
    (16,) uint64.  num_gpus as in batch_range_proof_verify_host.  Returns (count,) bool."""
    require_gpu()
    b = _blob_arg(blob)
    count = proof_blob_info(b)["count"]
    g, h = _u64(g, 16), _u64(h, 16)
    G, H = _u64(G, 16), _u64(H, 16)
    if V is not None:
        V = _u64(V, 16).reshape(-1, 16)
        if len(V) != count:
            raise ValueError(f"V must be ({count}, 16)")
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    ok = np.zeros(max(count, 1), np.uint8)
    _chk(lib().hipbp_batch_range_proof_verify_bytes_host(_p(b), _sz(len(b)), _p(V) if V is not None else None,
                                                         _sz(int(n)), ctypes.byref(gv), ctypes.byref(hv), _p(g), _p(h),
                                                         ctypes.c_int(check), ctypes.c_int(num_gpus), _p(ok)))
    return ok[:count].astype(bool)


def batch_inner_product_prove(n, a, b, c, G, H, Q, transcript=None, stream=None, gens=None):
    """inner_product_prove (bulletproof_vectors.cu:277) over a batch, on the GPU, for any power-of-two
    n up to 65536 (hipbp_batch_inner_product_prove).

    a, b (B,n,4); c (B,4) the claimed inner products; transcript (B,4) the 32 initial transcript bytes
    as LE limbs (None: zeros); G, H (n,16), Q (16,): int64 CUDA tensors of the u64 limbs.  With
    gens= a Generators set, its G, H and prefix tables are used and Q is its h (G, H, Q are not
    read); the bits are the same.  Returns a dict of CUDA tensors: a, b (B,1,4), c, c_final, x (B,4),
    L, R (B,log2 n,16); c is the claimed value as given, c_final = add(0, mul(a, b)) of the final a, b,
    the value with which the reference's verifier accepts.  ipa_proof_batch() makes it verifiable."""
    import contextlib

    import torch
    B = int(a.shape[0])
    Lr = int(n).bit_length() - 1
    dev = a.device
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        z = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
        out = dict(a=z(B, 1, 4), b=z(B, 1, 4), c=z(B, 4), x=z(B, 4), c_final=z(B, 4), L=z(B, max(Lr, 0), 16),
                   R=z(B, max(Lr, 0), 16))
    ins = [t.contiguous() for t in (a, b, c)] + [transcript.contiguous() if transcript is not None else None]
    if ins[0].numel() != B * int(n) * 4 or ins[1].numel() != B * int(n) * 4 or ins[2].numel() != B * 4:
        raise BulletproofError("batch_inner_product_prove: a, b must be (B, n, 4) and c (B, 4)")
    ic = ProveIpaInputC(B, int(n), *[t.data_ptr() if t is not None else None for t in ins])
    oc = IpaProofOutC(*[out[k].data_ptr() if out[k].numel() else None for k in ("a", "b", "c", "x", "c_final", "L", "R")])
    if gens is not None:
        _chk(lib().hipbp_batch_inner_product_prove_gens(ctypes.byref(ic), _c(gens.h), ctypes.byref(oc),
                                                        _stream_ptr(stream)))
    else:
        _chk(lib().hipbp_batch_inner_product_prove(ctypes.byref(ic), _c(G.data_ptr()), _c(H.data_ptr()),
                                                   _c(Q.data_ptr()), ctypes.byref(oc), _stream_ptr(stream)))
    out["_keep"] = ins
    return out


def ipa_proof_batch(n, proof, c="c_final"):
    """A batch_inner_product_prove result as a RangeProofBatch for batch_inner_product_verify (zero
    V, A, S, T1, T2, t, which the inner-product check does not read).  c: "c_final" (the value the
    reference's verifier accepts with) or "c" (the claimed value as given)."""
    import torch
    if c not in ("c", "c_final"):
        raise ValueError("c must be 'c' or 'c_final'")
    B, dev = int(proof["a"].shape[0]), proof["a"].device
    zp = torch.zeros(B, 16, dtype=torch.int64, device=dev)
    return RangeProofBatch(n, V=zp, A=zp, S=zp, T1=zp, T2=zp, t=torch.zeros(B, 4, dtype=torch.int64, device=dev),
                           a=proof["a"], b=proof["b"], c=proof[c], x=proof["x"], L=proof["L"], R=proof["R"])


def inner_product_prove(a, b, G, H, Q, c, transcript=None):
    """inner_product_prove on host arrays through hipbp_inner_product_prove_host (the reference's own
    structs): a, b (n,4), G, H (n,16), Q (16,), c (4,) uint64; transcript 32 bytes (None: zeros).
    Returns dict(a, b (1,4), c, x (4,), L, R (log2 n,16)), or None where the reference's function
    returns early (length mismatch, n no power of two)."""
    require_gpu()
    a, b, G, H = _u64(a, 4), _u64(b, 4), _u64(G, 16), _u64(H, 16)
    Q, c = _u64(Q, 16), _u64(c, 4)
    tr = np.zeros(32, np.uint8) if transcript is None else np.ascontiguousarray(transcript, np.uint8)
    pr = InnerProductProof()
    av, bv = FieldVector(_p(a).value, len(a)), FieldVector(_p(b).value, len(b))
    gv, hv = PointVector(_p(G).value, len(G)), PointVector(_p(H).value, len(H))
    rc = lib().hipbp_inner_product_prove_host(ctypes.byref(pr), ctypes.byref(av), ctypes.byref(bv), ctypes.byref(gv),
                                              ctypes.byref(hv), _p(Q), _p(c), _p(tr))
    if rc != 0:
        if not pr.a.elements and rc == 1:
            return None
        _chk(rc)
    return dict(a=_take(pr.a, 4), b=_take(pr.b, 4), c=np.array(pr.c, np.uint64), x=np.array(pr.x, np.uint64),
                L=_take(pr.L, 16), R=_take(pr.R, 16), L_len=int(pr.L_len), n=int(pr.n))


def msm(result, scalars, points, stream=None):
    """Canonical-tree MSM on CUDA tensors: result (16,), scalars (n,4), points (n,16)."""
    _chk(lib().hipbp_msm(_c(result.data_ptr()), _c(scalars.data_ptr()), _c(points.data_ptr()),
                         _sz(points.shape[0]), _stream_ptr(stream)))


def msm_batch(results, scalars, points, stream=None):
    """count canonical-tree MSMs over the same points: results (count,16), scalars (count*n,4) or
    (count,n,4), points (n,16); CUDA tensors."""
    n = points.shape[0]
    count = results.shape[0]
    if scalars.numel() != count * n * 4:
        raise BulletproofError("msm_batch: scalars must hold count * n rows")
    _chk(lib().hipbp_msm_batch(_c(results.data_ptr()), _c(scalars.data_ptr()), _c(points.data_ptr()), _sz(n),
                               _sz(count), _stream_ptr(stream)))


def msm_batch_gens(results, scalars, gens, stream=None):
    """msm_batch over a Generators set's G||H (2n points) with its prefix tables: results (count,16),
    scalars (count*2n,4); the same bits as msm_batch(results, scalars, cat(G, H))."""
    count, n2 = results.shape[0], 2 * gens.n
    if scalars.numel() != count * n2 * 4:
        raise BulletproofError("msm_batch_gens: scalars must hold count * 2n rows")
    _chk(lib().hipbp_msm_batch_gens(_c(results.data_ptr()), _c(scalars.data_ptr()), _c(gens.h), _sz(count),
                                    _stream_ptr(stream)))


def msm_pippenger(result, scalars, points, window_bits=12, stream=None):
    """Pippenger bucket MSM on CUDA tensors (labelled alternative: not the reference's MSM bits,
    see include/cudabulletproof_hip.h)."""
    _chk(lib().hipbp_msm_pippenger(_c(result.data_ptr()), _c(scalars.data_ptr()), _c(points.data_ptr()),
                                   _sz(points.shape[0]), ctypes.c_int(window_bits), _stream_ptr(stream)))


def msm_pippenger_batch(results, scalars, points, window_bits=12, stream=None):
    """count Pippenger MSMs over the same points: results (count,16), scalars (count*n,4) or
    (count,n,4), points (n,16), device tensors."""
    count, n = results.shape[0], points.shape[0]
    if scalars.numel() != count * n * 4:
        raise BulletproofError("msm_pippenger_batch: scalars must hold count * n rows")
    _chk(lib().hipbp_msm_pippenger_batch(_c(results.data_ptr()), _c(scalars.data_ptr()), _c(points.data_ptr()),
                                         _sz(n), _sz(count), ctypes.c_int(window_bits), _stream_ptr(stream)))


def pippenger_num_windows(window_bits=12):
    return (256 + int(window_bits) - 1) // int(window_bits)


def msm_pippenger_windows(window_sums, scalars, points, w_begin, w_end, window_bits=12, stream=None):
    """Window sums S_w, w in [w_begin, w_end), of the Pippenger MSM into window_sums[w] (a (W,16)
    device tensor, W = pippenger_num_windows; other rows untouched)."""
    W = pippenger_num_windows(window_bits)
    if window_sums.numel() != W * 16:
        raise BulletproofError(f"msm_pippenger_windows: window_sums must be ({W}, 16)")
    if scalars.numel() != points.shape[0] * 4:
        raise BulletproofError("msm_pippenger_windows: one scalar per point")
    _chk(lib().hipbp_msm_pippenger_windows(_c(window_sums.data_ptr()), _c(scalars.data_ptr()),
                                           _c(points.data_ptr()), _sz(points.shape[0]), ctypes.c_int(window_bits),
                                           ctypes.c_int(w_begin), ctypes.c_int(w_end), _stream_ptr(stream)))


def msm_pippenger_horner(results, window_sums, window_bits=12, stream=None):
    """Horner over all W window sums: results (count,16) or (16,), window_sums (count*W,16)."""
    W = pippenger_num_windows(window_bits)
    count = results.numel() // 16
    if window_sums.numel() != count * W * 16:
        raise BulletproofError(f"msm_pippenger_horner: window_sums must hold count * {W} rows")
    _chk(lib().hipbp_msm_pippenger_horner(_c(results.data_ptr()), _c(window_sums.data_ptr()), _sz(count),
                                          ctypes.c_int(window_bits), _stream_ptr(stream)))


def release_stream_workspaces(stream=None):
    """hipbp_release_stream_workspaces: free every workspace cached for `stream` on the current
    device (MSM, prover, commitments, blob encoder, one-shot pipelines, Pippenger pair); call before dropping a stream."""
    _chk(lib().hipbp_release_stream_workspaces(_stream_ptr(stream)))


def point_tree(result, points, stream=None):
    """Canonical tree over device points (the MSM's reduction half): result (16,), points (n,16)."""
    _chk(lib().hipbp_point_tree(_c(result.data_ptr()), _c(points.data_ptr()), _sz(points.shape[0]),
                                _stream_ptr(stream)))


def field_op(op, r, a, b=None, stream=None):
    ops = {"add": 0, "sub": 1, "mul": 2, "square": 3, "soa_add": 4, "invert": 5, "fold": 6, "sq": 7,
           "addsub_add": 8, "addsub_sub": 9,   # 8/9: the fused add/sub block's sum / difference
           "mul_q4": 10,   # 10: fe25519_mul as the drain forms' quad-split product (fe_mul_q4)
           "mul_k": 11,    # 11: fe25519_mul(a, k), the point operations' product by the constant (fe_mul_k)
           "mul_q4_k": 12,   # 12: the same split over a lane quad (fe_mul_q4_k, the drain forms' C)
           # the row step's latency forms (13, 15/16, 19) and deferred rare-edge forms (14, 17/18, 20)
           "add_lat": 13, "add_defer": 14, "addsub_lat_add": 15, "addsub_lat_sub": 16,
           "addsub_defer_add": 17, "addsub_defer_sub": 18, "fold_lat": 19, "fold_defer": 20,
           # the lane loops' deferred forms (ge25519_dev.h), recomputed per element on an edge or a failed gate
           "add_acc": 21, "addsub_acc_add": 22, "addsub_acc_sub": 23, "fold_acc": 24, "mul_acc": 25, "sq_acc": 26,
           "sub_acc": 27}
    _chk(lib().hipbp_field_op(ops[op], _c(r.data_ptr()), _c(a.data_ptr()), _c(b.data_ptr()) if b is not None else None,
                              _sz(a.shape[0]), _stream_ptr(stream)))


def sm_probe(force, out, scalars, points, stream=None):
    """hipbp_sm_probe: out[i] (N, 16) = scalarmult(scalars[i] (N, 4), points[i] (N, 16)), raw extended
    points; force: through the deferred pass's recovery path (the same bits)."""
    _chk(lib().hipbp_sm_probe(int(bool(force)), _c(out.data_ptr()), _c(scalars.data_ptr()), _c(points.data_ptr()),
                              _sz(scalars.shape[0]), _stream_ptr(stream)))


def sm_form_probe(form, force, out, scalars, points, stream=None):
    """hipbp_sm_form_probe: the same through the drain-tick forms, form 1 lane quads (sm_quad), 2 lane pairs
    (sm_pair), 3 16-lane rows (sm_row); force = 1 (form 3 only): every step through the row step's deferred
    recompute (the same bits).  form and force go to the library as given: it refuses any other value."""
    _chk(lib().hipbp_sm_form_probe(ctypes.c_int(int(form)), ctypes.c_int(int(force)), _c(out.data_ptr()),
                                   _c(scalars.data_ptr()), _c(points.data_ptr()), _sz(scalars.shape[0]),
                                   _stream_ptr(stream)))


def sha_probe(kind, out, inp, stream=None):
    """hipbp_sha_probe: the verify path's SHA-256 message shapes on the device (kind 0 y, 1 z, 2 x,
    3 inner-product round, 4 prover IPA start, 5 raw digest of four values); inp (N, 6, 4), out (N, 4)."""
    _chk(lib().hipbp_sha_probe(int(kind), _c(out.data_ptr()), _c(inp.data_ptr()), _sz(inp.shape[0]),
                               _stream_ptr(stream)))


# ====================================================================== per-kernel timing
def timing_enable(on=True):
    """Record HIP events around each verify-pipeline kernel launch (resets the totals)."""
    L = lib()
    L.hipbp_timing_enable.restype = ctypes.c_int
    _chk(L.hipbp_timing_enable(1 if on else 0))


def timing_collect():
    """{kernel_name: (total_ms, launches)} accumulated since timing_enable()."""
    L = lib()
    L.hipbp_kernel_name.restype = ctypes.c_char_p
    L.hipbp_timing_collect.restype = ctypes.c_int
    k = L.hipbp_kernel_count()
    ms = (ctypes.c_double * k)()
    cnt = (ctypes.c_uint64 * k)()
    _chk(L.hipbp_timing_collect(ms, cnt))
    return {L.hipbp_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(k)}


# ====================================================================== streaming verify pipeline
class VerifyPipeline:
    """hipbp_pipeline_*: up to `depth` batches in flight; each push runs one tick in which
    every in-flight batch advances one stage (stage 0 / fold round r / final).  A batch's
    outputs are complete after depth-1 further pushes or flush()."""

    def __init__(self, max_batch, n, G, H, h, range_mode=True, stream=None, g=None):
        """range_mode: True/1 cuda_range_proof_verify, 2 range_proof_verify (needs g), False/0
        cuda_inner_product_verify (h = Q)."""
        L = lib()
        L.hipbp_pipeline_create.restype = ctypes.c_void_p
        L.hipbp_pipeline_push.restype = ctypes.c_int
        L.hipbp_pipeline_flush.restype = ctypes.c_int
        L.hipbp_pipeline_depth.restype = ctypes.c_int
        self._keep = (G, H, h, g)
        self.stream = stream   # the torch stream the ticks run on (None: the null stream)
        self.mode = int(range_mode)
        self.h = L.hipbp_pipeline_create(_sz(max_batch), _sz(n), self.mode, _c(G.data_ptr()), _c(H.data_ptr()),
                                         _c(g.data_ptr()) if g is not None else None, _c(h.data_ptr()),
                                         _stream_ptr(stream))
        if not self.h:
            raise BulletproofError(L.hipbp_last_error().decode())
        self.depth = L.hipbp_pipeline_depth(_c(self.h))

    def push(self, batch, ok=None, P_out=None, check_out=None, P_in=None, flags_out=None, poly_out=None):
        s = batch.c_struct() if batch is not None else None
        opt = lambda t: _c(t.data_ptr()) if t is not None else None
        _chk(lib().hipbp_pipeline_push(
            _c(self.h), ctypes.byref(s) if s is not None else None, opt(P_in), opt(ok), opt(P_out), opt(check_out),
            opt(flags_out), opt(poly_out)))

    def flush(self):
        _chk(lib().hipbp_pipeline_flush(_c(self.h)))

    def use_gens(self, gens):
        """hipbp_pipeline_use_gens: generators and prefix tables from a Generators set."""
        _chk(lib().hipbp_pipeline_use_gens(_c(self.h), _c(gens.h)))
        self._gens = gens

    def defer_msm(self, on=True):
        """hipbp_pipeline_defer_msm: split stage 0 for the batches pushed from now on (the MSM
        terms, t*h and c*Q as RK_MSMT chunks inside the batch's fold-round ticks, stages 2 .. L, on
        the pipeline's own stream; the lane trees at the final-terms tick); same bits.  Raises
        BulletproofError where the split does not apply (inner-product mode, n above the lane-tree
        limit, n > 512)."""
        _chk(lib().hipbp_pipeline_defer_msm(_c(self.h), ctypes.c_int(1 if on else 0)))

    def prefix_tables(self, bits):
        """hipbp_pipeline_prefix_tables: fixed-base prefix tables of the generators (same bits,
        fewer point operations); bits = 0 frees them.  Synchronous; the pipeline must be idle."""
        _chk(lib().hipbp_pipeline_prefix_tables(_c(self.h), ctypes.c_int(int(bits))))

    def close(self):
        if self.h:
            lib().hipbp_pipeline_destroy(_c(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

// bp_commit.hip — gfx950 kernels for the reference's pedersen_commit
// (bulletproof_range_proof.cu:277-296) over a batch, bit-exact:
//   out[i] = N(add(N(sm(tobytes(v[i]), g)), N(sm(tobytes(gamma[i]), h))))
// with N the host ge25519_normalize, sm ge25519_scalarmult over all 256 bits and tobytes the host,
// canonicalising fe25519_tobytes: the V that k_prove_terms0 / k_prove_commit form inside a proof, for
// any four limbs (there is no validate_range_input here) and any g, h as given.
//
// One chunk of c commitments:
//   k_commit_sort_*   lane/term        each class's lanes into chain-length order (chunks >= 4096; HIPBP_COMMIT_SORT)
//   k_commit_terms    lane/term        the 2c scalar multiplications, host-normalized, into ws.terms
//   k_commit_combine  lane/commitment  N(add(t_v, t_gamma)) into out, or (open form) compared with V[i]
//
// Grid of k_commit_terms: the two classes have very different chains (a blinding term is ~255
// doublings + popcount adds, the value term of a 64-bit amount about a quarter of that, its >= 192
// leading zeros being one dtab lookup), and a wave runs as long as its longest lane.  So the lanes
// are laid out class by class, each class padded to a whole wave: lanes [0, P) the blinding terms,
// [P, 2P) the value terms, P = c rounded up to 64 (the long class first: the short one fills the
// launch's tail).  A wave never mixes the classes, and its base point and table row are uniform.
// Within a class the sort puts the longest chains first, so the lanes of a wave end together: measured
// at 2^20 commitments, +4.8 % for uniform 64-bit values and +11.7 % for values of log-uniform
// magnitude, against a 0.4 % spread of the unsorted runs (profiles/ab/r13a_commit_sort.json).
//
// There are no latency forms (row, quad, pair) here.  One commitment is a full scalar-mult chain at a
// lone wave's issue rate, whatever form runs it (1.5 ms measured), and the CPU restatement of the
// reference's function takes 0.21 ms on one core: for a handful of commitments the CPU wins, and this
// path is for batches.  tools/bench_commit.py records where the device call overtakes count x one CPU
// commitment: at 8 (profiles/bench/commit_p01.json).
#include "bp_kernels.h"
#include "ge25519_dev.h"

namespace bp {

namespace {
constexpr int TPB = 256;
__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline unsigned nblk(size_t items) { return (unsigned)((items + TPB - 1) / TPB); }
}  // namespace

// term j of a class in tobytes form (val: the value term's, else the blinding term's scalar)
__device__ __forceinline__ fe commit_scalar(const CommitIn& in, bool val, size_t j) {
    return fe_canon(val ? in.v[j] : in.gamma[j]);
}

// ---------------------------------------------------------------- chain-length sort (HIPBP_COMMIT_SORT)
// Within each class the lanes take the terms longest chain first: a counting sort over sm_ops_prefix
// (k_prove_sort_hist / k_prove_sort_scatter's scheme), both classes in one launch, a block of SORT_T
// lanes belonging to one class (blocks [0, nb) the blinding terms, [nb, 2 nb) the value terms).
constexpr int SORT_T = 256;
inline unsigned sort_blocks(size_t c) { return (unsigned)((c + SORT_T - 1) / SORT_T); }

__global__ __launch_bounds__(SORT_T) void k_commit_sort_hist(CommitIn in, CommitWs ws, unsigned nb) {
    __shared__ unsigned hb[MSM_BINS];
    for (int k = threadIdx.x; k < MSM_BINS; k += SORT_T) hb[k] = 0;
    __syncthreads();
    const bool val = blockIdx.x >= nb;
    const size_t j = (size_t)(blockIdx.x - (val ? nb : 0)) * SORT_T + threadIdx.x;
    if (j < in.count) atomicAdd(&hb[sm_ops_prefix(commit_scalar(in, val, j), in.ptab ? in.pbits : 0)], 1u);
    __syncthreads();
    unsigned* bins = ws.bins + (val ? MSM_BINS : 0);
    for (int k = threadIdx.x; k < MSM_BINS; k += SORT_T)
        if (hb[k]) atomicAdd(&bins[k], hb[k]);
}

__global__ __launch_bounds__(SORT_T) void k_commit_sort_scatter(CommitIn in, CommitWs ws, unsigned nb) {
    __shared__ unsigned cnt[MSM_BINS], base[MSM_BINS];
    for (int k = threadIdx.x; k < MSM_BINS; k += SORT_T) cnt[k] = 0;
    __syncthreads();
    const bool val = blockIdx.x >= nb;
    const size_t j = (size_t)(blockIdx.x - (val ? nb : 0)) * SORT_T + threadIdx.x;
    int key = 0;
    unsigned rank = 0;
    const bool live = j < in.count;
    if (live) {
        key = sm_ops_prefix(commit_scalar(in, val, j), in.ptab ? in.pbits : 0);
        rank = atomicAdd(&cnt[key], 1u);
    }
    __syncthreads();
    unsigned* bins = ws.bins + (val ? MSM_BINS : 0);   // start offsets within the class (launch_ops_scan)
    for (int k = threadIdx.x; k < MSM_BINS; k += SORT_T)
        if (cnt[k]) base[k] = atomicAdd(&bins[k], cnt[k]);
    __syncthreads();
    if (live) ws.order[(val ? in.count : 0) + base[key] + rank] = (uint32_t)j;
}

// ---------------------------------------------------------------- the terms
// k_prove_terms0's set-up: TPB lanes, one LDS q slot per lane, three blocks per CU.
__global__ __launch_bounds__(TPB, 3) void k_commit_terms(CommitIn in, CommitWs ws, const ge* __restrict__ dtab) {
    __shared__ geq qs[TPB];
    const size_t c = in.count;
    bool lane_val;
    size_t j = commit_lane_item(c, gid(), lane_val);
    // the class is the same in every lane of a wave (a class's lanes are whole waves)
    const bool val = __builtin_amdgcn_readfirstlane((uint32_t)lane_val) != 0;
    if (j == SIZE_MAX) return;
    if (ws.order) j = ws.order[(val ? c : 0) + j];
    // operands are selected per wave and ONE scalar-mult follows (k_prove_terms0): two call sites
    // would run both loops back to back
    const fe s = commit_scalar(in, val, j);
    const ge B = val ? *in.g : *in.h;
    // prefix-table rows of a generator set: 2n (h), 2n + 1 (g)
    const ge* pt = in.ptab ? in.ptab + ((size_t)(2 * in.n + (val ? 1 : 0)) << in.pbits) : nullptr;
    const ge r = scalarmult<true>(s, B, &qs[threadIdx.x], dtab, pt, pt ? in.pbits : 0);
    ws.terms[(val ? 0 : c) + j] = ge_norm_host(r);
}

// OPEN: ok[i] = 1 iff all 16 limbs of V[i] equal the commitment; out is not written.
template <bool OPEN>
__global__ __launch_bounds__(TPB) void k_commit_combine(CommitIn in, CommitWs ws, ge* __restrict__ out,
                                                        const ge* __restrict__ V, uint8_t* __restrict__ ok) {
    const size_t c = in.count, i = gid();
    if (i >= c) return;
    const ge r = ge_norm_host(ge_add(ws.terms[i], ws.terms[c + i]));   // pedersen_commit (rp.cu:293-296)
    if (!OPEN) {
        out[i] = r;
        return;
    }
    const ge w = V[i];
    uint64_t d = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        d |= (r.X.v[k] ^ w.X.v[k]) | (r.Y.v[k] ^ w.Y.v[k]) | (r.Z.v[k] ^ w.Z.v[k]) | (r.T.v[k] ^ w.T.v[k]);
    ok[i] = d == 0 ? 1 : 0;
}

void launch_commit(const CommitIn& in, const CommitWs& ws, ge* out, const ge* V, uint8_t* ok, const ge* dtab,
                   hipStream_t s) {
    const size_t c = in.count;
    if (ws.order) {   // both classes' lanes into chain-length order, longest first
        const unsigned nb = sort_blocks(c);
        (void)hipMemsetAsync(ws.bins, 0, 2 * MSM_BINS * sizeof(unsigned), s);
        k_commit_sort_hist<<<2 * nb, SORT_T, 0, s>>>(in, ws, nb);
        launch_ops_scan(ws.bins, 1, s);
        launch_ops_scan(ws.bins + MSM_BINS, 1, s);
        k_commit_sort_scatter<<<2 * nb, SORT_T, 0, s>>>(in, ws, nb);
    }
    k_commit_terms<<<nblk(2 * commit_class_lanes(c)), TPB, 0, s>>>(in, ws, dtab);
    if (V) k_commit_combine<true><<<nblk(c), TPB, 0, s>>>(in, ws, nullptr, V, ok);
    else k_commit_combine<false><<<nblk(c), TPB, 0, s>>>(in, ws, out, nullptr, nullptr);
}

}  // namespace bp

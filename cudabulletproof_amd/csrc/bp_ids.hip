// bp_ids.hip — the kernels of the proof ids and the batch Merkle root (bp_ids.h has the messages and
// every lane body).  Plain C++: one lane per proof or per tree node, 256-lane blocks,
// exact grids, no atomics; the hash state and block of a lane stay in registers.  Nothing depends on
// timing: a lane writes only its own 32 bytes, and the failed records of a blob are counted per
// block and summed by one block.
#include <hip/hip_runtime.h>

#include "bp_ids.h"

namespace bp {

namespace {

constexpr int TPB = IDS_BLK;

__global__ __launch_bounds__(TPB) void k_proof_ids(CodecArrays A, CodecLayout l, size_t n, uint8_t* ids, uint8_t* kind) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= l.count) return;
    const uint8_t k = ids_flat_proof(A, l, n, i, ids + ID_BYTES * i);
    if (kind) kind[i] = k;
}

// blk[block] = the block's records that failed their checks
__global__ __launch_bounds__(TPB) void k_blob_ids(BlobView v, CodecLayout l, size_t n, uint8_t* ids, uint32_t* blk) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    const unsigned bad = i < v.count ? ids_blob_proof(v, l, n, i, ids + ID_BYTES * i) : 0;
    const int c = __syncthreads_count((int)bad);
    if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)c;
}

// *out = blk[0] + ... + blk[nb - 1].  One block.
__global__ __launch_bounds__(TPB) void k_ids_sum(const uint32_t* blk, uint32_t nb, uint32_t* out) {
    __shared__ uint32_t s[TPB];
    const uint32_t t = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t i = t; i < nb; i += TPB) sum += blk[i];
    s[t] = sum;
    __syncthreads();
    for (int d = TPB / 2; d > 0; d >>= 1) {
        if (t < (uint32_t)d) s[t] += s[t + d];
        __syncthreads();
    }
    if (t == 0) *out = s[0];
}

// one lane per node of the level above the m nodes (LEAF: ids) at `in`
template <bool LEAF>
__global__ __launch_bounds__(TPB) void k_merkle_level(const uint8_t* in, size_t m, uint8_t* out) {
    const size_t k = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= merkle_up(m)) return;
    merkle_level_node<LEAF>(in, m, k, out);
}

__global__ __launch_bounds__(64) void k_merkle_empty(uint8_t* root) {
    if (threadIdx.x) return;
    uint32_t d[8];
    merkle_empty(d);
    ids_store(root, d);
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + TPB - 1) / TPB); }

}  // namespace

void launch_proof_ids(const CodecArrays& A, const CodecLayout& l, size_t n, uint8_t* ids, uint8_t* kind, hipStream_t s) {
    if (l.count) hipLaunchKernelGGL(k_proof_ids, dim3(blocks(l.count)), dim3(TPB), 0, s, A, l, n, ids, kind);
}

void launch_blob_ids(const BlobView& v, const CodecLayout& l, size_t n, uint8_t* ids, const IdsWs& w, uint32_t* bad,
                     hipStream_t s) {
    const unsigned nb = blocks(v.count);
    if (nb) hipLaunchKernelGGL(k_blob_ids, dim3(nb), dim3(TPB), 0, s, v, l, n, ids, w.bad);
    hipLaunchKernelGGL(k_ids_sum, dim3(1), dim3(TPB), 0, s, w.bad, nb, bad);
}

void launch_merkle_root(const uint8_t* ids, size_t count, uint8_t* root, const IdsWs& w, hipStream_t s) {
    if (count == 0) {
        hipLaunchKernelGGL(k_merkle_empty, dim3(1), dim3(64), 0, s, root);
        return;
    }
    // level 1 from the ids (count = 1: the leaf hash is the root), then level by level; the last one
    // goes to root itself
    size_t m = merkle_up(count);
    uint8_t* bufs[2] = {w.ping, w.pong};
    int cur = 0;
    uint8_t* out = m == 1 ? root : bufs[cur];
    hipLaunchKernelGGL(k_merkle_level<true>, dim3(blocks(m)), dim3(TPB), 0, s, ids, count, out);
    while (m > 1) {
        const uint8_t* in = out;
        const size_t up = merkle_up(m);
        cur ^= 1;
        out = up == 1 ? root : bufs[cur];
        hipLaunchKernelGGL(k_merkle_level<false>, dim3(blocks(up)), dim3(TPB), 0, s, in, m, out);
        m = up;
    }
}

}  // namespace bp

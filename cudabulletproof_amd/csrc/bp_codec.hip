// bp_codec.hip — the compact proof blob's kernels (bp_codec.h has the format and every lane body).
// Plain C++: the work is memory-bound.  256-thread blocks; a block of the encoder owns CODEC_BLK = 256
// consecutive proofs, so the raw proofs are ranked in index order inside the block and across blocks
// by the scanned block counts: nothing depends on timing.
#include <hip/hip_runtime.h>

#include "bp_codec.h"

namespace bp {

namespace {

constexpr int TPB = (int)CODEC_BLK;

// inclusive scan of one value per thread over the block's TPB threads
__device__ uint32_t block_scan(uint32_t v, uint32_t* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
        const uint32_t add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

// One lane per point of the block's proofs; a proof is compact when all of its points and its
// scalars are.  kind[i] and the block's raw count.
__global__ __launch_bounds__(TPB) void k_codec_classify(CodecArrays A, CodecLayout l, uint8_t* kind, uint32_t* blk) {
    __shared__ uint32_t raw[TPB];
    const size_t t = threadIdx.x, p0 = (size_t)blockIdx.x * TPB;
    const size_t nb = l.count - p0 < (size_t)TPB ? l.count - p0 : (size_t)TPB, np = l.npts();
    raw[t] = 0;
    __syncthreads();
    if (l.abl == 1)   // (otherwise every proof is raw whatever its points are)
        for (size_t it = t; it < nb * np; it += TPB) {
            const size_t pl = it / np;
            if (!codec_point_compact(codec_point(A, l, p0 + pl, it % np))) raw[pl] = 1;   // (lanes that race write the same 1)
        }
    __syncthreads();
    int r = 0;
    if (t < nb) {
        r = raw[t] || !codec_scalars_compact(A, l, p0 + t);
        kind[p0 + t] = (uint8_t)r;
    }
    const int c = __syncthreads_count(r);
    if (t == 0) blk[blockIdx.x] = (uint32_t)c;
}

// blk[0 .. nb) -> their exclusive prefix sums, blk[nb] = the total R.  One block: nb <= 16384.
__global__ __launch_bounds__(TPB) void k_codec_scan(uint32_t* blk, uint32_t nb) {
    __shared__ uint32_t s[TPB];
    const uint32_t t = threadIdx.x, per = (nb + TPB - 1) / TPB;
    const uint32_t lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += blk[i];
    uint32_t base = block_scan(sum, s) - sum;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = blk[i];
        blk[i] = base;
        base += c;
    }
    if (t == TPB - 1) blk[nb] = s[TPB - 1];
}

// The block's compact slots (zeros for raw proofs), its raw proofs' raw_index entries and records in
// index order, in 16-byte units over consecutive lanes; block 0's first lane writes the header, the
// padding after kind and raw_index, and the blob's size.
__global__ __launch_bounds__(TPB) void k_codec_write(CodecArrays A, CodecLayout l, size_t n, uint8_t* blob,
                                                    const uint32_t* blk, uint32_t nblk, uint64_t* bytes_out) {
    __shared__ uint32_t s[TPB];
    __shared__ uint32_t rl[TPB];
    __shared__ uint8_t kd[TPB];
    const size_t t = threadIdx.x, p0 = (size_t)blockIdx.x * TPB;
    const size_t R = nblk ? blk[nblk] : 0;
    if (blockIdx.x == 0 && t == 0) {
        codec_write_header(blob, l, n, R);
        for (size_t k = l.count; k < pad8(l.count); k++) blob[l.o_kind() + k] = 0;
        for (size_t k = 4 * R; k < pad8(4 * R); k++) blob[l.o_rawidx() + k] = 0;
        *bytes_out = l.bytes(R);
    }
    if (p0 >= l.count) return;   // (count = 0: the header alone)
    const size_t nb = l.count - p0 < (size_t)TPB ? l.count - p0 : (size_t)TPB;
    const uint8_t k = t < nb ? blob[l.o_kind() + p0 + t] : 0;
    kd[t] = k;
    const uint32_t rank = block_scan(k, s) - k, nraw = s[TPB - 1];
    const size_t j0 = blk[blockIdx.x];
    if (k) {
        rl[rank] = (uint32_t)t;
        *(uint32_t*)(blob + l.o_rawidx() + 4 * (j0 + rank)) = (uint32_t)(p0 + t);
    }
    __syncthreads();
    const size_t uc = l.Sc() / 16, ur = l.Sr() / 16;
    uint8_t* cdst = blob + l.o_compact() + p0 * l.Sc();
    for (size_t u = t; u < nb * uc; u += TPB) {
        const size_t pl = u / uc;
        blob_st(cdst + 16 * u, kd[pl] ? u128{0, 0} : codec_compact_unit(A, l, p0 + pl, u % uc));
    }
    uint8_t* rdst = blob + l.o_raw(R) + j0 * l.Sr();
    for (size_t u = t; u < nraw * ur; u += TPB) blob_st(rdst + 16 * u, codec_raw_unit(A, l, p0 + rl[u / ur], u % ur));
}

// one lane per item: a proof's (a raw record's) points and, as the last item, its field elements
__global__ __launch_bounds__(TPB) void k_codec_read_compact(BlobView v, CodecArrays A, CodecLayout l, uint32_t* bad) {
    const size_t it = (size_t)blockIdx.x * TPB + threadIdx.x, per = l.npts() + 1;
    if (it >= v.count * per) return;
    if (codec_read_compact_item(v, A, l, it / per, it % per)) atomicAdd(bad, 1u);   // (a sum: any order)
}
__global__ __launch_bounds__(TPB) void k_codec_read_raw(BlobView v, CodecArrays A, CodecLayout l, uint32_t* bad) {
    const size_t it = (size_t)blockIdx.x * TPB + threadIdx.x, per = l.npts() + 1;
    if (it >= v.R * per) return;
    if (codec_read_raw_item(v, A, l, it / per, it % per)) atomicAdd(bad, 1u);
}

}  // namespace

void launch_codec_encode(const CodecArrays& A, const CodecLayout& l, size_t n, uint8_t* blob, const CodecWs& w,
                         uint64_t* bytes_out, hipStream_t s) {
    const uint32_t nblk = (uint32_t)codec_blocks(l.count);
    if (nblk) {
        hipLaunchKernelGGL(k_codec_classify, dim3(nblk), dim3(TPB), 0, s, A, l, blob + l.o_kind(), w.blk);
        hipLaunchKernelGGL(k_codec_scan, dim3(1), dim3(TPB), 0, s, w.blk, nblk);
    }
    hipLaunchKernelGGL(k_codec_write, dim3(nblk ? nblk : 1), dim3(TPB), 0, s, A, l, n, blob, w.blk, nblk, bytes_out);
}

void launch_codec_decode(const BlobView& v, const CodecArrays& A, const CodecLayout& l, uint32_t* bad, hipStream_t s) {
    const size_t per = l.npts() + 1;
    if (v.count)
        hipLaunchKernelGGL(k_codec_read_compact, dim3((unsigned)((v.count * per + TPB - 1) / TPB)), dim3(TPB), 0, s, v, A, l,
                           bad);
    if (v.R)
        hipLaunchKernelGGL(k_codec_read_raw, dim3((unsigned)((v.R * per + TPB - 1) / TPB)), dim3(TPB), 0, s, v, A, l, bad);
}

}  // namespace bp

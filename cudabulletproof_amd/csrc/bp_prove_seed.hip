// bp_prove_seed.hip — the seeded prover's derive kernels (bp_prove_seed.h) and, below
// them, the accepted prover's retry kernels.
//
// Two launches.  k_seed_keys: one lane per proof, key_p (three compressions) into keys[B].
// k_seed_scalars: one lane per (proof, slot), one compression, one 32-byte store into rnd / sL / sR.
// The key is computed once per proof in its own small launch, not per block in LDS: a block of 256
// lanes at n = 64 spans 2-3 proofs, so a per-block key phase would run three more compressions in a
// nearly empty wave while the block's other waves wait at the barrier (7 wave-compressions per
// block where 4 do the work); the key launch costs 3 B / 64 wave-compressions against the scalar
// launch's B (2n + 4) / 64, 2 % at n = 64, and the key read is one 32-byte line shared by the
// 2n + 4 lanes of a proof.
//
// Block shape: 256 lanes, no LDS; a compression keeps its state and 16-word schedule in VGPRs
// (sha256_dev.h), well under the 64 VGPRs of full occupancy, and the work is pure VALU, so the
// grid is exact (one lane per item) and needs no stride loop.
#include "bp_prove_seed.h"

namespace bp {

__global__ __launch_bounds__(256) void k_seed_keys(SeedWords seed, const fe* __restrict__ v,
                                                   const fe* __restrict__ gamma, uint64_t index_base, uint32_t B,
                                                   uint32_t n, fe* __restrict__ keys) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= B) return;
    const fe vp = v[p], gp = gamma[p];
    fe k;
    seed_key(k.v, seed, vp.v, gp.v, index_base + p, n);
    keys[p] = k;
}

__global__ __launch_bounds__(256) void k_seed_scalars(const fe* __restrict__ keys, uint32_t B, uint32_t n,
                                                      fe* __restrict__ sL, fe* __restrict__ sR,
                                                      fe* __restrict__ rnd) {
    const uint32_t S = 2u * n + 4u;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;   // B S < 2^32 (launch_seed_derive)
    if (gid >= B * S) return;
    const uint32_t p = gid / S, slot = gid - p * S;
    const fe key = keys[p];
    fe r;
    seed_scalar(r.v, key.v, slot);
    fe* dst = slot < 4u       ? rnd + (size_t)p * 4 + slot
              : slot < 4u + n ? sL + (size_t)p * n + (slot - 4u)
                              : sR + (size_t)p * n + (slot - 4u - n);
    *dst = r;
}

void launch_seed_derive(const SeedWords& seed, const fe* v, const fe* gamma, uint64_t index_base, uint32_t B,
                        uint32_t n, fe* keys, fe* sL, fe* sR, fe* rnd, hipStream_t s) {
    launch_seed_keys(seed, v, gamma, index_base, B, n, keys, s);
    launch_seed_scalars(keys, B, n, sL, sR, rnd, s);
}

void launch_seed_keys(const SeedWords& seed, const fe* v, const fe* gamma, uint64_t index_base, uint32_t B, uint32_t n,
                      fe* keys, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(k_seed_keys, dim3((B + 255u) / 256u), dim3(256), 0, s, seed, v, gamma, index_base, B, n, keys);
}

void launch_seed_scalars(const fe* keys, uint32_t B, uint32_t n, fe* sL, fe* sR, fe* rnd, hipStream_t s) {
    if (B == 0) return;
    const uint64_t total = (uint64_t)B * (2ull * n + 4ull);   // callers bound B <= 2^22, n <= 128
    hipLaunchKernelGGL(k_seed_scalars, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, s, keys, B, n, sL, sR,
                       rnd);
}

// ------------------------------------------------------------------ the accepted prover
// The retry loop's kernels, in the derive kernels' shape: 256 lanes, exact grids, one item per lane.
// All of them are bandwidth- or latency-trivial beside the prover and verifier launches they sit
// between (a round moves 2400 bytes per retried proof at n = 64 where the prover computes ~650 scalar
// multiplications for it), so they are written for a fixed result, not for speed: the rejected list
// is built by block counts, a one-block scan and a ballot-ranked fill, never by atomics, and comes
// out ascending whatever the launch order.

// out[j] = key_{p,a} for p = list[j] (list null: p = j) and a = attempt[p] (attempt null: a0).  One
// lane per proof, one compression (none for a = 0).
__global__ __launch_bounds__(256) void k_try_keys(const fe* __restrict__ keys, const uint32_t* __restrict__ list,
                                                  const uint8_t* __restrict__ attempt, uint32_t a0, uint32_t m,
                                                  fe* __restrict__ out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t p = list ? list[j] : j;
    const uint32_t a = attempt ? attempt[p] : a0;
    const fe key = keys[p];
    fe k;
    seed_try_key(k.v, key.v, a);
    out[j] = k;
}

// proof i of the round: its batch index, whether it is rejected (valid, not ok) or accepted (valid, ok)
struct AcceptLane {
    uint32_t p;
    bool rej, acc;
};
__device__ __forceinline__ AcceptLane accept_lane(const uint8_t* __restrict__ ok, const uint8_t* __restrict__ valid,
                                                  const uint32_t* __restrict__ src, uint32_t m, uint32_t i) {
    AcceptLane l{0, false, false};
    if (i < m) {
        l.p = src ? src[i] : i;
        const bool v = valid[i] != 0, o = ok[i] != 0;
        l.rej = v && !o;
        l.acc = v && o;
    }
    return l;
}

// k_accept_select, step 1: the verdicts into attempts[], the block's rejected count into blk[].
// Every lane of the block reaches the ballot and the barrier (no early return).
__global__ __launch_bounds__(ACCEPT_BLK) void k_accept_count(const uint8_t* __restrict__ ok,
                                                             const uint8_t* __restrict__ valid,
                                                             const uint32_t* __restrict__ src, uint32_t m,
                                                             uint32_t round, uint8_t* __restrict__ attempts,
                                                             uint32_t* __restrict__ blk) {
    static_assert(ACCEPT_BLK == 256, "four waves per block");
    __shared__ uint32_t wc[ACCEPT_BLK / 64];
    const uint32_t i = blockIdx.x * ACCEPT_BLK + threadIdx.x;
    const AcceptLane l = accept_lane(ok, valid, src, m, i);
    if (i < m) {
        if (l.acc) attempts[l.p] = (uint8_t)round;
        else if (round == 1u) attempts[l.p] = 0;
    }
    const unsigned long long b = __ballot(l.rej);
    if ((threadIdx.x & 63u) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// k_accept_select, step 2: blk[nb] to its exclusive scan in place, the total to *cnt.  One block;
// lane t owns the `per` consecutive entries from t * per (nb <= 2^14 for 2^22 proofs: per <= 64).
__global__ __launch_bounds__(256) void k_accept_scan(uint32_t* __restrict__ blk, uint32_t nb, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t sh[256];
    const uint32_t t = threadIdx.x, per = (nb + 255u) / 256u;
    const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
    uint32_t sum = 0;
    for (uint32_t k = lo; k < hi; k++) sum += blk[k];
    sh[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const uint32_t add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    uint32_t run = sh[t] - sum;
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t c = blk[k];
        blk[k] = run;
        run += c;
    }
    if (t == 255u) *cnt = sh[255];
}

// k_accept_select, step 3: the rejected proofs' batch indices into list[], ascending, with their
// v | gamma gathered.  A lane's position: the block's scanned offset, the earlier waves' counts, its
// rank in its wave's ballot; at most *cnt positions in all (the host sized list, cv, cg from it).
__global__ __launch_bounds__(ACCEPT_BLK) void k_accept_fill(const uint8_t* __restrict__ ok,
                                                            const uint8_t* __restrict__ valid,
                                                            const uint32_t* __restrict__ src, uint32_t m,
                                                            const uint32_t* __restrict__ blk, const fe* __restrict__ v,
                                                            const fe* __restrict__ gamma, uint32_t* __restrict__ list,
                                                            fe* __restrict__ cv, fe* __restrict__ cg) {
    __shared__ uint32_t wc[ACCEPT_BLK / 64];
    const uint32_t i = blockIdx.x * ACCEPT_BLK + threadIdx.x;
    const AcceptLane l = accept_lane(ok, valid, src, m, i);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(l.rej);
    if (lane == 0) wc[w] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!l.rej) return;
    uint32_t k = blk[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < w; q++) k += wc[q];
    list[k] = l.p;
    cv[k] = v[l.p];
    cg[k] = gamma[l.p];
}

// One lane per 16-byte piece.  The pieces are numbered along the compact source, so a wave reads
// 1 KiB of consecutive bytes; it writes whole 32- or 128-byte records at the rows list[j].  Per
// proof: 5 points of 8 pieces, 7 scalars of 2, L and R of 8 Lr each, and the valid byte (a lane of
// its own, after the pieces).
__global__ __launch_bounds__(256) void k_accept_scatter(const uint4* __restrict__ spts, const uint4* __restrict__ sfe,
                                                        const uint4* __restrict__ slr,
                                                        const uint8_t* __restrict__ svalid, ProveOut dst,
                                                        const uint32_t* __restrict__ list, uint32_t m, uint32_t Lr) {
    const uint32_t npt = 40u * m, nfe = 14u * m, nlr = 16u * Lr * m;
    uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < npt) {
        const uint32_t f = g / (8u * m), r = g - f * 8u * m, j = r >> 3;
        ge* d = f == 0 ? dst.V : f == 1 ? dst.A : f == 2 ? dst.S : f == 3 ? dst.T1 : dst.T2;
        ((uint4*)(d + list[j]))[r & 7u] = spts[g];
    } else if ((g -= npt) < nfe) {
        const uint32_t f = g / (2u * m), r = g - f * 2u * m, j = r >> 1;
        fe* d = f == 0 ? dst.taux : f == 1 ? dst.mu : f == 2 ? dst.t : f == 3 ? dst.c : f == 4 ? dst.x
                : f == 5 ? dst.a : dst.b;
        ((uint4*)(d + list[j]))[r & 1u] = sfe[g];
    } else if ((g -= nfe) < nlr) {
        const uint32_t per = 8u * Lr, f = g / (per * m), r = g - f * per * m, j = r / per;
        ge* d = f == 0 ? dst.L : dst.R;
        ((uint4*)(d + (size_t)list[j] * Lr))[r - j * per] = slr[g];
    } else if ((g -= nlr) < m) {
        dst.valid[list[g]] = svalid[g];
    }
}

void launch_try_keys_list(const fe* keys, const uint32_t* list, uint32_t m, uint32_t a, fe* out, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_try_keys, dim3((m + 255u) / 256u), dim3(256), 0, s, keys, list, (const uint8_t*)nullptr, a, m,
                       out);
}

void launch_try_keys_at(const fe* keys, const uint8_t* attempt, uint32_t B, fe* out, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(k_try_keys, dim3((B + 255u) / 256u), dim3(256), 0, s, keys, (const uint32_t*)nullptr, attempt, 0u,
                       B, out);
}

void launch_accept_count(const uint8_t* ok, const uint8_t* valid, const uint32_t* src, uint32_t m, uint32_t round,
                         uint8_t* attempts, uint32_t* blk, uint32_t* cnt, hipStream_t s) {
    if (m == 0) return;
    const uint32_t nb = (m + ACCEPT_BLK - 1u) / ACCEPT_BLK;
    hipLaunchKernelGGL(k_accept_count, dim3(nb), dim3(ACCEPT_BLK), 0, s, ok, valid, src, m, round, attempts, blk);
    hipLaunchKernelGGL(k_accept_scan, dim3(1), dim3(256), 0, s, blk, nb, cnt);
}

void launch_accept_fill(const uint8_t* ok, const uint8_t* valid, const uint32_t* src, uint32_t m, const uint32_t* blk,
                        const fe* v, const fe* gamma, uint32_t* list, fe* cv, fe* cg, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_accept_fill, dim3((m + ACCEPT_BLK - 1u) / ACCEPT_BLK), dim3(ACCEPT_BLK), 0, s, ok, valid, src,
                       m, blk, v, gamma, list, cv, cg);
}

void launch_accept_scatter(const ProveOut& src, const ProveOut& dst, const uint32_t* list, uint32_t m, uint32_t Lr,
                           hipStream_t s) {
    if (m == 0) return;
    const uint64_t total = (uint64_t)m * (54ull + 16ull * Lr + 1ull);   // pieces + the valid bytes
    hipLaunchKernelGGL(k_accept_scatter, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, s,
                       (const uint4*)src.V, (const uint4*)src.taux, (const uint4*)src.L, (const uint8_t*)src.valid, dst,
                       list, m, Lr);
}

}  // namespace bp

// bp_prove_seed.hip — the seeded prover's derive kernels (bp_prove_seed.h).
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
    if (B == 0) return;
    const uint64_t total = (uint64_t)B * (2ull * n + 4ull);   // callers bound B <= 2^22, n <= 128
    hipLaunchKernelGGL(k_seed_keys, dim3((B + 255u) / 256u), dim3(256), 0, s, seed, v, gamma, index_base, B, n, keys);
    hipLaunchKernelGGL(k_seed_scalars, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, s, keys, B, n, sL, sR,
                       rnd);
}

}  // namespace bp

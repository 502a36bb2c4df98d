// bp_gens_derive.hip — the kernels that derive generators from seeds (bp_gens_derive.h has the rule
// and both lane bodies).  Plain C++: one lane per point, 256-lane blocks, exact grids.
// The seed comes by value in the kernel arguments (eight wave-uniform words), the hash states and
// blocks stay in registers, and a lane writes only its own 128 bytes, as eight 16-byte stores: no
// LDS, no scratch, no atomics.
#include <hip/hip_runtime.h>

#include "bp_gens_derive.h"

namespace bp {

namespace {

constexpr int TPB = GENS_BLK;
constexpr uint64_t LAUNCH_LANES = 1ull << 30;   // lanes of one launch (a grid stays far below 2^32 threads)

__device__ __forceinline__ void store_point(ge* out, const ge& p) {
    const fe* f = &p.X;
    uint4* o = (uint4*)out;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        o[2 * k] = make_uint4(lo32(f[k].v[0]), hi32(f[k].v[0]), lo32(f[k].v[1]), hi32(f[k].v[1]));
        o[2 * k + 1] = make_uint4(lo32(f[k].v[2]), hi32(f[k].v[2]), lo32(f[k].v[3]), hi32(f[k].v[3]));
    }
}

// out[k] = point first + k; first + k < 2^32 for every k < count (the launcher's callers check)
__global__ __launch_bounds__(TPB) void k_derive_base_points(GenSeed seed, uint64_t first, uint64_t count, ge* out) {
    const uint64_t k = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    store_point(out + k, derive_base_point(seed, (uint32_t)(first + k)));
}

__global__ __launch_bounds__(64) void k_derive_single_point(GenSeed seed, ge* out) {
    if (threadIdx.x) return;
    store_point(out, derive_single_point(seed));
}

}  // namespace

void launch_derive_base_points(ge* out, const GenSeed& seed, uint64_t first, uint64_t count, hipStream_t s) {
    for (uint64_t done = 0; done < count; done += LAUNCH_LANES) {
        const uint64_t m = count - done < LAUNCH_LANES ? count - done : LAUNCH_LANES;
        hipLaunchKernelGGL(k_derive_base_points, dim3((unsigned)((m + TPB - 1) / TPB)), dim3(TPB), 0, s, seed,
                           first + done, m, out + done);
    }
}

void launch_derive_single_point(ge* out, const GenSeed& seed, hipStream_t s) {
    hipLaunchKernelGGL(k_derive_single_point, dim3(1), dim3(64), 0, s, seed, out);
}

}  // namespace bp

// bp_buf.h — the engine's grow-only buffers and the workspaces built from them that more than one
// source file touches (internal to the library).  Calls the HIP runtime; the sizes are bp_layout.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "bp_layout.h"

namespace bp {

// A grow-only device buffer (Buf) or pinned host staging buffer (PinnedBuf).  need() frees the old
// allocation when it grows: what must be drained first is each call site's own rule.
template <bool PINNED>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    static hipError_t free_(void* q) { return PINNED ? hipHostFree(q) : hipFree(q); }
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = free_(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            cap = 0;
        }
        hipError_t e = PINNED ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    // frees the buffer; the pointer is dropped even if the free fails (nothing is left to free twice)
    hipError_t release() {
        hipError_t e = p ? free_(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    template <class T> T* as() const { return (T*)p; }
};
using Buf = GrowBuf<false>;
using PinnedBuf = GrowBuf<true>;
// every buffer of a workspace grown to its table's size (bp_layout.h)
template <size_t N>
hipError_t need_all(Buf (&b)[N], const size_t (&sz)[N]) {
    for (size_t i = 0; i < N; i++) {
        hipError_t e = b[i].need(sz[i]);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// A caller stream's Pippenger state (bp_pippenger.hip; owned by the engine's per-stream record): the
// top and the bottom part's buffers (BP_PIP_BUFS), and the side stream that carries the latency-bound
// chains with its events, created on first use — all of them or none.
struct PipPair {
    Buf hi[PIP_COUNT], lo[PIP_COUNT];
    hipStream_t side = nullptr;
    hipEvent_t ev[3] = {};   // [0] top part's buckets done, [1] bottom part done, [2] chain done
};

}  // namespace bp

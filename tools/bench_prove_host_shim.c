/* bench_prove_host_shim.c — the timed region of tools/bench_prove_host.py in C: one host prover call
 * and the freeing of every vector it handed out, between two readings of the monotonic clock.  (From
 * Python the 4 x count calls of free alone would cost more than the prover.)  The entry point comes
 * in as a pointer, so the same shim times this checkout's library and another checkout's. */
#include <stdlib.h>
#include <time.h>

#include "../include/cudabulletproof_hip.h"

typedef int (*seeded_host_fn)(RangeProof*, uint8_t*, const fe25519*, const fe25519*, size_t, size_t, const PointVector*,
                              const PointVector*, const ge25519*, const ge25519*, const uint8_t*, uint64_t);
typedef int (*accepted_host_fn)(RangeProof*, uint8_t*, uint8_t*, const fe25519*, const fe25519*, size_t, size_t,
                                const PointVector*, const PointVector*, const ge25519*, const ge25519*, const uint8_t*,
                                uint64_t, int, int, int);

static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static void free_all(RangeProof* proofs, size_t count) {
    for (size_t i = 0; i < count; i++) {
        InnerProductProof* ip = &proofs[i].ip_proof;
        free(ip->a.elements); free(ip->b.elements); free(ip->L.elements); free(ip->R.elements);
        ip->a.elements = ip->b.elements = NULL;
        ip->L.elements = ip->R.elements = NULL;
    }
}

/* ms of call + free; *rc the call's return code; *call_ms the call alone */
double shim_seeded_host(seeded_host_fn fn, RangeProof* proofs, uint8_t* valid, const fe25519* v, const fe25519* gamma,
                        size_t count, size_t n, const PointVector* G, const PointVector* H, const ge25519* g,
                        const ge25519* h, const uint8_t* seed32, uint64_t index_base, int* rc, double* call_ms) {
    const double t0 = now_ms();
    *rc = fn(proofs, valid, v, gamma, count, n, G, H, g, h, seed32, index_base);
    const double t1 = now_ms();
    if (*rc == 0) free_all(proofs, count);
    *call_ms = t1 - t0;
    return now_ms() - t0;
}

/* keep != 0: the vectors are left for the caller to read (and to free with shim_free) */
double shim_accepted_host(accepted_host_fn fn, RangeProof* proofs, uint8_t* valid, uint8_t* attempts, const fe25519* v,
                          const fe25519* gamma, size_t count, size_t n, const PointVector* G, const PointVector* H,
                          const ge25519* g, const ge25519* h, const uint8_t* seed32, uint64_t index_base, int max_attempts,
                          int check, int num_gpus, int keep, int* rc, double* call_ms) {
    const double t0 = now_ms();
    *rc = fn(proofs, valid, attempts, v, gamma, count, n, G, H, g, h, seed32, index_base, max_attempts, check, num_gpus);
    const double t1 = now_ms();
    if (*rc == 0 && !keep) free_all(proofs, count);
    *call_ms = t1 - t0;
    return now_ms() - t0;
}

void shim_free(RangeProof* proofs, size_t count) { free_all(proofs, count); }

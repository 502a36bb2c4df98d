/* cudabulletproof_hip.h — C ABI of libcudabulletproof_hip.so (MI355X / gfx950).
 *
 * Part 1 is the drop-in boundary: every entry point of the reference's
 * cuda_bulletproof.h, same names, same argument meaning, same conventions
 * (host pointers owned by the caller, synchronous, inputs never modified,
 * length mismatch -> message on stderr and *result untouched / false,
 * device errors -> message on stderr and exit(EXIT_FAILURE), as CUDA_CHECK does
 * in cuda_bulletproof_kernels.cu:13-21).  The reference's bulletproof_range_proof.cu
 * and complete_bulletproof_test.cu link against this library unchanged
 * (INTEGRATION.md).
 *
 * Part 2 is additive: batched, device-resident entry points (flat wire format,
 * explicit stream, error codes) used by the Python package and bench.py.  Every
 * `void* stream` is a hipStream_t; NULL means the default (null) stream.
 *
 * The types are layout-identical to the reference's (curve25519_ops.h:15-25,
 * bulletproof_vectors.h:8-17, :65-74, bulletproof_range_proof.h:7-18); when the
 * reference headers are included first, theirs are used.
 *
 * Points are taken as given, as the reference takes them: a ge25519 is sixteen limbs,
 * any limbs.  Z need not be 1, T need not be X*Y, no coordinate need be below p; the
 * result has the bits the reference's arithmetic gives on those limbs.  This holds for
 * every point argument: MSM points, generators (with or without prefix tables), proof
 * points, Pippenger inputs.  The kernels' Z = 1 shortcuts test exact limb equality
 * (1, 0, 0, 0), wave-uniformly, so p + 1 or 1 + 2^255 take the general product.  Pinned by
 * tests/test_projective_points.py against the reference's own outputs
 * (tests/golden/projective.npz, point.npz) and the CPU restatement.
 */
#ifndef CUDABULLETPROOF_HIP_H
#define CUDABULLETPROOF_HIP_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifndef CURVE25519_OPS_H
typedef struct { uint64_t limbs[4]; } fe25519;              /* curve25519_ops.h:15-17 */
typedef struct { fe25519 X, Y, Z, T; } ge25519;              /* curve25519_ops.h:20-25 */
#endif
#ifndef BULLETPROOF_VECTORS_H
typedef struct { fe25519* elements; size_t length; } FieldVector;   /* bulletproof_vectors.h:8-11 */
typedef struct { ge25519* elements; size_t length; } PointVector;   /* bulletproof_vectors.h:14-17 */
typedef struct {                                                    /* bulletproof_vectors.h:65-74 */
    size_t n;
    FieldVector a;
    FieldVector b;
    fe25519 c;
    PointVector L;
    PointVector R;
    size_t L_len;
    fe25519 x;
} InnerProductProof;
#endif
#ifndef BULLETPROOF_RANGE_PROOF_H
typedef struct {                                                    /* bulletproof_range_proof.h:7-18 */
    ge25519 V, A, S, T1, T2;
    fe25519 taux, mu, t;
    InnerProductProof ip_proof;
} RangeProof;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================== Part 1: reference surface */

/* cuda_bulletproof.h:13 (cuda_bulletproof_kernels.cu:62). result = canonical-tree sum of
 * device-normalized scalar*point terms. */
void cuda_point_vector_multi_scalar_mul(ge25519* result, const FieldVector* scalars, const PointVector* points);
/* cuda_bulletproof.h:17 (cuda_bulletproof_kernels.cu:119): same result. */
void cuda_point_vector_multi_scalar_mul_shared(ge25519* result, const FieldVector* scalars,
                                               const PointVector* points);

/* cuda_bulletproof.h:22 (cuda_inner_product.cu:97): the reference's GPU reduction order
 * (n <= 512: block halving tree; n > 512: grid-stride + two trees). */
void cuda_field_vector_inner_product(fe25519* result, const FieldVector* a, const FieldVector* b);
/* cuda_bulletproof.h:26 (declared there, never defined with C linkage in the reference):
 * the n <= 512 halving-tree order for any n. */
void cuda_field_vector_inner_product_shared(fe25519* result, const FieldVector* a, const FieldVector* b);
/* cuda_inner_product.cu:302 (extern "C", not in the reference header). */
void cuda_batch_field_vector_inner_product(fe25519* results, const FieldVector* a_vectors,
                                           const FieldVector* b_vectors, size_t num_vectors);

/* cuda_bulletproof.h:31-46 (cuda_field_ops.cu:257, :293, :329, :374). */
void cuda_batch_field_add(fe25519* results, const fe25519* a, const fe25519* b, size_t count);
void cuda_batch_field_sub(fe25519* results, const fe25519* a, const fe25519* b, size_t count);
void cuda_batch_field_mul(fe25519* results, const fe25519* a, const fe25519* b, size_t count);
void cuda_batch_field_mul_karatsuba(fe25519* results, const fe25519* a, const fe25519* b, size_t count);
/* reproduces field_square_kernel (cuda_field_ops.cu:147), which is NOT fe25519_sq */
void cuda_batch_field_square(fe25519* results, const fe25519* inputs, size_t count);
/* cuda_bulletproof.h:50 (cuda_field_ops.cu:405): the reference kernel races;
 * this defines it as the host fe25519_invert chain applied elementwise. */
void cuda_batch_field_invert(fe25519* results, const fe25519* inputs, size_t count);
/* cuda_bulletproof.h:55 (cuda_field_ops.cu:533): limbwise u64 add, no carry, no reduction */
void cuda_soa_field_add(fe25519* results, const fe25519* a, const fe25519* b, size_t count);

/* cuda_bulletproof.h:61 (cuda_range_proof_verify.cu:82, notebook-only in the reference). */
bool cuda_range_proof_verify(const RangeProof* proof, const ge25519* V, size_t n, const PointVector* G,
                             const PointVector* H, const ge25519* g, const ge25519* h);
/* cuda_bulletproof.h:72 (cuda_range_proof_verify.cu:130). */
bool cuda_inner_product_verify(const InnerProductProof* proof, const ge25519* P, const PointVector* G,
                               const PointVector* H, const ge25519* Q);

/* cuda_bulletproof.h:81-84: declared but never defined by the reference; here they time the
 * corresponding GPU path and print one line each. */
void cuda_benchmark_multi_scalar_mul(int iterations, size_t vector_size);
void cuda_benchmark_inner_product(int iterations, size_t vector_size);
void cuda_benchmark_field_operations(int iterations, size_t batch_size);
void cuda_benchmark_range_proof(int iterations, size_t bit_size);

/* ===================================================================== Part 2: batched device API */

/* Flat wire format of a batch of range proofs; every pointer is DEVICE memory.
 * Per proof p: V[p], A[p], S[p], T1[p], T2[p], t[p], c[p], x[p]; a/b: ab_len entries
 * at p*ab_len; L/R: L_len entries at p*L_len (L[0]/R[0] are never read, crv:180-205).
 * V is the caller's V argument of the verify.  taux, mu and Vp (the proof's own V) are read
 * only by the range_proof_verify semantics (hipbp_batch_range_proof_verify_std); Vp NULL means
 * "equal to V". */
typedef struct {
    size_t count, n, ab_len, L_len;
    const ge25519 *V, *A, *S, *T1, *T2;
    const fe25519 *t, *a, *b, *c, *x;
    const ge25519 *L, *R;
    const fe25519 *taux, *mu;
    const ge25519* Vp;
} hipbp_proof_batch;

typedef enum {
    HIPBP_OK = 0,
    HIPBP_ERR_ARG = 1,       /* unsupported shape / null pointer */
    HIPBP_ERR_DEVICE = 2,    /* HIP runtime error (message via hipbp_last_error) */
} hipbp_status;

const char* hipbp_last_error(void);
/* Number of HIP devices visible. */
int hipbp_device_count(void);

/* cuda_range_proof_verify (cuda_bulletproof.h:61, crv:82) over an ARRAY of the reference's own host
 * structs: ok[i] = cuda_range_proof_verify(&proofs[i], &V[i], n, G, H, g, h) for i < count, bit for
 * bit, with the reference's length check per proof (message on stderr, ok[i] = 0).  The proofs are
 * packed into the flat batch format, sharded in contiguous blocks over num_gpus devices (<= 0: all
 * visible; more than are visible: HIPBP_ERR_ARG, nothing verified) starting at the calling thread's
 * current device (shard d on device (current + d) mod the device count, so num_gpus = 1 stays on
 * the current device), one host thread per device: 1024-proof chunks are packed into pinned staging, copied
 * and pushed as they are packed, alternating over two verify pipelines on two streams; one D2H of
 * the verdicts; no data-path exchange between devices.  Each device's engine keeps the fixed-base
 * prefix tables of the last generator set it was called with (G | H | h, exact byte compare;
 * HIPBP_HOST_PREFIX_BITS, default 16, at most 1.25 GB; 0: none), so calls after the first against
 * the same generators run the table-started scalar multiplications.  Proofs whose a/b length or round
 * count differs from the first valid proof's go through the single-proof path.  Host pointers,
 * synchronous.  Returns HIPBP_OK or an error code (hipbp_last_error); on an error ok is
 * undefined.  No reference counterpart (the additive batch entry point). */
int hipbp_batch_range_proof_verify_host(const RangeProof* proofs, const ge25519* V, size_t count, size_t n,
                                        const PointVector* G, const PointVector* H, const ge25519* g,
                                        const ge25519* h, int num_gpus, uint8_t* ok);

/* Batched cuda_range_proof_verify semantics. G/H: n generators, g/h: 1 point (device).
 * ok[count] gets 1/0; P_out / check_out (nullable) get the IPA point P and the check point. */
int hipbp_batch_range_proof_verify(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                   const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                   ge25519* check_out, void* stream);
/* Batched range_proof_verify semantics (bulletproof_range_proof.cu:1717, the reference's CPU
 * "STANDARD VERIFICATION": V match, compute_precise_delta, enhanced_range_check,
 * robust_polynomial_identity_check, calculate_inner_product_point, inner_product_verify with its
 * own accept rule).  Needs batch->taux/mu.  Nullable extra outputs:
 * flags_out[count]: bit0 V match, bit1 enhanced_range_check, bit2 polynomial identity methods 1|2,
 * bit3 method 3, bit4 method 4, bit5 inner_product_verify;
 * poly_out[4*count]: per proof left side, right side, and the two method-3 products. */
int hipbp_batch_range_proof_verify_std(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                       const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                       ge25519* check_out, uint8_t* flags_out, ge25519* poly_out, void* stream);
/* Batched cuda_inner_product_verify semantics; P[count] given (device). */
int hipbp_batch_inner_product_verify(const hipbp_proof_batch* batch, const ge25519* P, const ge25519* G,
                                     const ge25519* H, const ge25519* Q, uint8_t* ok, ge25519* check_out,
                                     void* stream);
/* Streaming verify pipeline.  A verify has a log2(n)+1-deep chain of dependent stages
 * (stage 0, IPA fold rounds 1..L-1, final); the pipeline keeps up to log2(n)+1 batches in
 * flight and each push runs ONE tick: stage 0 of the pushed batch, round r of the batch
 * pushed r ticks earlier, the final stage of the oldest, all in one kernel launch.
 * A batch's outputs (ok / P_out / check_out, device memory) are complete after
 * depth-1 further pushes or a flush; its inputs (and P_in) are consumed by its own push.
 * range_mode 1: cuda_range_proof_verify semantics (h = the generator h; g may be NULL);
 * range_mode 2: range_proof_verify semantics (g, h the generators; batch taux/mu required);
 * range_mode 0: cuda_inner_product_verify semantics (h = Q, P_in required, g may be NULL).
 * Returns NULL on error (see hipbp_last_error). */
void* hipbp_pipeline_create(size_t max_batch, size_t n, int range_mode, const ge25519* G, const ge25519* H,
                            const ge25519* g, const ge25519* h, void* stream);
/* A push is accepted or refused, never half done.  Batches of different L_len (or with and without
 * a split stage 0) may share the ring; a batch that, with those in flight, would bring a later tick
 * past the kernel's region list (or past 2^32 lanes) is refused: HIPBP_ERR_ARG, hipbp_last_error says
 * "push refused ... run a drain tick (push(NULL)) and retry", no tick runs and the pipeline is exactly
 * as before the call.  The in-flight batches complete under drain ticks or a flush as usual, and the
 * same batch is accepted after at most `depth` drain ticks.  Batches that all have one L_len and one
 * split setting (the steady state) are never refused for the region list. */
int hipbp_pipeline_push(void* pipeline, const hipbp_proof_batch* batch /* NULL = drain tick */,
                        const ge25519* P_in, uint8_t* ok, ge25519* P_out, ge25519* check_out,
                        uint8_t* flags_out /* range_mode 2, nullable */, ge25519* poly_out /* idem */);
int hipbp_pipeline_flush(void* pipeline);
int hipbp_pipeline_depth(void* pipeline);
/* Fixed-base prefix tables for the pipeline's generators (no reference counterpart; an
 * additive speed-up with the same bits).  bits = K in 1..24 builds, for each of the 2n + 2
 * bases G_i, H_i, h, g, the state of ge25519_scalarmult after every possible top-K-bit prefix
 * of a scalar ((2n + 2) * 2^K * 128 bytes of device memory: 17.4 GB at n = 64, K = 20).  The
 * scalar multiplications on those bases (the two MSMs, fold round 0, t*h, c*Q, the polynomial
 * terms on g and h) then start at bit 255 - K from the table entry; the operations after it are
 * unchanged, so every output has the same bits.  Built from the generator CONTENTS at this call
 * (synchronous); the caller must not change G/H/g/h afterwards while tables are on.  bits = 0
 * frees them.  The pipeline must be idle (flushed). */
int hipbp_pipeline_prefix_tables(void* pipeline, int bits);
/* Generator sets (no reference counterpart): a device snapshot of G[n], H[n], g, h (device
 * buffers, copied at create; the caller may free them afterwards) plus, for prefix_bits in 1..24,
 * their fixed-base prefix tables (as hipbp_pipeline_prefix_tables; 0 = none).  Synchronous.
 * Returns NULL on error.  One set serves the prover and any number of verify pipelines. */
void* hipbp_gens_create(size_t n, const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                        int prefix_bits, void* stream);
void hipbp_gens_destroy(void* gens);
/* Generators derived from 32-byte seeds (no library counterpart in the reference: the rule is its
 * test driver's, complete_bulletproof_test.cu:33-109, bit for bit).
 *   vector form, point i:  X = le(SHA-256(seed32 | BE32(i)))  Y = le(SHA-256(the 32 bytes of X))
 *                          Z = 1                              T = fe25519_mul(X, Y)
 *   single form (g, h):    X = le(SHA-256(seed32))            Y = Z = 1    T = fe25519_mul(X, 1)
 * le() is a plain little-endian load: bit 255 is kept and nothing is reduced or canonicalised; T is
 * a product in the reference's arithmetic in both forms.  out[k] is point first + k.  Only the low
 * 32 bits of an index are hashed, so first + count <= 2^32 is required; a block [first, first + count)
 * gives the same bytes however it is cut into calls.  count = 0 returns HIPBP_OK and writes nothing;
 * a null out or seed32, or first + count > 2^32, gives HIPBP_ERR_ARG, writes nothing and enqueues
 * nothing.
 * device out[count]; seed32 is HOST memory, read at the call (the caller may free it on return);
 * asynchronous on stream */
int hipbp_derive_base_points(ge25519* out, const uint8_t seed32[32], uint64_t first, size_t count, void* stream);
int hipbp_derive_single_point(ge25519* out, const uint8_t seed32[32], void* stream);
/* the same on host memory, on the CPU (one thread); works in a process that sees no device */
int hipbp_derive_base_points_host(ge25519* out, const uint8_t seed32[32], uint64_t first, size_t count);
int hipbp_derive_single_point_host(ge25519* out, const uint8_t seed32[32]);
/* hipbp_gens_create with the four arrays derived in place (no staging buffer, no copy): G and H the
 * first n points of seed_G's and seed_H's vectors, g and h the single points of seed_g and seed_h;
 * then the prefix tables as before.  The seeds are HOST memory, read at the call.  The checks on n
 * and prefix_bits are hipbp_gens_create's.  Synchronous; NULL on error. */
void* hipbp_gens_create_seeded(size_t n, const uint8_t seed_G[32], const uint8_t seed_H[32],
                               const uint8_t seed_g[32], const uint8_t seed_h[32], int prefix_bits, void* stream);
/* Copy a set's points out to caller-owned DEVICE buffers G[n], H[n], g[1], h[1] (any may be NULL =
 * skip); *n and *prefix_bits (HOST, nullable) are written at the call.  For the entry points that
 * take arrays (a seeded set's caller never held its points); serves any set.  A null gens, or one
 * created on another device, gives HIPBP_ERR_ARG.  Asynchronous on stream. */
int hipbp_gens_copy_points(void* gens, ge25519* G, ge25519* H, ge25519* g, ge25519* h, size_t* n, int* prefix_bits,
                           void* stream);
/* The pipeline reads its generators and prefix tables from `gens` (same n; the pipeline must be
 * idle; the set must outlive the pipeline's use of it).  Results keep their bits. */
int hipbp_pipeline_use_gens(void* pipeline, void* gens);
/* hipbp_batch_range_proof_verify with the generators and prefix tables of a generator set (same n,
 * same device): a one-shot batch that starts its generator-based scalar multiplications from the
 * tables (the pipeline path's speed without a pipeline handle).  Same bits as the plain call. */
int hipbp_batch_range_proof_verify_gens(const hipbp_proof_batch* batch, void* gens, uint8_t* ok, ge25519* P_out,
                                        ge25519* check_out, void* stream);
/* Split stage 0 for the batches pushed from now on (on = 1; range_mode 1 or 2, 4 <= n <= 64): a
 * batch's stage-0 tick runs only fold round 0 (and the range_proof_verify polynomial terms); its
 * two MSMs' terms, t*h and c*Q, which only the final assembly reads, run in chunks inside its
 * fold-round ticks, whose own items shrink round by round.  A finite batch then fills the rounds
 * before its latency-bound last ticks.  Same bits either way.  HIPBP_ERR_ARG where it does not
 * apply: inner-product mode, n above the lane-tree limit (HIPBP_LANE_TREE_MAX), or n > 512 (a
 * split tick's 2 log2 n + 5 regions must fit the kernel's region list). */
int hipbp_pipeline_defer_msm(void* pipeline, int on);
void hipbp_pipeline_destroy(void* pipeline);

/* ---- prover: generate_range_proof (bulletproof_range_proof.cu:1159) + inner_product_prove
 * (bulletproof_vectors.cu:277) + fix_inner_product_proof (rp.cu:198), batched, bit-exact.
 * The prover's randomness is an input: each random scalar is the 32 bytes that
 * generate_random_scalar (rp.cu:153) produces (RAND_bytes + its masks), as 4 LE limbs.
 * All pointers DEVICE memory.  n: power of two, 1..128 (validate_range_input reads byte n/8). */
typedef struct {
    size_t count, n;
    const fe25519* v;       /* [count] value (fe25519_frombytes of the value bytes) */
    const fe25519* gamma;   /* [count] blinding of V = g^v h^gamma */
    const fe25519* sL;      /* [count*n] */
    const fe25519* sR;      /* [count*n] */
    const fe25519* rnd;     /* [count*4] alpha, rho, tau1, tau2 */
} hipbp_prove_input;
/* Output in the flat wire format of hipbp_proof_batch (ab_len = 1, L_len = log2 n), so it can be
 * verified as is.  valid[p] = 0: validate_range_input refused the value; the proof is then the
 * reference's zeroed one (V, A, S, T1, T2 identity; taux, mu, t 0; the rest 0). */
typedef struct {
    ge25519 *V, *A, *S, *T1, *T2;          /* [count] */
    fe25519 *taux, *mu, *t, *c, *x;        /* [count] */
    fe25519 *a, *b;                        /* [count] */
    ge25519 *L, *R;                        /* [count*L_len] */
    uint8_t* valid;                        /* [count] */
} hipbp_proof_out;
int hipbp_batch_generate_range_proof(const hipbp_prove_input* in, const ge25519* G, const ge25519* H,
                                     const ge25519* g, const ge25519* h, hipbp_proof_out* out, void* stream);
/* The same with a generator set's generators and prefix tables (every scalar multiplication of
 * the prover is on G_i, H_i, g or h); same bits as hipbp_batch_generate_range_proof on them. */
int hipbp_batch_generate_range_proof_gens(const hipbp_prove_input* in, void* gens, hipbp_proof_out* out,
                                          void* stream);

/* ---- seeded prover (no reference counterpart): the 2n + 4 random scalars of every proof derived
 * on the GPU from one 32-byte SECRET seed, so a caller supplies values, blindings and the seed
 * instead of 2n + 4 scalars of 32 bytes per proof.  Byte-exact derivation, all integers little-endian:
 *   key_p  = SHA-256("hipbpProverKeyV1" || seed[32] || v_p || gamma_p || LE64(index_base + p) || LE32(n))
 *   d      = SHA-256("hipbpProverRndV1" || key_p || LE32(slot))
 *   d[0] &= 0xF8; d[31] &= 0x7F; d[31] |= 0x40      (generate_random_scalar's masks, rp.cu:153-159)
 *   scalar = d as 4 LE u64 limbs
 * v_p, gamma_p: the 32 bytes of the four limbs as stored (not canonicalised); index_base + p wraps
 * mod 2^64.  slot 0..3 = alpha, rho, tau1, tau2 (rnd's order), 4 + i = sL[i], 4 + n + i = sR[i].
 * The key binds v, gamma and the proof's global index, so a seed reused with other values never
 * reuses a nonce, and a batch cut into several calls (each with its own index_base) yields the
 * proofs of the single call.  seed32 is a HOST pointer, read during the call (it travels in the
 * kernel arguments); every other pointer is DEVICE memory.
 *
 * hipbp_derive_prover_scalars: the derivation alone, into sL[count*n], sR[count*n], rnd[count*4]
 * (hipbp_prove_input's layout); asynchronous on `stream`.  n: power of two, 1..128; count <= 2^22;
 * a bad n, count or a null pointer gives HIPBP_ERR_ARG and writes nothing. */
int hipbp_derive_prover_scalars(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                size_t count, size_t n, fe25519* sL, fe25519* sR, fe25519* rnd, void* stream);
/* hipbp_batch_generate_range_proof / _gens with derived scalars: in->sL, in->sR, in->rnd must be
 * NULL (anything else: HIPBP_ERR_ARG, nothing written).  The scalars are derived into a workspace
 * kept per (device, stream) (count (2n + 5) * 32 bytes: the scalars and the per-proof keys;
 * hipbp_release_stream_workspaces frees it), then the explicit prover runs on them unchanged: the
 * same bits as hipbp_derive_prover_scalars followed by the explicit call, the same argument
 * checks, limits and valid = 0 zeroed proof.  Asynchronous on `stream`. */
int hipbp_batch_generate_range_proof_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                            const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                                            hipbp_proof_out* out, void* stream);
int hipbp_batch_generate_range_proof_seeded_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                 uint64_t index_base, void* gens, hipbp_proof_out* out, void* stream);
/* ---- accepted prover (no reference counterpart): the seeded prover, re-proving on the GPU what the
 * verifier rejects.  The reference's arithmetic makes its own verifier reject a share of honest
 * proofs (about one in ten at n = 64), and the rejection depends on the nonces, so each rejected
 * proof is proved again with the scalars of its next try key, byte-exact and little-endian:
 *   key_{p,0} = key_p
 *   key_{p,a} = SHA-256("hipbpProverTryV1" || key_p || LE32(a))        a >= 1 (52 bytes)
 *   scalar(p, a, slot) = the seeded prover's scalar of `slot` under key_{p,a} in place of key_p
 * Attempt a of proof p depends only on (seed, v_p, gamma_p, index_base + p, n, a), never on the
 * batch, so a batch cut into several calls yields the single call's proofs and attempts.  The try
 * key is derived from the secret key_p alone: no new secret, no nonce reused between attempts.
 *
 * Round 1 is hipbp_batch_generate_range_proof_seeded into `out` (attempt 0), then the one-shot
 * batched verify of `out` (check 1: cuda_range_proof_verify semantics, as
 * hipbp_batch_range_proof_verify; check 2: range_proof_verify semantics, as
 * hipbp_batch_range_proof_verify_std; V = the proof's own V).  Rounds 2 .. max_attempts (1..16)
 * prove the rejected proofs again (attempt index round - 1), verify them, and write each new proof
 * over its row of `out`.  The loop ends when nothing is rejected or after max_attempts rounds.
 * attempts[p] (DEVICE, [count]) = k >= 1: proof p was accepted at its k-th attempt and `out` holds
 * that proof (the scalars of key_{p,k-1}).  attempts[p] = 0: valid[p] = 0, the value was refused
 * (the zeroed proof, never retried), or valid[p] = 1, not accepted within max_attempts (`out`
 * holds the last attempt's proof).  With max_attempts = 1 the output is the seeded prover's, with
 * the verifier's verdicts in attempts.
 *
 * SYNCHRONOUS, unlike the other device calls: after each round the host waits for `stream` and
 * reads the number of rejected proofs to size the next round, so the outputs are complete on
 * return.  The seeded prover's argument checks and limits, made before anything is enqueued (a bad
 * argument, max_attempts or check, or a null attempts: HIPBP_ERR_ARG, nothing written).  A HIP
 * error ends the call with HIPBP_ERR_DEVICE and launches nothing more; `out` and attempts are
 * then undefined.  The retry workspace is kept per (device, stream) and grows with the number of
 * rejected proofs; hipbp_release_stream_workspaces frees it. */
int hipbp_batch_generate_range_proof_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                              int max_attempts, int check, const ge25519* G, const ge25519* H,
                                              const ge25519* g, const ge25519* h, hipbp_proof_out* out,
                                              uint8_t* attempts, void* stream);
/* The same with a generator set: its generators; its prefix tables for the prover in both checks
 * and for the verify in check 1 (where the one-shot verify takes them,
 * hipbp_batch_range_proof_verify_gens); check 2 verifies without tables.  Same bits either way. */
int hipbp_batch_generate_range_proof_accepted_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                   uint64_t index_base, int max_attempts, int check, void* gens,
                                                   hipbp_proof_out* out, uint8_t* attempts, void* stream);
/* hipbp_derive_prover_scalars for chosen attempts: proof p's scalars under key_{p, attempt[p]}
 * (attempt: DEVICE [count], 0-based; NULL: all 0, hipbp_derive_prover_scalars itself).  With
 * attempt[p] = max(attempts[p], 1) - 1 these are the scalars the accepted prover's output was
 * proved with.  Asynchronous on `stream`; the same checks. */
int hipbp_derive_prover_scalars_at(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                   const uint8_t* attempt, size_t count, size_t n, fe25519* sL, fe25519* sR,
                                   fe25519* rnd, void* stream);
/* What the calling thread's last accepted call did (for benchmarks): its rounds, the proofs proved
 * in each (proved[16]; proved[0] = count) and, when HIPBP_ACCEPT_TIMING=1 was set, the HIP-event
 * times in ms of the loop's own kernels summed over the rounds (kernel_ms[3]: k_try_keys,
 * k_accept_select's launches, k_accept_scatter).  Any pointer may be NULL. */
int hipbp_accepted_last_stats(int* rounds, uint32_t* proved, float* kernel_ms);
/* The seeded prover on host data: proofs[i] = the proof of (v[i], gamma[i]) under seed32 at index
 * index_base + i, for i < count, with the bytes the device call gives.  Host pointers, synchronous,
 * on the calling thread's current device.  n: power of two, 1..128, G->length = H->length = n.
 * valid[i] = 1: proofs[i] is filled as hipbp_inner_product_prove_host fills its proof (ip_proof.n = n,
 * a and b of length 1, L and R of L_len = log2 n, all malloc'ed, so the reference's range_proof_free
 * frees them).  valid[i] = 0 (validate_range_input refused the value): the reference's zeroed proof
 * (V, A, S, T1, T2 identity; taux, mu, t 0) with ip_proof all zero (NULL vectors: freeing is safe).
 * Large counts go through in chunks (HIPBP_PROVE_HOST_CHUNK proofs, default 16384) that alternate
 * over the engine's two streams, each chunk with its own index_base.  On an error nothing stays
 * allocated and every proofs[i] is zero.  It is hipbp_batch_generate_range_proof_host_sharded at
 * num_gpus = 1. */
int hipbp_batch_generate_range_proof_host(RangeProof* proofs, uint8_t* valid, const fe25519* v, const fe25519* gamma,
                                          size_t count, size_t n, const PointVector* G, const PointVector* H,
                                          const ge25519* g, const ge25519* h, const uint8_t seed32[32],
                                          uint64_t index_base);
/* The same, split over several devices; the bytes do not depend on the split.  num_gpus as in
 * hipbp_batch_range_proof_verify_host: <= 0 all visible devices; more than are visible HIPBP_ERR_ARG
 * ("num_gpus = K but N HIP device(s) visible"), nothing written.  Shard d proves the contiguous block
 * [count d / ng, count (d + 1) / ng) with index_base + its first index (mod 2^64) on device
 * (current + d) mod the device count, in a host thread of its own (an empty block starts none; a
 * call of one shard runs it on the caller's thread), so num_gpus = 1 stays on the caller's device;
 * the caller's current device is restored on return.
 * Inside a shard the chunks are as above.  HIPBP_HOST_SHARDS=k, read only when num_gpus <= 0: k
 * shards (at most 64, at most one per proof), shard d on device (current + d) % the device count;
 * shards that share a device run one after another.  Argument errors (a null pointer, a bad n,
 * G->length != n, too many GPUs) write nothing; count = 0 returns HIPBP_OK.  A failure in any shard
 * (a HIP error, a failed malloc) is reported as "device d: ..." after every thread was joined: every
 * vector handed out in every shard is freed and proofs and valid are zero throughout. */
int hipbp_batch_generate_range_proof_host_sharded(RangeProof* proofs, uint8_t* valid, const fe25519* v,
                                                  const fe25519* gamma, size_t count, size_t n, const PointVector* G,
                                                  const PointVector* H, const ge25519* g, const ge25519* h,
                                                  const uint8_t seed32[32], uint64_t index_base, int num_gpus);
/* The accepted prover on host data: proofs[i], valid[i] and attempts[i] (HOST, [count]) are what
 * hipbp_batch_generate_range_proof_accepted gives for the same inputs, index_base, max_attempts
 * (1..16) and check (1 or 2).  attempts[i] = k >= 1: accepted at the k-th attempt, the struct holds
 * that proof.  attempts[i] = 0 with valid[i] = 0: a refused value, the zeroed proof with an all-zero
 * ip_proof; with valid[i] = 1: not accepted within max_attempts, the struct holds the last
 * attempt's proof.  Filled structs are as hipbp_batch_generate_range_proof_host leaves them.
 * Synchronous; num_gpus, the split, HIPBP_HOST_SHARDS, the argument errors (also max_attempts,
 * check, a null attempts) and the failure behaviour (attempts zeroed too) as in _host_sharded.
 * A shard runs ONE accepted device call per chunk of HIPBP_PROVE_HOST_ACCEPT_CHUNK proofs (default
 * 65536, at most 2^22: the retry rounds' fixed cost is per call) and brings a chunk's output to the
 * host in pieces of HIPBP_PROVE_HOST_CHUNK proofs through the seeded call's two pinned slots, a
 * piece unpacked while the next one copies.  No prefix tables.  Afterwards
 * hipbp_accepted_last_stats on the calling thread reports the call as a whole: rounds the largest
 * round count of any chunk, proved[r] summed over all shards and chunks. */
int hipbp_batch_generate_range_proof_accepted_host(RangeProof* proofs, uint8_t* valid, uint8_t* attempts,
                                                   const fe25519* v, const fe25519* gamma, size_t count, size_t n,
                                                   const PointVector* G, const PointVector* H, const ge25519* g,
                                                   const ge25519* h, const uint8_t seed32[32], uint64_t index_base,
                                                   int max_attempts, int check, int num_gpus);

/* ---- Pedersen commitments: pedersen_commit (bulletproof_range_proof.h:28,
 * bulletproof_range_proof.cu:277-296) over a batch, bit-exact.  With N the reference's host
 * ge25519_normalize, sm its ge25519_scalarmult over all 256 bits and tobytes its host,
 * canonicalising fe25519_tobytes, for every i < count
 *     out[i] = N( add( N(sm(tobytes(v[i]), g)), N(sm(tobytes(gamma[i]), h)) ) ):
 * the V that hipbp_batch_generate_range_proof writes for the same (v, gamma, g, h) where valid = 1.
 * Unlike the prover there is no validate_range_input: any four limbs are a value, any four a
 * blinding.  g and h are taken as given (Z != 1, T != X Y, limbs >= p), as everywhere in this
 * library, and a zero scalar gives the reference's 256 doublings of the identity, normalized.
 * One lane per scalar multiplication, the blinding terms and the value terms in waves of their own
 * (a 64-bit value's chain is about a quarter of a blinding's, and within each class the lanes are
 * ordered by chain length, longest first, in chunks of 4096 commitments or more; HIPBP_COMMIT_SORT,
 * read at every call: 0 never, 1 in every chunk; the bits are the same), then one lane per
 * commitment.  The
 * path is for batches: a handful of commitments is faster through the reference's CPU function
 * (DESIGN §16 records the crossover).  Large counts run in chunks of HIPBP_COMMIT_CHUNK commitments
 * (read at every call; default 2^20, which makes 256 MB of terms; at most 2^24) one after another
 * on `stream` through the stream's commit workspace, which grows to the largest chunk seen and is
 * freed by hipbp_release_stream_workspaces; count itself is not bounded.
 * All pointers DEVICE memory; asynchronous on `stream`; out must not overlap the inputs.  count = 0
 * returns HIPBP_OK and writes nothing.  A null pointer gives HIPBP_ERR_ARG, writes nothing and
 * enqueues nothing; a HIP error gives HIPBP_ERR_DEVICE with hipbp_last_error. */
int hipbp_batch_pedersen_commit(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, const ge25519* g,
                                const ge25519* h, void* stream);
/* The same with the g and h of a generator set (hipbp_gens_create; any n) and, where the set has
 * prefix tables, the scalar multiplications started from them (the blinding term from row 2n, the
 * value term from row 2n + 1, for a scalar with fewer than `prefix_bits` leading zeros): the same
 * bits.  A null gens, or one created on another device, gives HIPBP_ERR_ARG. */
int hipbp_batch_pedersen_commit_gens(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, void* gens,
                                     void* stream);
/* Checks openings: ok[i] (DEVICE, [count]) = 1 iff all 16 limbs of V[i] equal the commitment of
 * (v[i], gamma[i]) as hipbp_batch_pedersen_commit gives it, else 0: a compare of the stored limbs,
 * not of the points they stand for, so a V that is the same point in other coordinates gives 0.
 * gens NULL: g and h are used; gens non-NULL: the set's g, h and tables, and g, h are ignored (they
 * may be NULL).  Nothing but ok is written.  Errors as above. */
int hipbp_batch_pedersen_open(uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma, size_t count,
                              const ge25519* g, const ge25519* h, void* gens, void* stream);
/* hipbp_batch_pedersen_commit on host data: HOST pointers (g, h single points), synchronous, the
 * same bytes.  The call is split into contiguous blocks over num_gpus devices exactly as
 * hipbp_batch_generate_range_proof_host_sharded splits: num_gpus <= 0 all visible devices; more than
 * are visible HIPBP_ERR_ARG ("num_gpus = K but N HIP device(s) visible"), nothing written; shard d
 * takes [count d / ng, count (d + 1) / ng) on device (current + d) mod the device count in a host
 * thread of its own (a call of one shard runs on the caller's thread); HIPBP_HOST_SHARDS=k is read
 * the same way; the caller's current device is restored on return.  A shard goes through in pieces
 * of one commit chunk, each copied up, committed and copied back on the engine's stream.  No prefix
 * tables.  count = 0 returns HIPBP_OK; a null pointer gives HIPBP_ERR_ARG and writes nothing; a
 * failure in any shard is reported as "device d: ..." after every thread was joined (out may then
 * hold the blocks that finished). */
int hipbp_batch_pedersen_commit_host(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count,
                                     const ge25519* g, const ge25519* h, int num_gpus);

/* ---- prover: the stand-alone inner_product_prove (bulletproof_vectors.h:94,
 * bulletproof_vectors.cu:277-523) for any power-of-two length, batched, bit-exact: the reference's
 * sequential MSM chains and inner products in its order, the ORIGINAL G, H in every round, Q any
 * point, the transcript's 32 bytes as raw limbs, proof.c = the claimed c as given.  Every O(n)
 * piece of a round runs one lane per element or term; only the order-bound addition chains run one
 * lane per chain.  `count` is processed in chunks that alternate over two internal workspaces, the
 * second on an internal side stream (one chunk's chains run under the other's scalar
 * multiplications); the caller's stream waits for it at the end, so the outputs are ready in the
 * caller's stream order.  HIPBP_IPA_WS_MB: the per-workspace budget that sizes a chunk (default 512).
 * All pointers DEVICE memory; asynchronous on `stream`.  A bad n or a null pointer gives
 * HIPBP_ERR_ARG and writes nothing. */
typedef struct {
    size_t count, n;              /* n: power of two, 1..65536 */
    const fe25519 *a, *b;         /* [count*n] */
    const fe25519 *c;             /* [count] the claimed c_in */
    const fe25519 *transcript;    /* [count] 32 initial transcript bytes as 4 LE limbs; NULL = zeros */
} hipbp_ipa_prove_input;
/* Output in the verifier's wire format (ab_len = 1, L_len = log2 n): with P = hipbp_msm_batch(a||b,
 * G||H) it goes straight into hipbp_batch_inner_product_verify.  n = 1: no rounds, a, b copies of
 * the inputs, x = 0. */
typedef struct {
    fe25519 *a, *b, *c, *x;       /* [count]: final length-1 a, b; c = c_in; x = first challenge */
    fe25519 *c_final;             /* nullable: add(0, mul(a, b)) of the final a, b — the c with which the
                                   * reference's verifier accepts (it compares c with <a, b> first) */
    ge25519 *L, *R;               /* [count*log2 n]; may be NULL when n = 1 */
} hipbp_ipa_proof_out;
int hipbp_batch_inner_product_prove(const hipbp_ipa_prove_input* in, const ge25519* G, const ge25519* H,
                                    const ge25519* Q, hipbp_ipa_proof_out* out, void* stream);
/* The same with a generator set's G, H and prefix tables (same n, same device), Q = its h; the same
 * bits as the plain form on those generators. */
int hipbp_batch_inner_product_prove_gens(const hipbp_ipa_prove_input* in, void* gens, hipbp_ipa_proof_out* out,
                                         void* stream);
/* inner_product_prove on the reference's own host structs (host pointers, synchronous, one proof):
 * on a length mismatch or a length that is no power of two it prints the reference's message on
 * stderr and leaves *proof untouched (HIPBP_ERR_ARG); otherwise *proof is filled as the reference
 * leaves it: a, b of length 1, L, R of L_len = log2 n, all malloc'ed, so inner_product_proof_free
 * frees them.  Unlike the reference it does not print the inner products.  A reference user renames
 * the call; the name inner_product_prove itself is not exported (the reference's host code defines
 * it and links against this library). */
int hipbp_inner_product_prove_host(InnerProductProof* proof, const FieldVector* a, const FieldVector* b,
                                   const PointVector* G, const PointVector* H, const ge25519* Q,
                                   const fe25519* c_in, const uint8_t* transcript32 /* NULL = zeros */);

/* ---- compact proof blobs (no reference counterpart): a batch of range proofs as one byte string, to
 * store or send ("HBPC", version 1).  The reference's points are not on a curve, so there
 * is no 32-byte point encoding; but every point its prover writes went through ge25519_normalize (Z
 * limbs (1, 0, 0, 0), T = fe25519_mul(X, Y)) and fix_inner_product_proof leaves a = [t], b = [1],
 * c = t, so Z, T, a, b and c are dropped and recomputed bit for bit.  A proof where any of that does
 * not hold limb for limb (never mod p: a Z of p + 1, a T off in one limb, a b of 1 + p) is stored
 * verbatim, so decode(encode(x)) = x for any limbs.  All integers little-endian, a field element is
 * its four limbs as stored (32 bytes); Lr = L_len, f = 1 when the records carry taux and mu:
 *   0  u8[4] "HBPC"   4  u16 version = 1   6  u16 flags (bit 0 = f, others 0)
 *   8  u32 n         12  u32 ab_len       16  u32 L_len    20  u32 raw_count R    24  u64 count
 *   32 kind[count]   u8: 0 compact, 1 raw; zero-padded to a multiple of 8 bytes
 *      compact area  count slots of S_c bytes; slot i all zero when kind[i] = 1
 *      raw_index[R]  u32, strictly ascending: the proofs of kind 1; zero-padded to a multiple of 8 bytes
 *      raw area      R records of S_r bytes; record j belongs to proof raw_index[j]
 *   compact slot, S_c = 64 (5 + 2 Lr) + 64 + 64 f (0 when ab_len != 1: every proof is then raw):
 *      X | Y of V, A, S, T1, T2, L[0..Lr), R[0..Lr); t, x; taux, mu if f
 *   raw record, S_r = 128 (5 + 2 Lr) + 96 + 64 f + 64 ab_len:
 *      the same points whole; t, c, x; taux, mu if f; a[ab_len]; b[ab_len]
 * n = 64, Lr = 6, f = 1: S_c = 1216 against the 2400 bytes of S_r.  The blob is a function of the
 * proofs alone: the CPU and the GPU encoder give identical bytes.  Limits: count <= 2^22, n a power of
 * two <= 65536, L_len <= log2 n, ab_len >= 1.  The V encoded is the batch's Vp when non-NULL, else V. */
typedef struct {
    size_t count, n, ab_len, L_len;
    unsigned flags;      /* bit 0: the records carry taux and mu */
    size_t raw_count;    /* R */
    size_t bytes;        /* the blob's exact size */
} hipbp_proof_blob_info;
/* The size of a blob of `count` proofs when every one is raw: what an encoder's buffer must hold. */
size_t hipbp_proof_blob_bound(size_t count, size_t ab_len, size_t L_len, unsigned flags);
/* Validates a HOST copy of a blob's 32 header bytes (magic, version, flags, the limits, R <= count)
 * and that the sections the header implies make exactly blob_bytes; fills *info.  For blobs that
 * live in device memory: hipbp_batch_proof_decode takes the info.  HIPBP_ERR_ARG with a message. */
int hipbp_proof_blob_header(const uint8_t* header32, size_t blob_bytes, hipbp_proof_blob_info* info);
/* Fully validates a HOST blob: the header as above, every kind <= 1, R equal to the number of kind-1
 * bytes, raw_index strictly ascending and naming exactly those proofs, zero padding and zero slots
 * of raw proofs.  Anything wrong: HIPBP_ERR_ARG with a message, *info undefined.  No HIP call. */
int hipbp_proof_blob_parse(const uint8_t* blob, size_t bytes, hipbp_proof_blob_info* info);
/* Encodes a device batch into blob_dev (DEVICE, 8-byte aligned, `cap` bytes) and writes the blob's
 * size to *bytes_out_dev (DEVICE).  with_blinding != 0 (f = 1) needs the batch's taux and mu.
 * Three launches: classify (one lane per point), a one-block scan of the per-block raw counts, and
 * the write (compact slots, the raw proofs ranked in index order, padding, header); no step's
 * result depends on timing.  A cap below hipbp_proof_blob_bound, a bad shape or a null pointer give
 * HIPBP_ERR_ARG and enqueue nothing.  count = 0 gives the 32-byte header.  Asynchronous on `stream`;
 * the block counts live in a workspace kept per (device, stream), freed by
 * hipbp_release_stream_workspaces. */
int hipbp_batch_proof_encode(const hipbp_proof_batch* batch, int with_blinding, uint8_t* blob_dev, size_t cap,
                             uint64_t* bytes_out_dev, void* stream);
/* Decodes a DEVICE blob (8-byte aligned) whose header the host validated into *info
 * (hipbp_proof_blob_header) into out's arrays (hipbp_proof_out's layout with a, b of count ab_len
 * elements and L, R of count L_len; out->valid is ignored; taux, mu may be NULL when f = 0; c is
 * written).  One launch over the compact slots (T recomputed), one over the R raw records.  Every
 * index read from the blob is checked against the header and info->bytes before use; a record that
 * fails is skipped and counted: *bad_dev (DEVICE, set by the call) = the number skipped, 0 for a
 * blob hipbp_proof_blob_parse accepts.  Asynchronous on `stream`. */
int hipbp_batch_proof_decode(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, hipbp_proof_out* out,
                             uint32_t* bad_dev, void* stream);
/* The encoder on the reference's host structs, on the CPU: no HIP call, no device needed; the bytes
 * are the device encoder's.  The first proof sets ab_len (a.length) and L_len; a proof of another
 * shape, or with b.length != a.length, L or R shorter than L_len, or a missing vector, gives
 * HIPBP_ERR_ARG naming its index, as does a cap below hipbp_proof_blob_bound; nothing is written
 * then.  with_blinding != 0 stores each proof's taux and mu.  *bytes = the blob's size. */
int hipbp_proofs_encode_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* blob,
                             size_t cap, size_t* bytes);
/* The decoder into host structs, on the CPU: parses the blob (hipbp_proof_blob_parse), then fills
 * proofs[0 .. count) as hipbp_batch_generate_range_proof_host leaves valid proofs: ip_proof.n = n, a
 * and b of ab_len, L and R of L_len, all malloc'ed, so range_proof_free frees them; taux and mu are
 * zero when f = 0.  On any error nothing stays allocated; every struct is zero, except where the blob
 * does not parse: its count is not known then and proofs is left untouched. */
int hipbp_proofs_decode_host(const uint8_t* blob, size_t bytes, RangeProof* proofs);
/* Verifies a HOST blob on the GPU(s), uploading the blob's bytes instead of the structs'.
 * check 1: cuda_range_proof_verify semantics, ok[i] = hipbp_batch_range_proof_verify_host on the
 * decoded structs; check 2: range_proof_verify semantics (needs f = 1 and g), ok[i] =
 * hipbp_batch_range_proof_verify_std on the decoded batch.  V (HOST, [count]) is the caller's V
 * argument; NULL: each proof's own V.  The blob is parsed on the host before anything is uploaded;
 * n != the header's n, a shape the pipelines cannot take, a bad check: HIPBP_ERR_ARG, nothing
 * verified.  Sharding as hipbp_batch_range_proof_verify_host (contiguous blocks over num_gpus,
 * HIPBP_HOST_SHARDS, the device restored, errors as "device d: ...").  Per 1024-proof chunk a shard
 * uploads that chunk's kind bytes, its compact slots and its raw records (found by binary search in
 * raw_index), decodes them on the chunk's stream into a flat device chunk and pushes it, alternating
 * over two pipelines.  check 1 uses the cached host prefix tables (HIPBP_HOST_PREFIX_BITS) as
 * _verify_host does; check 2 runs without tables.  Synchronous. */
int hipbp_batch_range_proof_verify_bytes_host(const uint8_t* blob, size_t bytes, const ge25519* V, size_t n,
                                              const PointVector* G, const PointVector* H, const ge25519* g,
                                              const ge25519* h, int check, int num_gpus, uint8_t* ok);

/* ---- Proof ids and a batch Merkle root: a name for a proof, a fingerprint for a batch,
 * computed where the proofs are.  A proof's record is what an "HBPC" version 1 blob stores for it (above):
 * its compact slot when the encoder classifies it compact (kind 0), else its raw record (kind 1), with
 * the encoder's V (the batch's Vp when non-NULL, else V).  All integers little-endian:
 *   hdr  = "hipbpProofIdV1" (14 bytes) | u8 kind | u8 f | u32 n | u32 ab_len | u32 L_len | u32 0      (32 bytes)
 *   id   = SHA-256(hdr | record)
 *   leaf = SHA-256(0x00 | id)      node = SHA-256(0x01 | left | right)
 *   root(ids[0 .. count)) = RFC 6962 §2.1 MTH with the ids as the leaf inputs; count = 0: SHA-256("")
 * kind and f are hashed: a proof has one id without its blinding scalars (f = 0) and another with
 * them.  The tree is built level by level: nodes (2k, 2k + 1) are paired, an unpaired last node moves
 * up unchanged (the same tree as the RFC's recursive split).  The audit path of leaf `index` is RFC
 * 6962 §2.1.1 PATH, bottom-up: at each level no entry if the node is the level's unpaired last one,
 * else its sibling; at most 22 entries for count <= 2^22.  The ids of a batch, of its blob, on the
 * GPU and on the CPU are the same bytes.
 *
 * The ids of a device batch: ids_dev (DEVICE, 4-byte aligned, [count * 32]) and, when kind_dev is not
 * NULL, each proof's kind (DEVICE, [count]).  One launch, one lane per proof: classify, then hash
 * the record from the flat arrays.  The encoder's limits and checks: a bad shape, with_blinding
 * without taux and mu, or a null pointer give HIPBP_ERR_ARG, write nothing and enqueue nothing.
 * count = 0 is a no-op.  Asynchronous on `stream`. */
int hipbp_batch_proof_ids(const hipbp_proof_batch* batch, int with_blinding, uint8_t* ids_dev, uint8_t* kind_dev,
                          void* stream);
/* The ids of the proofs of a DEVICE blob (8-byte aligned) whose header the host validated into *info
 * (hipbp_proof_blob_header), as hipbp_batch_proof_decode takes it.  One lane per proof: its kind byte,
 * then its compact slot or the raw record raw_index names for it (binary search).  Every index read
 * from the blob is checked against the header and info->bytes before use, by the decoder's rules; a
 * record that fails gets an all-zero id and is counted: *bad_dev (DEVICE, 4-byte aligned, set by the
 * call) = the number that failed, 0 for a blob hipbp_proof_blob_parse accepts.  The per-block counts
 * live in a workspace kept per (device, stream), freed by hipbp_release_stream_workspaces.
 * HIPBP_ERR_ARG enqueues nothing.  Asynchronous on `stream`. */
int hipbp_blob_proof_ids(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, uint8_t* ids_dev, uint32_t* bad_dev,
                         void* stream);
/* root_dev (DEVICE, 4-byte aligned, [32]) = the Merkle root over ids_dev (DEVICE, 4-byte aligned,
 * [count * 32]); count <= 2^24, count = 0 gives SHA-256("").  One launch per level, one lane per node
 * of the level above (level 0 fused with the leaf hash); the levels alternate between two buffers of
 * a workspace kept per (device, stream), grow-only, freed by hipbp_release_stream_workspaces.  A
 * multi-GPU caller concatenates its shards' ids.  HIPBP_ERR_ARG enqueues nothing.  Asynchronous on
 * `stream`. */
int hipbp_merkle_root(const uint8_t* ids_dev, size_t count, uint8_t* root_dev, void* stream);
/* The same ids from the reference's host structs, on the CPU: no HIP call, no device needed.
 * hipbp_proofs_encode_host's checks: the first proof sets ab_len and L_len; a proof of another shape,
 * or with inconsistent vector lengths, gives HIPBP_ERR_ARG naming its index, nothing written.  ids
 * (HOST, [count * 32]).  count = 0 is a no-op.  The proofs are split over HIPBP_HOST_THREADS threads
 * (unset: the machine's, 16 at most; at least 256 proofs a thread), as are hipbp_blob_proof_ids_host's. */
int hipbp_proof_ids_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* ids);
/* ... and from a HOST blob, which is parsed fully first (hipbp_proof_blob_parse): a malformed blob
 * gives HIPBP_ERR_ARG with the parser's message, nothing written.  ids (HOST, [count * 32]). */
int hipbp_blob_proof_ids_host(const uint8_t* blob, size_t bytes, uint8_t* ids);
/* The root, an audit path and its check, on the CPU.  _path_host: path (HOST, room for 22 entries of
 * 32 bytes) and *path_len for leaf `index` < count <= 2^22.  _verify_host recomputes the root from
 * (id, index, count, path) and returns 1 only if it consumes exactly path_len entries and arrives at
 * `root`; 0 otherwise, also for index >= count or a null pointer. */
int hipbp_merkle_root_host(const uint8_t* ids, size_t count, uint8_t root[32]);
int hipbp_merkle_path_host(const uint8_t* ids, size_t count, size_t index, uint8_t* path, size_t* path_len);
int hipbp_merkle_verify_host(const uint8_t id[32], size_t index, size_t count, const uint8_t* path, size_t path_len,
                             const uint8_t root[32]);

/* Canonical-tree MSM on device buffers.  Asynchronous on `stream`; the MSM, MSM-batch
 * and point-tree calls keep one workspace per (device, stream), so calls on different streams may
 * run concurrently. */
int hipbp_msm(ge25519* result, const fe25519* scalars, const ge25519* points, size_t n, void* stream);

/* count independent canonical-tree MSMs of n points each over the SAME points (e.g. the IPA
 * commitments P = MSM(a||b, G||H) of a batch of proofs): scalars
 * [count*n] (MSM k = rows k*n .. k*n+n-1), points [n], results [count]; each result is bit-exact
 * with hipbp_msm on its rows.  Device buffers. */
int hipbp_msm_batch(ge25519* results, const fe25519* scalars, const ge25519* points, size_t n, size_t count,
                    void* stream);

/* hipbp_msm_batch over a generator set's G||H (2n points, hipbp_gens_create) with its fixed-base
 * prefix tables: each point's scalar multiplication starts from the table entry of its scalar's
 * top K bits, so every result has hipbp_msm_batch's bits with fewer point operations.  scalars
 * [count*2n] (MSM k = rows k*2n .. k*2n+2n-1, the a||b of an IPA commitment P), results [count]. */
int hipbp_msm_batch_gens(ge25519* results, const fe25519* scalars, const void* gens, size_t count, void* stream);

/* Pippenger bucket MSM with window_bits-bit windows (4..12; BASELINE configs[2] names 12), over
 * the same fe25519/ge25519 arithmetic, on device buffers.  A LABELLED ALTERNATIVE, not a drop-in
 * for cuda_point_vector_multi_scalar_mul: the reference's MSM bits come from per-point
 * double-and-add + the canonical tree (hipbp_msm), and this arithmetic is not associative, so a
 * bucket regrouping yields different bits.  Its own result is fixed (stable bucket order, fixed
 * trees) and equals the C restatement oracle/bp_oracle.c orc_msm_pippenger.  Asynchronous: the
 * host does not wait (the bucket-tree depth is read on the device); the Horner chain runs on an
 * internal side stream that the caller's stream waits on, so the result is ready in the caller's
 * stream order.  Workspaces are per (device, stream): MSMs on different streams run concurrently.
 * No reference counterpart. */
int hipbp_msm_pippenger(ge25519* result, const fe25519* scalars, const ge25519* points, size_t n,
                        int window_bits, void* stream);
/* count Pippenger MSMs over the SAME n device points in one call: results[m] = hipbp_msm_pippenger
 * of scalars[m n .. m n + n) (bit for bit).  One sort, one set of bucket-tree launches and one
 * Horner launch serve all of them, so the latency-bound chains are shared.  count <= 65535. */
int hipbp_msm_pippenger_batch(ge25519* results, const fe25519* scalars, const ge25519* points, size_t n,
                              size_t count, int window_bits, void* stream);
/* The two halves of hipbp_msm_pippenger, for a multi-GPU MSM that splits the windows over the
 * ranks (cudabulletproof_amd/shard.py sharded_msm_pippenger).  _windows writes the
 * window sums S_w, w in [w_begin, w_end), into window_sums[w] (W = ceil(256 / window_bits)
 * entries; the others are left untouched), each with the bits the single call forms; _horner
 * runs the Horner chain over all W sums of each of count MSMs (window_sums[m W .. m W + W)), so
 * every rank that holds all sums gets hipbp_msm_pippenger's result bit for bit.  Device buffers,
 * asynchronous on `stream`. */
int hipbp_msm_pippenger_windows(ge25519* window_sums, const fe25519* scalars, const ge25519* points, size_t n,
                                int window_bits, int w_begin, int w_end, void* stream);
int hipbp_msm_pippenger_horner(ge25519* results, const ge25519* window_sums, size_t count, int window_bits,
                               void* stream);
/* Canonical tree over n device points: for stride 1, 2, 4, ...: T[i] = Ndev(T[i] + T[i+stride])
 * for i % (2 stride) == 0 and i + stride < n; result = T[0] (the reduction half of
 * cuda_bulletproof_kernels.cu:45-115).  hipbp_msm = this tree over the per-point
 * terms; a multi-GPU MSM combines per-rank shard roots with it. */
int hipbp_point_tree(ge25519* result, const ge25519* points, size_t n, void* stream);
/* Elementwise device field ops: op 0 add, 1 sub, 2 mul, 3 square (reference kernel quirk),
 * 4 SoA add (limbwise, no carry), 5 invert (host chain), 6 the product fold alone on the
 * 512-bit t = a || b (fe25519_mul's reduction, curve25519_ops.cu:114-145), 7 fe25519_sq,
 * 8 / 9 the sum / difference of the fused add-and-sub block the lane-quad forms use (the same
 * values as ops 0 / 1), 10 fe25519_mul formed as the drain forms' quad-split product (fe_mul_q4:
 * four lanes per element, the same value as op 2), 11 fe25519_mul(a, k) for the curve constant k
 * (fe_mul_k: only provably possible carries counted; the same value as op 2 with b = k; b unused),
 * 12 the same split over a lane quad (fe_mul_q4_k, four lanes per element); the 16-lane row step's
 * field blocks (same values as ops 0 / 8 / 9 / 6): 13 add, 15 / 16 add-sub, 19 fold in their latency
 * forms, and 14, 17 / 18, 20 the same through their deferred rare-edge test (fast form, recomputed
 * when the element's test words hit 2^32-1); the lane loops' deferred forms, each recomputed with
 * the gated form when the element's running words report an edge or a failed product gate: 21 add,
 * 22 / 23 add-sub, 24 fold, 25 mul, 26 sq (b unused), 27 sub (same values as ops 0, 8 / 9, 6, 2, 7, 1). */
int hipbp_field_op(int op, fe25519* r, const fe25519* a, const fe25519* b, size_t count, void* stream);
/* The verify path's SHA-256 message shapes on the device, item i over in[6i .. 6i+5] (device
 * pointers): kind 0 the y challenge (points (in0,in1), (in2,in3), (in4,in5) as X, Y), 1 z (in0),
 * 2 x (points (in0,in1), (in2,in3)), 3 an inner-product round challenge (transcript in0, L.X in1,
 * R.X in2), 4 the prover's IPA transcript start (t in0, taux in1, mu in2), 5 the unmasked digest of
 * in0..in3 in raw limb order.  For checking against FIPS 180-4 (bulletproof_challenge.cu:6-77). */
int hipbp_sha_probe(int kind, fe25519* out, const fe25519* in, size_t count, void* stream);
/* out[i] = ge25519_scalarmult(scalars[i], points[i]) as the raw extended point, through the call site
 * every kernel uses (device pointers).  force != 0: the loops' deferred pass reports a hit after its
 * first chunk of steps whatever the data, so the call takes the recovery path (the rerun with the
 * gated forms); the results are the same bits either way.  For tests. */
int hipbp_sm_probe(int force, ge25519* out, const fe25519* scalars, const ge25519* points, size_t count, void* stream);
/* The same function through the drain-tick forms, by the calls the verify kernels make: form takes
 * HIPBP_QUAD's values, 1 a lane quad per item (sm_quad), 2 a lane pair (sm_pair), 3 a 16-lane row (sm_row,
 * the form of every cuda_range_proof_verify call); no prefix table.  Item i occupies lanes [L i, L i + L) of
 * the grid, L = 4, 2, 16, its scalar and point replicated over them; the items past count in the last wave
 * stay out whole.  force = 1 (form 3 only): every step of every chain takes the row step's deferred
 * recompute whatever the data; the results are the same bits either way.  Any other form or force, and
 * force = 1 with form 1 or 2, is HIPBP_ERR_ARG with a message and launches nothing; count = 0 is a no-op.
 * For tests. */
int hipbp_sm_form_probe(int form, int force, ge25519* out, const fe25519* scalars, const ge25519* points, size_t count,
                        void* stream);
/* Frees every workspace the library caches for `stream` on the current device (canonical MSM /
 * point-tree, prover, the Pedersen commitments' terms, the seeded prover's scalars and keys, the accepted prover's retry workspace, the proof blob encoder's block counts, the proof ids' and Merkle root's level buffers and bad counts, one-shot verify pipelines, the Pippenger workspace pair and the IPA prover's
 * workspace pair, each with its side stream and events), after waiting for the stream.  Workspaces otherwise live as long as the process;
 * a caller that makes short-lived streams calls this before destroying one.  No reference
 * counterpart. */
int hipbp_release_stream_workspaces(void* stream);
/* Wait for `stream`. */
int hipbp_sync(void* stream);

/* Per-kernel HIP-event timing of the verify pipeline (on the stream the kernels run on).
 * enable(1) resets the accumulators; collect() waits for the recorded events and returns,
 * per kernel kind, the summed launch durations (ms) and the launch counts. */
int hipbp_timing_enable(int on);
int hipbp_timing_collect(double* total_ms, uint64_t* launches);
int hipbp_kernel_count(void);
const char* hipbp_kernel_name(int kind);

#ifdef __cplusplus
}
#endif
#endif

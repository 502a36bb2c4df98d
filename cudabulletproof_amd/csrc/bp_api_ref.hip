// bp_api_ref.hip — Part 1 of the C ABI (include/cudabulletproof_hip.h): the reference's surface.
//   cuda_point_vector_multi_scalar_mul / _shared
//   cuda_field_vector_inner_product / _shared, cuda_batch_field_vector_inner_product
//   cuda_batch_field_add / _sub / _mul / _mul_karatsuba / _square / _invert, cuda_soa_field_add
//   cuda_range_proof_verify, cuda_inner_product_verify
//   hipbp_inner_product_prove_host
//   cuda_benchmark_multi_scalar_mul / _inner_product / _field_operations / _range_proof
// It keeps the reference's cuda_bulletproof.h conventions: host buffers in, result out, synchronous
// on the engine's own stream, stderr message + early return on a length mismatch, stderr message +
// exit(EXIT_FAILURE) on a device error (CUDA_CHECK, cuda_bulletproof_kernels.cu:13-21).
#include <chrono>

#include "bp_engine.h"

using namespace bpe;

// Stage one proof (host structs) into the engine's device staging buffers as a batch of 1.
static bool stage_single(Engine& e, const InnerProductProof* ip, const RangeProof* rp, const ge25519* V,
                         hipbp_proof_batch* b) {
    size_t abl = ip->a.length, Lr = ip->L_len;
    if (ip->b.length != abl || abl == 0 || ip->L.length < Lr || ip->R.length < Lr) return false;
    const bp::ChunkLayout lay{1, abl, Lr};
    const size_t bytes = lay.bytes();
    BP_EXIT_ON(e.proof1.need(bytes));
    BP_EXIT_ON(e.need_pinned(bytes));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));   // previous user of the staging buffer is done
    lay.pack(e.pinned.p, 0, *ip, rp, V);
    BP_EXIT_ON(hipMemcpyAsync(e.proof1.p, e.pinned.p, bytes, hipMemcpyHostToDevice, e.stream));
    lay.view(e.proof1.p, b);
    return true;
}

bool bpe::verify_single(const InnerProductProof* ip, const RangeProof* rp, const ge25519* V, const ge25519* P,
                        size_t n, const PointVector* G, const PointVector* H, const ge25519* h) {
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    hipbp_proof_batch b;
    memset(&b, 0, sizeof b);
    if (!stage_single(e, ip, rp, V, &b)) return false;
    b.n = n;
    // the packed generators without g (neither semantics reads it), P in g's place
    const size_t cap0 = e.gens1.cap, kb = bp::gens_bytes(n, false), GE = bp::GE;
    BP_EXIT_ON(e.gens1.need(bp::gens_bytes(n) + GE));
    if (e.gens1.cap != cap0) e.single_gens.clear();   // a new buffer (maybe at the old address) holds nothing
    const GenView dg = GenView::at(e.gens1.p, n, false);
    ge25519* dP = (ge25519*)dg.h + 1;
    std::vector<uint8_t>& sg = e.single_gens;
    const bool same = e.single_gens_dev == e.gens1.p && sg.size() == kb &&
                      bp::packed_gens_equal(sg.data(), G->elements, H->elements, h, n);
    if (!same) {   // (every earlier user of dg has finished: each call ends with a stream sync)
        BP_EXIT_ON(hipMemcpyAsync((void*)dg.G, G->elements, n * GE, hipMemcpyHostToDevice, e.stream));
        BP_EXIT_ON(hipMemcpyAsync((void*)dg.H, H->elements, n * GE, hipMemcpyHostToDevice, e.stream));
        BP_EXIT_ON(hipMemcpyAsync((void*)dg.h, h, GE, hipMemcpyHostToDevice, e.stream));
        sg.resize(kb);
        bp::pack_gens(sg.data(), G->elements, H->elements, nullptr, h, n);
        e.single_gens_dev = e.gens1.p;
    }
    if (P) BP_EXIT_ON(hipMemcpyAsync(dP, P, GE, hipMemcpyHostToDevice, e.stream));
    BP_EXIT_ON(e.ok1.need(64));
    int rc = run_verify(e, &b, P ? dP : nullptr, dg, e.ok1.as<uint8_t>(), nullptr, nullptr, rp != nullptr ? 1 : 0,
                        e.stream);
    if (rc == HIPBP_ERR_ARG) {
        fprintf(stderr, "Error: %s\n", g_err.c_str());
        return false;
    }
    if (rc != HIPBP_OK) {
        fprintf(stderr, "HIP error - %s\n", g_err.c_str());
        exit(EXIT_FAILURE);
    }
    uint8_t ok = 0;
    BP_EXIT_ON(hipMemcpyAsync(&ok, e.ok1.p, 1, hipMemcpyDeviceToHost, e.stream));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));
    return ok != 0;
}

extern "C" {

void cuda_point_vector_multi_scalar_mul(ge25519* result, const FieldVector* scalars, const PointVector* points) {
    if (scalars->length != points->length) {   // cuda_bulletproof_kernels.cu:65-68
        fprintf(stderr, "Error: Vector lengths must match for multi-scalar multiplication\n");
        return;
    }
    size_t n = scalars->length;
    if (n == 0) return;
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    BP_EXIT_ON(e.op_a.need(n * sizeof(fe25519)));
    BP_EXIT_ON(e.op_b.need(n * sizeof(ge25519)));
    BP_EXIT_ON(e.op_out.need(sizeof(ge25519)));
    BP_EXIT_ON(hipMemcpyAsync(e.op_a.p, scalars->elements, n * sizeof(fe25519), hipMemcpyHostToDevice, e.stream));
    BP_EXIT_ON(hipMemcpyAsync(e.op_b.p, points->elements, n * sizeof(ge25519), hipMemcpyHostToDevice, e.stream));
    BP_EXIT_ON(msm_run(e, e.op_out.as<bp::ge>(), e.op_a.as<bp::fe>(), e.op_b.as<bp::ge>(), n, 1, e.stream));
    BP_EXIT_ON(hipMemcpyAsync(result, e.op_out.p, sizeof(ge25519), hipMemcpyDeviceToHost, e.stream));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));
}

void cuda_point_vector_multi_scalar_mul_shared(ge25519* result, const FieldVector* scalars,
                                               const PointVector* points) {
    // cuda_bulletproof_kernels.cu:119-138: the n <= 64 shared-memory kernel computes the
    // same canonical tree; larger n delegates to the standard path.
    cuda_point_vector_multi_scalar_mul(result, scalars, points);
}

static void ip_common(fe25519* result, const FieldVector* a, const FieldVector* b, bool force_shared) {
    if (a->length != b->length) {   // cuda_inner_product.cu:100-103
        fprintf(stderr, "Error: Vector lengths must match for inner product\n");
        return;
    }
    size_t n = a->length;
    if (n == 0) return;
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    BP_EXIT_ON(e.op_a.need(n * sizeof(fe25519)));
    BP_EXIT_ON(e.op_b.need(n * sizeof(fe25519)));
    BP_EXIT_ON(e.op_out.need(sizeof(fe25519)));
    BP_EXIT_ON(e.ip_part.need(1024 * sizeof(fe25519)));
    BP_EXIT_ON(hipMemcpyAsync(e.op_a.p, a->elements, n * sizeof(fe25519), hipMemcpyHostToDevice, e.stream));
    BP_EXIT_ON(hipMemcpyAsync(e.op_b.p, b->elements, n * sizeof(fe25519), hipMemcpyHostToDevice, e.stream));
    if (force_shared || n <= 512)
        bp::launch_ip_shared(e.op_out.as<bp::fe>(), e.op_a.as<bp::fe>(), e.op_b.as<bp::fe>(), n, e.stream);
    else
        bp::launch_ip_grid(e.op_out.as<bp::fe>(), e.ip_part.as<bp::fe>(), e.op_a.as<bp::fe>(),
                           e.op_b.as<bp::fe>(), n, e.stream);
    BP_EXIT_ON(hipGetLastError());
    BP_EXIT_ON(hipMemcpyAsync(result, e.op_out.p, sizeof(fe25519), hipMemcpyDeviceToHost, e.stream));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));
}

void cuda_field_vector_inner_product(fe25519* result, const FieldVector* a, const FieldVector* b) {
    ip_common(result, a, b, false);
}

void cuda_field_vector_inner_product_shared(fe25519* result, const FieldVector* a, const FieldVector* b) {
    ip_common(result, a, b, true);
}

void cuda_batch_field_vector_inner_product(fe25519* results, const FieldVector* a_vectors,
                                           const FieldVector* b_vectors, size_t num_vectors) {
    if (num_vectors == 0) return;
    size_t n = a_vectors[0].length;   // cuda_inner_product.cu:306: every vector taken at vector 0's length
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    size_t tot = num_vectors * n;
    BP_EXIT_ON(e.op_a.need(tot * sizeof(fe25519) + 32));
    BP_EXIT_ON(e.op_b.need(tot * sizeof(fe25519) + 32));
    BP_EXIT_ON(e.op_out.need(num_vectors * sizeof(fe25519)));
    for (size_t i = 0; i < num_vectors; i++) {
        BP_EXIT_ON(hipMemcpyAsync(e.op_a.as<fe25519>() + i * n, a_vectors[i].elements, n * sizeof(fe25519),
                                  hipMemcpyHostToDevice, e.stream));
        BP_EXIT_ON(hipMemcpyAsync(e.op_b.as<fe25519>() + i * n, b_vectors[i].elements, n * sizeof(fe25519),
                                  hipMemcpyHostToDevice, e.stream));
    }
    bp::launch_ip_batch(e.op_out.as<bp::fe>(), e.op_a.as<bp::fe>(), e.op_b.as<bp::fe>(), n, num_vectors, e.stream);
    BP_EXIT_ON(hipGetLastError());
    BP_EXIT_ON(hipMemcpyAsync(results, e.op_out.p, num_vectors * sizeof(fe25519), hipMemcpyDeviceToHost, e.stream));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));
}

static void field_common(int op, fe25519* results, const fe25519* a, const fe25519* b, size_t count) {
    if (count == 0) return;
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    BP_EXIT_ON(e.op_a.need(count * sizeof(fe25519)));
    BP_EXIT_ON(e.op_b.need(count * sizeof(fe25519)));
    BP_EXIT_ON(e.op_out.need(count * sizeof(fe25519)));
    BP_EXIT_ON(hipMemcpyAsync(e.op_a.p, a, count * sizeof(fe25519), hipMemcpyHostToDevice, e.stream));
    if (b) BP_EXIT_ON(hipMemcpyAsync(e.op_b.p, b, count * sizeof(fe25519), hipMemcpyHostToDevice, e.stream));
    if (op == 5)
        bp::launch_invert(e.op_out.as<bp::fe>(), e.op_a.as<bp::fe>(), count, e.stream);
    else
        bp::launch_field_op(op, e.op_out.as<bp::fe>(), e.op_a.as<bp::fe>(), e.op_b.as<bp::fe>(), count, e.stream);
    BP_EXIT_ON(hipGetLastError());
    BP_EXIT_ON(hipMemcpyAsync(results, e.op_out.p, count * sizeof(fe25519), hipMemcpyDeviceToHost, e.stream));
    BP_EXIT_ON(hipStreamSynchronize(e.stream));
}

void cuda_batch_field_add(fe25519* r, const fe25519* a, const fe25519* b, size_t count) { field_common(0, r, a, b, count); }
void cuda_batch_field_sub(fe25519* r, const fe25519* a, const fe25519* b, size_t count) { field_common(1, r, a, b, count); }
void cuda_batch_field_mul(fe25519* r, const fe25519* a, const fe25519* b, size_t count) { field_common(2, r, a, b, count); }
void cuda_batch_field_mul_karatsuba(fe25519* r, const fe25519* a, const fe25519* b, size_t count) {
    field_common(2, r, a, b, count);   // cuda_field_ops.cu:73: schoolbook + the same fold == fe25519_mul
}
void cuda_batch_field_square(fe25519* r, const fe25519* in, size_t count) { field_common(3, r, in, nullptr, count); }
void cuda_batch_field_invert(fe25519* r, const fe25519* in, size_t count) { field_common(5, r, in, nullptr, count); }
void cuda_soa_field_add(fe25519* r, const fe25519* a, const fe25519* b, size_t count) { field_common(4, r, a, b, count); }

bool cuda_range_proof_verify(const RangeProof* proof, const ge25519* V, size_t n, const PointVector* G,
                             const PointVector* H, const ge25519* g, const ge25519* h) {
    (void)g;
    const InnerProductProof* ip = &proof->ip_proof;
    if (G->length != ip->n || H->length != ip->n || n != ip->n) {   // crv:140-143 (and rp.cu:658 reads n entries)
        fprintf(stderr, "Error: Vector lengths must match for inner product verification\n");
        return false;
    }
    return verify_single(ip, proof, V, nullptr, n, G, H, h);
}

bool cuda_inner_product_verify(const InnerProductProof* proof, const ge25519* P, const PointVector* G,
                               const PointVector* H, const ge25519* Q) {
    if (G->length != proof->n || H->length != proof->n) {   // crv:140-143
        fprintf(stderr, "Error: Vector lengths must match for inner product verification\n");
        return false;
    }
    return verify_single(proof, nullptr, nullptr, P, proof->n, G, H, Q);
}

// inner_product_prove (bulletproof_vectors.cu:277) on the reference's own host structs: its two
// checks with its messages (the proof is left untouched), then one proof through the batched
// prover on the engine's stream, synchronously; the proof's vectors are malloc'ed as
// inner_product_proof_init / field_vector_copy leave them (a, b of length 1, L, R of log2 n).
int hipbp_inner_product_prove_host(InnerProductProof* proof, const FieldVector* a, const FieldVector* b,
                                   const PointVector* G, const PointVector* H, const ge25519* Q,
                                   const fe25519* c_in, const uint8_t* transcript32) {
    if (!proof || !a || !b || !G || !H || !Q || !c_in) { g_err = "ipa prover: null argument"; return HIPBP_ERR_ARG; }
    if (a->length != b->length || a->length != G->length || a->length != H->length) {   // vectors.cu:288-291
        fprintf(stderr, "Error: Vector lengths must match for inner product proof\n");
        return HIPBP_ERR_ARG;
    }
    const size_t n = a->length;
    if (!is_pow2(n)) {                                                                  // vectors.cu:295-298
        fprintf(stderr, "Error: Inner product proof length must be a power of 2\n");
        return HIPBP_ERR_ARG;
    }
    if (n > MAX_N) { g_err = "ipa prover: n must be a power of two <= 65536"; return HIPBP_ERR_ARG; }
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    const size_t FE = sizeof(fe25519), GE = sizeof(ge25519), Lr = (size_t)log2i(n);
    // device staging: G | H | Q | L | R (points), then a | b | c | transcript | out a, b, c, x
    BP_EXIT_ON(e.ipa_stage.need((2 * n + 1 + 2 * Lr) * GE + (2 * n + 6) * FE));
    ge25519* dG = e.ipa_stage.as<ge25519>();
    ge25519 *dH = dG + n, *dQ = dH + n, *dL = dQ + 1, *dR = dL + Lr;
    fe25519* da = (fe25519*)(dR + Lr);
    fe25519 *db = da + n, *dc = db + n, *dt = dc + 1, *oa = dt + 1;
    hipStream_t s = e.stream;
    BP_EXIT_ON(hipMemcpyAsync(dG, G->elements, n * GE, hipMemcpyHostToDevice, s));
    BP_EXIT_ON(hipMemcpyAsync(dH, H->elements, n * GE, hipMemcpyHostToDevice, s));
    BP_EXIT_ON(hipMemcpyAsync(dQ, Q, GE, hipMemcpyHostToDevice, s));
    BP_EXIT_ON(hipMemcpyAsync(da, a->elements, n * FE, hipMemcpyHostToDevice, s));
    BP_EXIT_ON(hipMemcpyAsync(db, b->elements, n * FE, hipMemcpyHostToDevice, s));
    BP_EXIT_ON(hipMemcpyAsync(dc, c_in, FE, hipMemcpyHostToDevice, s));
    if (transcript32) BP_EXIT_ON(hipMemcpyAsync(dt, transcript32, FE, hipMemcpyHostToDevice, s));
    hipbp_ipa_prove_input in{1, n, da, db, dc, transcript32 ? dt : nullptr};
    hipbp_ipa_proof_out out{oa, oa + 1, oa + 2, oa + 3, nullptr, dL, dR};
    if (ipa_enqueue(e, &in, GenView(dG, dH, nullptr, dQ), &out, s) != HIPBP_OK) {
        fprintf(stderr, "HIP error in inner_product_prove - %s\n", g_err.c_str());
        exit(EXIT_FAILURE);
    }
    fe25519 res[4];
    if (!bp::proof_vectors_alloc(*proof, n, Lr)) {
        fprintf(stderr, "Error: Failed to allocate memory for field vector\n");
        exit(1);
    }
    BP_EXIT_ON(hipMemcpyAsync(res, oa, 4 * FE, hipMemcpyDeviceToHost, s));
    if (Lr) {
        BP_EXIT_ON(hipMemcpyAsync(proof->L.elements, dL, Lr * GE, hipMemcpyDeviceToHost, s));
        BP_EXIT_ON(hipMemcpyAsync(proof->R.elements, dR, Lr * GE, hipMemcpyDeviceToHost, s));
    }
    BP_EXIT_ON(hipStreamSynchronize(s));
    *proof->a.elements = res[0];
    *proof->b.elements = res[1];
    proof->c = res[2];
    proof->x = res[3];
    return HIPBP_OK;
}

// ---- cuda_benchmark_* (declared at cuda_bulletproof.h:81-84, never defined by the reference)
static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void cuda_benchmark_multi_scalar_mul(int iterations, size_t vector_size) {
    std::vector<ge25519> pts(vector_size);
    std::vector<fe25519> sc(vector_size);
    for (size_t i = 0; i < vector_size; i++) {
        memset(&pts[i], 0, sizeof(ge25519));
        for (int k = 0; k < 4; k++) {
            pts[i].X.limbs[k] = 0x9E3779B97F4A7C15ull * (i + 1) ^ k;
            pts[i].Y.limbs[k] = 0xBF58476D1CE4E5B9ull * (i + 7) ^ k;
            sc[i].limbs[k] = 0x94D049BB133111EBull * (i + 3) + k;
        }
        pts[i].Z.limbs[0] = 1;
        sc[i].limbs[3] &= 0x7FFFFFFFFFFFFFFFull;
    }
    FieldVector s = {sc.data(), vector_size};
    PointVector p = {pts.data(), vector_size};
    ge25519 r;
    cuda_point_vector_multi_scalar_mul(&r, &s, &p);
    double t0 = now_s();
    for (int i = 0; i < iterations; i++) cuda_point_vector_multi_scalar_mul(&r, &s, &p);
    double dt = (now_s() - t0) / (iterations > 0 ? iterations : 1);
    printf("cuda_benchmark_multi_scalar_mul: n=%zu  %.3f ms/call  %.1f points/s\n", vector_size, dt * 1e3,
           vector_size / dt);
    fflush(stdout);
}

void cuda_benchmark_inner_product(int iterations, size_t vector_size) {
    std::vector<fe25519> a(vector_size), b(vector_size);
    for (size_t i = 0; i < vector_size; i++)
        for (int k = 0; k < 4; k++) {
            a[i].limbs[k] = 0x9E3779B97F4A7C15ull * (i + 1) + k;
            b[i].limbs[k] = 0xBF58476D1CE4E5B9ull * (i + 5) + k;
        }
    FieldVector av = {a.data(), vector_size}, bv = {b.data(), vector_size};
    fe25519 r;
    cuda_field_vector_inner_product(&r, &av, &bv);
    double t0 = now_s();
    for (int i = 0; i < iterations; i++) cuda_field_vector_inner_product(&r, &av, &bv);
    double dt = (now_s() - t0) / (iterations > 0 ? iterations : 1);
    printf("cuda_benchmark_inner_product: n=%zu  %.3f ms/call\n", vector_size, dt * 1e3);
    fflush(stdout);
}

void cuda_benchmark_field_operations(int iterations, size_t batch_size) {
    std::vector<fe25519> a(batch_size), b(batch_size), r(batch_size);
    for (size_t i = 0; i < batch_size; i++)
        for (int k = 0; k < 4; k++) {
            a[i].limbs[k] = 0x9E3779B97F4A7C15ull * (i + 1) + k;
            b[i].limbs[k] = 0xBF58476D1CE4E5B9ull * (i + 5) + k;
        }
    cuda_batch_field_mul(r.data(), a.data(), b.data(), batch_size);
    const char* names[3] = {"add", "mul", "square"};
    for (int op = 0; op < 3; op++) {
        double t0 = now_s();
        for (int i = 0; i < iterations; i++) {
            if (op == 0) cuda_batch_field_add(r.data(), a.data(), b.data(), batch_size);
            if (op == 1) cuda_batch_field_mul(r.data(), a.data(), b.data(), batch_size);
            if (op == 2) cuda_batch_field_square(r.data(), a.data(), batch_size);
        }
        double dt = (now_s() - t0) / (iterations > 0 ? iterations : 1);
        printf("cuda_benchmark_field_operations: %s x %zu  %.3f ms/call\n", names[op], batch_size, dt * 1e3);
        fflush(stdout);
    }
}

static uint64_t bench_mix(uint64_t x) {   // splitmix64: deterministic benchmark inputs
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// max(iterations, 1) real bit_size-bit range proofs (values < 2^bit_size, random scalars shaped as
// generate_random_scalar, rp.cu:153-159) made by the GPU prover (hipbp_batch_generate_range_proof,
// same bits as generate_range_proof), then verified as the reference's host RangeProof structs:
// one cuda_range_proof_verify call per proof (the reference's per-proof entry point), and once
// more through hipbp_batch_range_proof_verify_host.  One line: per-call latency, batched rate,
// pass count, and whether the two verdict sets agree.
void cuda_benchmark_range_proof(int iterations, size_t bit_size) {
    const size_t n = bit_size;
    if (!is_pow2(n) || n > 64) {
        fprintf(stderr, "cuda_benchmark_range_proof: bit_size must be a power of two <= 64\n");
        return;
    }
    const size_t count = iterations > 0 ? std::min<size_t>((size_t)iterations, 65536) : 1;
    const size_t Lr = (size_t)log2i(n), ng = 2 * n + 2;
    uint64_t st = 0x5EEDull * 1000003 + n;
    auto rnd = [&]() { return bench_mix(st++); };
    // generators G[n] | H[n] | g | h: random X, Y < 2^255, Z = 1, T = X Y (the engine's fe25519_mul)
    std::vector<fe25519> X(ng), Y(ng), T(ng);
    for (size_t i = 0; i < ng; i++)
        for (int k = 0; k < 4; k++) {
            X[i].limbs[k] = rnd() & (k == 3 ? 0x7FFFFFFFFFFFFFFFull : ~0ull);
            Y[i].limbs[k] = rnd() & (k == 3 ? 0x7FFFFFFFFFFFFFFFull : ~0ull);
        }
    cuda_batch_field_mul(T.data(), X.data(), Y.data(), ng);
    std::vector<ge25519> gen(ng);
    for (size_t i = 0; i < ng; i++) {
        memset(&gen[i], 0, sizeof(ge25519));
        gen[i].X = X[i]; gen[i].Y = Y[i]; gen[i].Z.limbs[0] = 1; gen[i].T = T[i];
    }
    auto scalar = [&](fe25519& f) {   // generate_random_scalar's masks: byte 0 &= 0xF8, byte 31 &= 0x7F | 0x40
        for (int k = 0; k < 4; k++) f.limbs[k] = rnd();
        f.limbs[0] &= ~7ull;
        f.limbs[3] = (f.limbs[3] & 0x7FFFFFFFFFFFFFFFull) | 0x4000000000000000ull;
    };
    const size_t FE = sizeof(fe25519), GE = sizeof(ge25519);
    std::vector<fe25519> v(count), gamma(count), sL(count * n), sR(count * n), r4(count * 4);
    for (size_t p = 0; p < count; p++) {
        memset(&v[p], 0, FE);
        v[p].limbs[0] = n == 64 ? rnd() : rnd() & ((1ull << n) - 1);
        scalar(gamma[p]);
        for (size_t i = 0; i < n; i++) { scalar(sL[p * n + i]); scalar(sR[p * n + i]); }
        for (int i = 0; i < 4; i++) scalar(r4[p * 4 + i]);
    }
    Engine& e = engine_or_exit();
    // device: inputs | generators | outputs (bp::OutLayout)
    const bp::OutLayout lay{count, count, Lr, 0};
    const size_t in_b = (count * (2 + 2 * n + 4)) * FE, gen_b = ng * GE, out_b = lay.end();
    uint8_t* d = nullptr;
    BP_EXIT_ON(hipMalloc(&d, in_b + gen_b + out_b));
    fe25519* dv = (fe25519*)d;
    fe25519* dgam = dv + count;
    fe25519* dsL = dgam + count;
    fe25519* dsR = dsL + count * n;
    fe25519* dr4 = dsR + count * n;
    ge25519* dgen = (ge25519*)(d + in_b);
    uint8_t* o = d + in_b + gen_b;
    BP_EXIT_ON(hipMemcpy(dv, v.data(), count * FE, hipMemcpyHostToDevice));
    BP_EXIT_ON(hipMemcpy(dgam, gamma.data(), count * FE, hipMemcpyHostToDevice));
    BP_EXIT_ON(hipMemcpy(dsL, sL.data(), count * n * FE, hipMemcpyHostToDevice));
    BP_EXIT_ON(hipMemcpy(dsR, sR.data(), count * n * FE, hipMemcpyHostToDevice));
    BP_EXIT_ON(hipMemcpy(dr4, r4.data(), count * 4 * FE, hipMemcpyHostToDevice));
    BP_EXIT_ON(hipMemcpy(dgen, gen.data(), gen_b, hipMemcpyHostToDevice));
    hipbp_proof_out po;
    lay.view(o, &po);
    hipbp_prove_input pin{count, n, dv, dgam, dsL, dsR, dr4};
    if (hipbp_batch_generate_range_proof(&pin, dgen, dgen + n, dgen + 2 * n, dgen + 2 * n + 1, &po, nullptr) !=
        HIPBP_OK) {
        fprintf(stderr, "HIP error - %s\n", g_err.c_str());
        exit(EXIT_FAILURE);
    }
    BP_EXIT_ON(hipDeviceSynchronize());
    std::vector<uint8_t> host(out_b);
    BP_EXIT_ON(hipMemcpy(host.data(), o, out_b, hipMemcpyDeviceToHost));
    BP_EXIT_ON(hipFree(d));
    std::vector<RangeProof> proofs(count);
    std::vector<ge25519> V(count);
    for (size_t p = 0; p < count; p++) {
        if (lay.unpack(host.data(), p, n, proofs[p]) < 0) {
            fprintf(stderr, "Error: Failed to allocate memory for field vector\n");
            exit(1);
        }
        V[p] = proofs[p].V;
    }
    PointVector Gv = {gen.data(), n}, Hv = {gen.data() + n, n};
    const ge25519 *g = &gen[2 * n], *h = &gen[2 * n + 1];
    std::vector<uint8_t> ok1(count), ok2(count);
    (void)cuda_range_proof_verify(&proofs[0], &V[0], n, &Gv, &Hv, g, h);   // warm-up (pipeline, tables)
    double t0 = now_s();
    for (size_t p = 0; p < count; p++) ok1[p] = cuda_range_proof_verify(&proofs[p], &V[p], n, &Gv, &Hv, g, h) ? 1 : 0;
    const double dt1 = now_s() - t0;
    if (hipbp_batch_range_proof_verify_host(proofs.data(), V.data(), count, n, &Gv, &Hv, g, h, 1, ok2.data()) !=
        HIPBP_OK) {
        fprintf(stderr, "HIP error - %s\n", g_err.c_str());
        exit(EXIT_FAILURE);
    }
    t0 = now_s();
    BP_EXIT_ON(hipbp_batch_range_proof_verify_host(proofs.data(), V.data(), count, n, &Gv, &Hv, g, h, 1, ok2.data())
                   == HIPBP_OK ? hipSuccess : hipErrorUnknown);
    const double dt2 = now_s() - t0;
    size_t pass = 0, agree = 0;
    for (size_t p = 0; p < count; p++) {
        pass += ok1[p];
        agree += ok1[p] == ok2[p];
        InnerProductProof& ip = proofs[p].ip_proof;
        free(ip.a.elements); free(ip.b.elements); free(ip.L.elements); free(ip.R.elements);
    }
    printf("cuda_benchmark_range_proof: n=%zu  %zu proofs  cuda_range_proof_verify %.3f ms/call  "
           "batched (hipbp_batch_range_proof_verify_host) %.1f verifies/s  passes %zu/%zu  verdicts agree %zu/%zu\n",
           n, count, dt1 / count * 1e3, count / dt2, pass, count, agree, count);
    fflush(stdout);
}

}  // extern "C"

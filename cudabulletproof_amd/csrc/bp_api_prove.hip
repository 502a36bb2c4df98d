// bp_api_prove.hip — the provers of the C ABI (include/cudabulletproof_hip.h) on device data,
// asynchronous on the caller's stream:
//   hipbp_batch_generate_range_proof / _gens
//   hipbp_derive_prover_scalars / _at
//   hipbp_batch_generate_range_proof_seeded / _seeded_gens
//   hipbp_batch_generate_range_proof_accepted / _accepted_gens, hipbp_accepted_last_stats
//   hipbp_batch_pedersen_commit / _commit_gens / _open
//   hipbp_batch_inner_product_prove / _gens
// A _gens entry point is its plain twin's body on the view of a checked generator set.
#include "bp_engine.h"
#include "bp_prove_seed.h"

using namespace bpe;

static int prove_run(const hipbp_prove_input* in, const GenView& gv, hipbp_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (!in || !out || !gv.G || !gv.H || !gv.g || !gv.h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (in->count == 0) return HIPBP_OK;
    if (!is_pow2(in->n) || in->n > 128) { g_err = "prover: n must be a power of two <= 128"; return HIPBP_ERR_ARG; }
    if (in->count > ((size_t)1 << 22)) { g_err = "prover: batch too large"; return HIPBP_ERR_ARG; }
    if (!in->v || !in->gamma || !in->sL || !in->sR || !in->rnd) { g_err = "prover: null input"; return HIPBP_ERR_ARG; }
    if (!out->V || !out->A || !out->S || !out->T1 || !out->T2 || !out->taux || !out->mu || !out->t || !out->c ||
        !out->x || !out->a || !out->b || !out->valid || (in->n > 1 && (!out->L || !out->R))) {
        g_err = "prover: null output";
        return HIPBP_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(e->ensure_two((int)in->n));
    const size_t B = in->count, n = in->n;
    bp::ProveIn pin{(int)B, (int)n, log2i(n), (const bp::fe*)in->v, (const bp::fe*)in->gamma,
                    (const bp::fe*)in->sL, (const bp::fe*)in->sR, (const bp::fe*)in->rnd};
    const bp::ProveOut po = bp::prove_out_of(*out);
    // workspace: the stream's prover buffers (reused across calls on the engine's lock)
    using namespace bp;   // the table's ids and types
    hipStream_t s = pick(stream);
    Buf(&b)[PB_COUNT] = e->streams[s].prove;
    // terms0's heavy-list sort (HIPBP_PROVE_SORT=0 turns it off, for A/B runs: slist, sbins stay null)
    static const bool psort = getenv("HIPBP_PROVE_SORT") ? atoi(getenv("HIPBP_PROVE_SORT")) != 0 : true;
    size_t sz[PB_COUNT];
    prove_sizes(B, n, psort, sz);
    BP_RET_ON(need_all(b, sz));
    bp::ProveWs w{};
    BP_PROVE_BUFS(BP_BUF_FIELD)
    w.cap = prove_cap(B, n);
    w.ptab = gv.tab; w.pbits = gv.bits;
    auto run = [&](int stage, int r) { bp::launch_prove(stage, r, pin, w, po, gv.G, gv.H, gv.g, gv.h, e->dtab, e->two_i, s); };
    run(bp::PS_PREP, 0);
    run(bp::PS_SORT0, 0);
    run(bp::PS_TERMS0, 0);
    // the tail (chain0 .. final: ~20 short dependent launches) on the caller's stream; a side stream,
    // a terms0 gate across streams and other tail schedules were measured and rejected
    run(bp::PS_CHAIN0, 0);
    run(bp::PS_COMMIT, 0);
    run(bp::PS_TERMS1, 0);
    run(bp::PS_TX, 0);
    for (int r = 0; r < pin.L; r++) {
        run(bp::PS_RTERMS, r);
        run(bp::PS_RCHAIN, r);
        run(bp::PS_ROUND, r);
    }
    run(bp::PS_FINAL, 0);
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

// ---- seeded prover (bp_prove_seed.h / .hip): the prover's random scalars derived on the device
// from a 32-byte seed.  seed_check: the shape limits of prove_run, checked before anything is
// enqueued (the derive kernels index with them).
int bpe::seed_check(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, size_t count, size_t n) {
    if (!seed32) { g_err = "seeded prover: null seed"; return HIPBP_ERR_ARG; }
    if (!is_pow2(n) || n > 128) { g_err = "prover: n must be a power of two <= 128"; return HIPBP_ERR_ARG; }
    if (count > ((size_t)1 << 22)) { g_err = "prover: batch too large"; return HIPBP_ERR_ARG; }
    if (!v || !gamma) { g_err = "prover: null input"; return HIPBP_ERR_ARG; }
    return HIPBP_OK;
}

// what the seeded and the accepted prover check of their arguments before anything is enqueued
static int prove_seeded_check(const hipbp_prove_input* in, const uint8_t* seed32, const GenView& gv,
                              const hipbp_proof_out* out) {
    if (!in || !out || !gv.G || !gv.H || !gv.g || !gv.h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (in->sL || in->sR || in->rnd) {
        g_err = "seeded prover: sL, sR and rnd must be NULL (the scalars are derived from the seed)";
        return HIPBP_ERR_ARG;
    }
    return seed_check(seed32, in->v, in->gamma, in->count, in->n);
}

// the seeded prover's derive launches and prover enqueue: arguments checked, count > 0, seed_mu held
static int prove_seeded_locked(Engine* e, const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                               const GenView& gv, hipbp_proof_out* out, void* stream) {
    const size_t B = in->count, n = in->n;
    hipStream_t s = pick(stream);
    bp::fe* scal = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        StreamWs* sb = &e->streams[s];
        BP_RET_ON(sb->seed_keys.need(B * sizeof(bp::fe)));
        BP_RET_ON(sb->seed_scal.need(B * (2 * n + 4) * sizeof(bp::fe)));   // rnd [B*4] | sL [B*n] | sR [B*n]
        scal = sb->seed_scal.as<bp::fe>();
        bp::launch_seed_derive(bp::seed_words(seed32), (const bp::fe*)in->v, (const bp::fe*)in->gamma, index_base,
                               (uint32_t)B, (uint32_t)n, sb->seed_keys.as<bp::fe>(), scal + 4 * B, scal + (4 + n) * B, scal,
                               s);
        BP_RET_ON(hipGetLastError());
    }
    hipbp_prove_input full = *in;
    full.rnd = (const fe25519*)scal;
    full.sL = (const fe25519*)(scal + 4 * B);
    full.sR = (const fe25519*)(scal + (4 + n) * B);
    return prove_run(&full, gv, out, stream);
}

int bpe::prove_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, const GenView& gv,
                      hipbp_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    int rc = prove_seeded_check(in, seed32, gv, out);
    if (rc != HIPBP_OK) return rc;
    if (in->count == 0) return HIPBP_OK;
    std::lock_guard<std::mutex> slk(e->seed_mu);
    return prove_seeded_locked(e, in, seed32, index_base, gv, out, stream);
}

// ---- accepted prover: the seeded prover, the one-shot verify of its proofs, and up to
// max_attempts - 1 retry rounds over the proofs the verifier rejected, each with the scalars of
// the next try key (what the last call on this thread did: g_accept_stats).
// HIP events round the loop's own launches, read after the call's last synchronise
namespace {
struct AcceptClock {
    struct Rec { int kind; hipEvent_t a, b; };
    const bool on;
    hipStream_t s;
    std::vector<Rec> recs;
    AcceptClock(hipStream_t st) : on(getenv("HIPBP_ACCEPT_TIMING") && atoi(getenv("HIPBP_ACCEPT_TIMING")) != 0), s(st) {}
    void begin(int kind) {
        if (!on) return;
        Rec r{kind, nullptr, nullptr};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        (void)hipEventRecord(r.a, s);
        recs.push_back(r);
    }
    void end() { if (on && !recs.empty()) (void)hipEventRecord(recs.back().b, s); }
    void collect(float (&ms)[AK_COUNT]) {
        for (auto& r : recs) {
            float t = 0;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ms[r.kind] += t;
        }
    }
    ~AcceptClock() {
        for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    }
};
}  // namespace

// A generator set's prefix tables serve the prover and the check-1 verify (the one-shot verify takes
// them there, hipbp_batch_range_proof_verify_gens, and does not read g); check 2 reads g and takes none.
int bpe::prove_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, int max_attempts,
                        int check, const GenView& gv, hipbp_proof_out* out, uint8_t* attempts, void* stream) {
    using namespace bp;   // the table's ids and types
    BP_ENGINE_OR_RET(e);
    int rc = prove_seeded_check(in, seed32, gv, out);
    if (rc != HIPBP_OK) return rc;
    if (max_attempts < 1 || max_attempts > 16) { g_err = "accepted prover: max_attempts must be 1..16"; return HIPBP_ERR_ARG; }
    if (check != 1 && check != 2) { g_err = "accepted prover: check must be 1 or 2"; return HIPBP_ERR_ARG; }
    g_accept_stats = AcceptStats{};
    if (in->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!attempts) { g_err = "accepted prover: null attempts"; return HIPBP_ERR_ARG; }
    const size_t B = in->count, n = in->n, Lr = (size_t)log2i(n);
    hipStream_t s = pick(stream);
    AcceptClock clk(s);
    std::lock_guard<std::mutex> slk(e->seed_mu);
    // round 1: the seeded prover's proofs (attempt 0) into the caller's output
    if ((rc = prove_seeded_locked(e, in, seed32, index_base, gv, out, stream)) != HIPBP_OK) return rc;
    const GenView vgv = check == 2 ? gv.with_tables(nullptr, 0) : gv.without_g();
    hipbp_proof_out cur = *out;      // the round's proofs: the caller's output, then the compact workspace
    const uint32_t* src = nullptr;   // their batch indices (null: the whole batch)
    size_t m = B;
    StreamWs* sb = nullptr;
    AcceptWs w{};
    size_t sz[AB_COUNT];
    for (int round = 1;; round++) {
        g_accept_stats.m[round - 1] = (uint32_t)m;
        g_accept_stats.rounds = round;
        {
            std::lock_guard<std::mutex> lk(e->mu);
            sb = &e->streams[s];
            Buf(&b)[AB_COUNT] = sb->accept;
            accept_sizes(m, 0, n, Lr, sz);
            BP_RET_ON(need_all(b, sz));
            BP_RET_ON(sb->accept_cnt.need(sizeof(uint32_t)));
            BP_ACCEPT_BUFS(BP_BUF_FIELD)
            const hipbp_proof_batch bv = batch_of(cur, m, n, Lr);
            if ((rc = run_verify(*e, &bv, nullptr, vgv, w.ok, nullptr, nullptr, check, s)) != HIPBP_OK) return rc;
            clk.begin(AK_SELECT);
            launch_accept_count(w.ok, cur.valid, src, (uint32_t)m, (uint32_t)round, attempts, w.blk, w.cnt, s);
            clk.end();
            if (src) {   // a retry round's proofs, accepted or not, to their rows of the caller's output
                clk.begin(AK_SCATTER);
                launch_accept_scatter(prove_out_of(cur), prove_out_of(*out), src, (uint32_t)m, (uint32_t)Lr, s);
                clk.end();
            }
            BP_RET_ON(hipGetLastError());
            if (round < max_attempts)
                BP_RET_ON(hipMemcpyAsync(sb->accept_cnt.p, w.cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        }
        BP_RET_ON(hipStreamSynchronize(s));
        if (round == max_attempts) break;
        const size_t r = *sb->accept_cnt.as<uint32_t>();
        if (r == 0) break;
        if (r > m) { g_err = "accepted prover: rejected count exceeds the round (internal)"; return HIPBP_ERR_DEVICE; }
        {
            std::lock_guard<std::mutex> lk(e->mu);
            Buf(&b)[AB_COUNT] = sb->accept;
            accept_sizes(0, r, n, Lr, sz);
            BP_RET_ON(need_all(b, sz));
            BP_ACCEPT_BUFS(BP_BUF_FIELD)
            uint32_t* list = w.list[round & 1];
            clk.begin(AK_SELECT);
            launch_accept_fill(w.ok, cur.valid, src, (uint32_t)m, w.blk, (const fe*)in->v, (const fe*)in->gamma, list, w.v,
                               w.gamma, s);
            clk.end();
            clk.begin(AK_TRY_KEYS);
            launch_try_keys_list(sb->seed_keys.as<fe>(), list, (uint32_t)r, (uint32_t)round, w.keys, s);
            clk.end();
            launch_seed_scalars(w.keys, (uint32_t)r, (uint32_t)n, w.scal + 4 * r, w.scal + (4 + n) * r, w.scal, s);
            BP_RET_ON(hipGetLastError());
            src = list;
        }
        // attempt index `round` of the r rejected proofs, into the compact workspace
        hipbp_prove_input cin{r, n, (const fe25519*)w.v, (const fe25519*)w.gamma, (const fe25519*)(w.scal + 4 * r),
                              (const fe25519*)(w.scal + (4 + n) * r), (const fe25519*)w.scal};
        accept_out(r, Lr).view(w.out, &cur);
        if ((rc = prove_run(&cin, gv, &cur, stream)) != HIPBP_OK) return rc;
        m = r;
    }
    clk.collect(g_accept_stats.ms);
    return HIPBP_OK;
}

size_t bpe::env_commit_chunk(size_t count) {
    const char* ce = getenv("HIPBP_COMMIT_CHUNK");
    return bp::commit_chunk(count, ce ? atoll(ce) : 0);
}

// ---- Pedersen commitments (bp_commit.hip): pedersen_commit over a batch.  commit_run enqueues a whole
// call on `s`: chunks of HIPBP_COMMIT_CHUNK commitments (read at every call; bp::commit_chunk), one
// after another through the stream's one commit workspace (a chunk's launches are ordered behind the
// previous chunk's on the stream, so the terms are never overwritten while still read).  V null:
// out[i] = the commitment; else ok[i] = (V[i] == the commitment).
int bpe::commit_run(Engine& e, ge25519* out, uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma,
                    size_t count, const GenView& gv, hipStream_t s) {
    using namespace bp;   // the table's ids and types
    const size_t chunk = env_commit_chunk(count);
    std::lock_guard<std::mutex> lk(e.mu);
    Buf(&b)[CB_COUNT] = e.streams[s].commit;
    size_t sz[CB_COUNT];
    // the chain-length sort of each class's lanes (HIPBP_COMMIT_SORT, read at every call)
    const bool sort = commit_sorted(chunk, getenv("HIPBP_COMMIT_SORT"));
    commit_sizes(chunk, sort, sz);
    for (int k = 0; k < CB_COUNT; k++)   // nothing queued on `s` reads a buffer that grows
        if (sz[k] > b[k].cap && b[k].p) { BP_RET_ON(hipStreamSynchronize(s)); break; }
    BP_RET_ON(need_all(b, sz));
    CommitWs w{};
    BP_COMMIT_BUFS(BP_BUF_FIELD)
    if (!sort) { w.order = nullptr; w.bins = nullptr; }   // (a sorted call may have left them allocated)
    for (size_t c0 = 0; c0 < count; c0 += chunk) {
        const size_t c = std::min(chunk, count - c0);
        const CommitIn in{c, (const fe*)v + c0, (const fe*)gamma + c0, gv.g, gv.h, gv.tab, gv.bits, (int)gv.n};
        launch_commit(in, w, out ? (ge*)out + c0 : nullptr, V ? (const ge*)V + c0 : nullptr, ok ? ok + c0 : nullptr,
                      e.dtab, s);
    }
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

// ---- stand-alone IPA prover (bp_ipa_prove.hip).  The engine's lock is held by the caller.
// `count` is cut into chunks sized from a workspace budget (HIPBP_IPA_WS_MB per workspace, default
// 512: ~1.8 MB per proof at n = 4096) that alternate over two workspaces: even chunks on the
// caller's stream, odd ones on the internal side stream; the caller's stream waits for the side
// stream at the end.  A chunk's chain latency does not depend on its size, so the fewest chunks
// that fit are used (two whenever count >= 2).
int bpe::ipa_enqueue(Engine& e, const hipbp_ipa_prove_input* in, const GenView& gv, const hipbp_ipa_proof_out* out,
                     hipStream_t s) {
    const size_t B = in->count, n = in->n;
    const int Lr = log2i(n);
    using namespace bp;   // the IpaBuf names
    const size_t cap = ipa_cap(n), per_proof = ipa_per_proof(n);
    const char* env = getenv("HIPBP_IPA_WS_MB");
    size_t mb = env ? (size_t)atoll(env) : 512;
    if (mb < 1) mb = 1;
    size_t bmax = std::max<size_t>(1, (mb << 20) / per_proof);
    bmax = std::min(bmax, (size_t)0x7FFFFFFF / cap);   // item ids are 32-bit
    const size_t chunks = std::max((B + bmax - 1) / bmax, std::min<size_t>(B, 2));
    const size_t Bc = (B + chunks - 1) / chunks;
    StreamWs* ib = &e.streams[s];
    if (chunks > 1 && !ib->ipa_side) {
        BP_RET_ON(hipStreamCreateWithFlags(&ib->ipa_side, hipStreamNonBlocking));
        for (auto& ev : ib->ipa_ev) BP_RET_ON(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    size_t sz[IB_COUNT];
    ipa_sizes(Bc, n, sz);
    for (size_t w = 0; w < std::min<size_t>(chunks, 2); w++) BP_RET_ON(need_all(ib->ipa[w], sz));
    if (chunks > 1) {   // the side stream starts after the caller's queued work (the inputs' producers)
        BP_RET_ON(hipEventRecord(ib->ipa_ev[0], s));
        BP_RET_ON(hipStreamWaitEvent(ib->ipa_side, ib->ipa_ev[0], 0));
    }
    const bp::fe *ia = (const bp::fe*)in->a, *ibv = (const bp::fe*)in->b, *ic = (const bp::fe*)in->c,
                 *itr = (const bp::fe*)in->transcript;
    for (size_t c = 0; c < chunks; c++) {
        const size_t p0 = c * Bc;
        if (p0 >= B) break;
        const size_t bc = std::min(Bc, B - p0);
        Buf(&b)[IB_COUNT] = ib->ipa[c & 1];
        hipStream_t st = (c & 1) ? ib->ipa_side : s;
        bp::IpaWs w{};
        BP_IPA_BUFS(BP_BUF_FIELD)
        w.B = (int)bc; w.n = (int)n; w.Lr = Lr;
        w.L = Lr ? (bp::ge*)out->L + p0 * Lr : nullptr;
        w.R = Lr ? (bp::ge*)out->R + p0 * Lr : nullptr;
        w.ptab = gv.tab; w.pbits = gv.bits;
        bp::launch_ipa_load(w, ia + p0 * n, ibv + p0 * n, itr ? itr + p0 : nullptr, st);
        for (int r = 0; r < Lr; r++) bp::launch_ipa_round(w, r, gv.G, gv.H, gv.h, e.dtab, st);
        bp::launch_ipa_final(w, ic + p0, (bp::fe*)out->a + p0, (bp::fe*)out->b + p0, (bp::fe*)out->c + p0,
                             (bp::fe*)out->x + p0, out->c_final ? (bp::fe*)out->c_final + p0 : nullptr, st);
        BP_RET_ON(hipGetLastError());
    }
    if (chunks > 1) {
        BP_RET_ON(hipEventRecord(ib->ipa_ev[1], ib->ipa_side));
        BP_RET_ON(hipStreamWaitEvent(s, ib->ipa_ev[1], 0));
    }
    return HIPBP_OK;
}

// what the three _gens range provers begin with: the checked set's view (a set's n is never 0: a
// null `in` fails the n check)
static int prover_gens(const hipbp_prove_input* in, const void* gens, GenView* gv) {
    if (int rc = gens_check(gens, in ? in->n : 0, "prover: input n differs from the generator set's")) return rc;
    *gv = ((const Gens*)gens)->view();
    return HIPBP_OK;
}

static int ipa_check(const hipbp_ipa_prove_input* in, const hipbp_ipa_proof_out* out) {
    if (!in || !out) { g_err = "ipa prover: null argument"; return HIPBP_ERR_ARG; }
    if (!is_pow2(in->n) || in->n > MAX_N) { g_err = "ipa prover: n must be a power of two <= 65536"; return HIPBP_ERR_ARG; }
    if (in->count > ((size_t)1 << 24)) { g_err = "ipa prover: batch too large"; return HIPBP_ERR_ARG; }
    if (!in->a || !in->b || !in->c) { g_err = "ipa prover: null input"; return HIPBP_ERR_ARG; }
    if (!out->a || !out->b || !out->c || !out->x || (in->n > 1 && (!out->L || !out->R))) {
        g_err = "ipa prover: null output";
        return HIPBP_ERR_ARG;
    }
    return HIPBP_OK;
}

extern "C" {

int hipbp_batch_generate_range_proof(const hipbp_prove_input* in, const ge25519* G, const ge25519* H,
                                     const ge25519* g, const ge25519* h, hipbp_proof_out* out, void* stream) {
    return prove_run(in, GenView(G, H, g, h), out, stream);
}

int hipbp_batch_generate_range_proof_gens(const hipbp_prove_input* in, void* gens, hipbp_proof_out* out,
                                          void* stream) {
    GenView gv;
    if (int rc = prover_gens(in, gens, &gv)) return rc;
    return prove_run(in, gv, out, stream);
}

// The derivation of chosen attempts: proof p's scalars under key_{p, attempt[p]}; a null
// `attempt`: every proof's first key, the seeded prover's derivation.  seed_mu: the stream's keys (an
// accepted call may still need its own), and the try keys go through that prover's key buffer.
int hipbp_derive_prover_scalars_at(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                   const uint8_t* attempt, size_t count, size_t n, fe25519* sL, fe25519* sR,
                                   fe25519* rnd, void* stream) {
    BP_ENGINE_OR_RET(e);
    int rc = seed_check(seed32, v, gamma, count, n);
    if (rc != HIPBP_OK) return rc;
    if (!sL || !sR || !rnd) { g_err = "derive: null output"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    hipStream_t s = pick(stream);
    std::lock_guard<std::mutex> slk(e->seed_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    StreamWs* sb = &e->streams[s];
    BP_RET_ON(sb->seed_keys.need(count * sizeof(bp::fe)));
    bp::fe* keys = sb->seed_keys.as<bp::fe>();
    if (!attempt) {
        bp::launch_seed_derive(bp::seed_words(seed32), (const bp::fe*)v, (const bp::fe*)gamma, index_base, (uint32_t)count,
                               (uint32_t)n, keys, (bp::fe*)sL, (bp::fe*)sR, (bp::fe*)rnd, s);
    } else {
        BP_RET_ON(sb->accept[bp::AB_KEYS].need(count * sizeof(bp::fe)));
        bp::fe* tkeys = sb->accept[bp::AB_KEYS].as<bp::fe>();
        bp::launch_seed_keys(bp::seed_words(seed32), (const bp::fe*)v, (const bp::fe*)gamma, index_base, (uint32_t)count,
                             (uint32_t)n, keys, s);
        bp::launch_try_keys_at(keys, attempt, (uint32_t)count, tkeys, s);
        bp::launch_seed_scalars(tkeys, (uint32_t)count, (uint32_t)n, (bp::fe*)sL, (bp::fe*)sR, (bp::fe*)rnd, s);
    }
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_derive_prover_scalars(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                size_t count, size_t n, fe25519* sL, fe25519* sR, fe25519* rnd, void* stream) {
    return hipbp_derive_prover_scalars_at(seed32, v, gamma, index_base, nullptr, count, n, sL, sR, rnd, stream);
}

int hipbp_batch_generate_range_proof_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                            const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                                            hipbp_proof_out* out, void* stream) {
    return prove_seeded(in, seed32, index_base, GenView(G, H, g, h), out, stream);
}

int hipbp_batch_generate_range_proof_seeded_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                 uint64_t index_base, void* gens, hipbp_proof_out* out, void* stream) {
    GenView gv;
    if (int rc = prover_gens(in, gens, &gv)) return rc;
    return prove_seeded(in, seed32, index_base, gv, out, stream);
}

int hipbp_batch_generate_range_proof_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                              int max_attempts, int check, const ge25519* G, const ge25519* H,
                                              const ge25519* g, const ge25519* h, hipbp_proof_out* out,
                                              uint8_t* attempts, void* stream) {
    return prove_accepted(in, seed32, index_base, max_attempts, check, GenView(G, H, g, h), out, attempts, stream);
}

int hipbp_batch_generate_range_proof_accepted_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                   uint64_t index_base, int max_attempts, int check, void* gens,
                                                   hipbp_proof_out* out, uint8_t* attempts, void* stream) {
    GenView gv;
    if (int rc = prover_gens(in, gens, &gv)) return rc;
    return prove_accepted(in, seed32, index_base, max_attempts, check, gv, out, attempts, stream);
}

int hipbp_accepted_last_stats(int* rounds, uint32_t* proved, float* kernel_ms) {
    if (rounds) *rounds = g_accept_stats.rounds;
    if (proved) memcpy(proved, g_accept_stats.m, sizeof g_accept_stats.m);
    if (kernel_ms) memcpy(kernel_ms, g_accept_stats.ms, sizeof g_accept_stats.ms);
    return HIPBP_OK;
}

int hipbp_batch_pedersen_commit(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, const ge25519* g,
                                const ge25519* h, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    return commit_run(*e, out, nullptr, nullptr, v, gamma, count, GenView(nullptr, nullptr, g, h), pick(stream));
}

int hipbp_batch_pedersen_commit_gens(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, void* gens,
                                     void* stream) {
    BP_ENGINE_OR_RET(e);
    const Gens* gs = (const Gens*)gens;
    if (int rc = gens_check(gs, 0, nullptr)) return rc;
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    return commit_run(*e, out, nullptr, nullptr, v, gamma, count, gs->view(), pick(stream));
}

int hipbp_batch_pedersen_open(uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma, size_t count,
                              const ge25519* g, const ge25519* h, void* gens, void* stream) {
    BP_ENGINE_OR_RET(e);
    const Gens* gs = (const Gens*)gens;
    if (gs)
        if (int rc = gens_check(gs, 0, nullptr)) return rc;
    if (count == 0) return HIPBP_OK;
    if (!ok || !V || !v || !gamma || (!gs && (!g || !h))) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    return commit_run(*e, nullptr, ok, V, v, gamma, count, gs ? gs->view() : GenView(nullptr, nullptr, g, h), pick(stream));
}

int hipbp_batch_inner_product_prove(const hipbp_ipa_prove_input* in, const ge25519* G, const ge25519* H,
                                    const ge25519* Q, hipbp_ipa_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (!G || !H || !Q) { g_err = "ipa prover: null generator"; return HIPBP_ERR_ARG; }
    if (int rc = ipa_check(in, out)) return rc;
    if (in->count == 0) return HIPBP_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    return ipa_enqueue(*e, in, GenView(G, H, nullptr, Q), out, pick(stream));
}

int hipbp_batch_inner_product_prove_gens(const hipbp_ipa_prove_input* in, void* gens, hipbp_ipa_proof_out* out,
                                         void* stream) {
    BP_ENGINE_OR_RET(e);
    Gens* gs = (Gens*)gens;
    if (!gs) { g_err = "null gens"; return HIPBP_ERR_ARG; }
    if (int rc = ipa_check(in, out)) return rc;
    if (int rc = gens_check(gs, in->n, "ipa prover: input n differs from the generator set's")) return rc;
    if (in->count == 0) return HIPBP_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    return ipa_enqueue(*e, in, gs->view(), out, pick(stream));   // (Q: the set's h)
}

}  // extern "C"

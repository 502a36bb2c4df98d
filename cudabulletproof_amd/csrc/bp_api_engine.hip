// bp_api_engine.hip — the engine behind the C ABI of libcudabulletproof_hip.so
// (include/cudabulletproof_hip.h; the other surfaces: bp_engine.h), and the Part-2 entry points on
// device data that neither prove nor encode:
//   hipbp_last_error, hipbp_device_count, hipbp_sync, hipbp_timing_enable / _collect,
//   hipbp_kernel_count / _name, hipbp_release_stream_workspaces
//   hipbp_gens_create / _create_seeded / _copy_points / _destroy
//   hipbp_derive_base_points / _single_point, and their _host forms (CPU only: no HIP call)
//   hipbp_batch_range_proof_verify / _std / _gens, hipbp_batch_inner_product_verify
//   hipbp_pipeline_create / _push / _flush / _prefix_tables / _depth / _destroy / _use_gens / _defer_msm
//   hipbp_msm / _batch / _batch_gens, hipbp_msm_pippenger / _batch / _windows / _horner
//   hipbp_point_tree, hipbp_field_op, hipbp_sm_probe, hipbp_sm_form_probe, hipbp_sha_probe
// They run asynchronously on the caller's stream and return HIPBP_* codes with a message for
// hipbp_last_error.  Unlike the reference, no call allocates and frees device memory of its own: a
// per-device engine keeps grow-only buffers, the identity-doubling and 2^i tables, and one stream.
#include "bp_engine.h"
#include "bp_gens_derive.h"

namespace bpe __attribute__((visibility("hidden"))) {

thread_local std::string g_err;
thread_local AcceptStats g_accept_stats;
Engine* engines[64] = {};
std::mutex engines_mu;
const unsigned long long ROW_MAX_ITEMS = 2048;
const unsigned long long QUAD_MAX_ITEMS = 16384;
const unsigned long long PAIR_MAX_ITEMS = 32768;

hipError_t EventTimer::collect() {
    for (auto& r : pending) {
        hipError_t err = hipEventSynchronize(r.b);
        if (err != hipSuccess) return err;
        float ms = 0;
        if ((err = hipEventElapsedTime(&ms, r.a, r.b)) != hipSuccess) return err;
        total_ms[r.kind] += ms;
        count[r.kind]++;
    }
    pending.clear();
    used = 0;
    return hipSuccess;
}
void EventTimer::reset() {
    pending.clear();
    used = 0;
    for (int i = 0; i < bp::KT_COUNT; i++) { total_ms[i] = 0; count[i] = 0; }
}

hipError_t Engine::init() {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    device = dev;
    if ((e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipMalloc(&dtab, 258 * sizeof(bp::ge))) != hipSuccess) return e;
    // dtab[k] = the identity doubled k times (ge25519_scalarmult's leading zeros), [257] = the
    // host-normalized [256]: computed here with the C forms of the same arithmetic (the device asm
    // forms equal them bit for bit, tests/test_generated_asm.py, asm_check), so a one-proof call
    // launches no set-up kernel and loads no code object besides its own ticks'
    std::vector<bp::ge> t(258);
    t[0] = bp::ge_zero();
    for (int k = 1; k <= 256; k++) t[k] = bp::ge_add(t[k - 1], t[k - 1]);
    t[257] = bp::ge_norm_host(t[256]);
    if ((e = upload(dtab, t.data(), t.size() * sizeof(bp::ge))) != hipSuccess) return e;
    return ensure_two(64);   // grows with the largest n a call brings
}
// Host -> device (bytes a multiple of 16), synchronously: staged in the pinned buffer and read from
// there by a kernel (launch_upload), not by a copy-engine transfer (the process's first
// hipMemcpyAsync of these 33 KB cost ~7 ms on the first call's path).  The stream is drained
// first: a caller's own staged copy out of `pinned` may still be queued on it.
hipError_t Engine::upload(void* dst, const void* src, size_t bytes) {
    if (bytes % 16) return hipErrorInvalidValue;   // (whole uint4s: the tables are 32- / 128-B records)
    hipError_t e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if ((e = need_pinned(bytes)) != hipSuccess) return e;
    memcpy(pinned.p, src, bytes);
    bp::launch_upload(dst, pinned.p, bytes, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}
// two_i[i] = i successive fe_mul(., 2) from 1 (bulletproof_range_proof.cu:705-712): a grow-only
// table, extended on the host (C forms) and uploaded whole on growth.  The old device buffer is
// retired, never freed: ticks and prover launches already queued on OTHER streams (user
// pipelines, caller prover streams) may still read it, and upload() drains only the engine
// stream.  Growth doubles, so the retired buffers total less than the live one (a few KB).
hipError_t Engine::ensure_two(int n) {
    if (n <= two_cap) return hipSuccess;
    hipError_t e;
    const int cap = std::max(n, 2 * two_cap);
    const bp::fe two = bp::fe_add(bp::fe_set(1), bp::fe_set(1));
    while ((int)two_host.size() < cap)
        two_host.push_back(two_host.empty() ? bp::fe_set(1) : bp::fe_mul(two_host.back(), two));
    bp::fe* nt = nullptr;
    if ((e = hipMalloc(&nt, (size_t)cap * sizeof(bp::fe))) != hipSuccess) return e;
    if ((e = upload(nt, two_host.data(), (size_t)cap * sizeof(bp::fe))) != hipSuccess) return e;
    if (two_i) two_retired.push_back(two_i);
    two_i = nt;
    two_cap = cap;
    return hipSuccess;
}

Engine* engine_or_null(hipError_t* err) {
    int dev = 0;
    *err = hipGetDevice(&dev);
    if (*err != hipSuccess) return nullptr;
    if (dev < 0 || dev >= 64) { *err = hipErrorInvalidDevice; return nullptr; }
    std::lock_guard<std::mutex> lk(engines_mu);
    if (!engines[dev]) {
        Engine* e = new Engine();
        *err = e->init();
        if (*err != hipSuccess) {
            delete e;
            return nullptr;
        }
        engines[dev] = e;
    }
    return engines[dev];
}

Engine& engine_or_exit() {
    hipError_t err;
    Engine* e = engine_or_null(&err);
    BP_EXIT_ON(err);
    return *e;
}

int check_batch(const hipbp_proof_batch* b, int range_mode) {
    if (!b) { g_err = "null batch"; return HIPBP_ERR_ARG; }
    if (b->count == 0) return HIPBP_OK;
    if (!is_pow2(b->n) || b->n > MAX_N) { g_err = "n must be a power of two <= 65536"; return HIPBP_ERR_ARG; }
    if (b->ab_len < 1) { g_err = "ab_len must be >= 1"; return HIPBP_ERR_ARG; }
    if ((int)b->L_len > log2i(b->n)) { g_err = "L_len > log2(n)"; return HIPBP_ERR_ARG; }
    if (b->count > (size_t)1 << 24) { g_err = "batch too large"; return HIPBP_ERR_ARG; }
    if (!b->a || !b->b || !b->c || !b->x || (b->L_len && (!b->L || !b->R))) { g_err = "null ipa field"; return HIPBP_ERR_ARG; }
    if (range_mode && (!b->V || !b->A || !b->S || !b->T1 || !b->T2 || !b->t)) { g_err = "null range field"; return HIPBP_ERR_ARG; }
    if (range_mode == 2 && (!b->taux || !b->mu)) { g_err = "range_proof_verify semantics need taux and mu"; return HIPBP_ERR_ARG; }
    return HIPBP_OK;
}

bp::BatchView view_of(const hipbp_proof_batch* b) {
    using bp::fe;
    using bp::ge;
    return bp::BatchView{(int)b->count, (int)b->n, (int)b->ab_len, (int)b->L_len,   // (the struct's own field order)
                         (const ge*)b->V, (const ge*)b->A, (const ge*)b->S, (const ge*)b->T1, (const ge*)b->T2,
                         (const fe*)b->t, (const fe*)b->a, (const fe*)b->b, (const fe*)b->c, (const fe*)b->x,
                         (const ge*)b->L, (const ge*)b->R, (const fe*)b->taux, (const fe*)b->mu, (const ge*)b->Vp};
}

int gens_check(const void* gens, size_t n, const char* what) {
    const Gens* gs = (const Gens*)gens;
    if (!gs) { g_err = "null gens"; return HIPBP_ERR_ARG; }
    if (what && n != gs->n) { g_err = what; return HIPBP_ERR_ARG; }
    int dev = -1;
    BP_RET_ON(hipGetDevice(&dev));
    if (dev != gs->device) { g_err = "gens: created on another device"; return HIPBP_ERR_ARG; }
    return HIPBP_OK;
}

hipError_t Pipeline::init(Engine* eng, hipStream_t st, int nn, int range) {
    e = eng; s = st; n = nn; range_mode = range;
    cfg.n = n; cfg.range_mode = range;
    // the knobs, read once per pipeline (push runs on the issue path)
    const char* ls = getenv("HIPBP_LANE_SORT");
    cfg.lane_sort_mask = ls ? atoi(ls) : 7;
    const char* lt = getenv("HIPBP_LANE_TREE_MAX");
    cfg.lane_tree = n <= (lt ? atoi(lt) : bp::LANE_TREE_MAX);
    const char* qe = getenv("HIPBP_QUAD");
    cfg.quad_force = qe ? (atoi(qe) == 1 ? 4 : atoi(qe) == 2 ? 2 : atoi(qe) == 3 ? 16 : 1) : -1;
    const char* rm = getenv("HIPBP_ROW_MAX_ITEMS");
    const char* qm = getenv("HIPBP_QUAD_MAX_ITEMS");
    const char* pm = getenv("HIPBP_PAIR_MAX_ITEMS");
    cfg.row_max = rm ? strtoull(rm, nullptr, 10) : ROW_MAX_ITEMS;
    cfg.quad_max = qm ? strtoull(qm, nullptr, 10) : QUAD_MAX_ITEMS;
    cfg.pair_max = pm ? strtoull(pm, nullptr, 10) : PAIR_MAX_ITEMS;
    const char* dm = getenv("HIPBP_DEFER_MSM");
    defer_msm = dm && atoi(dm) != 0;
    D = bp::pipeline_depth(cfg);
    slots.resize(D);
    hipError_t r;
    if ((r = hipMalloc(&slots_dev, D * sizeof(bp::SlotDev))) != hipSuccess) return r;
    if ((r = hipHostMalloc(&host_dev, D * sizeof(bp::SlotDev))) != hipSuccess) return r;
    for (auto& sl : slots)
        if ((r = hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming)) != hipSuccess) return r;
    return hipSuccess;
}
void Pipeline::release() {
    if (s) (void)hipStreamSynchronize(s);
    for (auto& sl : slots) {
        for (auto& b : sl.b) (void)b.release();
        if (sl.copied) (void)hipEventDestroy(sl.copied);
    }
    if (slots_dev) (void)hipFree(slots_dev);
    if (host_dev) (void)hipHostFree(host_dev);
    (void)sort_bins.release();
    (void)sort_offs.release();
    (void)ptab.release();
}

hipError_t Pipeline::plan_sort(Slot& sl, int idx) {
    plan = bp::LaneSortPlan{};
    bp::SlotDev& d = sl.dev;
    d.perm0 = nullptr;
    for (auto& q : d.permr) q = nullptr;
    d.perm_ft = nullptr;
    const bp::SortSets ss = bp::lane_sort_sets(cfg, d.bv.B, d.bv.L_len);
    if (!ss.count) return hipSuccess;
    plan.longest_first = (cfg.lane_sort_mask & 8) ? 0 : 1;
    hipError_t r;
    if ((r = sl.b[bp::B_PERM].need(ss.total * sizeof(uint32_t))) != hipSuccess) return r;
    const size_t nb = (size_t)bp::LANE_SORT_SETS * bp::MSM_BINS * sizeof(unsigned);
    if (!sort_bins.p) {
        if ((r = sort_bins.need(nb)) != hipSuccess) return r;
        if ((r = hipMemsetAsync(sort_bins.p, 0, nb, s)) != hipSuccess) return r;
        if ((r = sort_offs.need(nb)) != hipSuccess) return r;
    }
    uint32_t* base = sl.b[bp::B_PERM].as<uint32_t>();
    for (int k = 0; k < ss.count; k++) {
        bp::LaneSortPlan::Set& st = plan.set[k];
        st.kind = ss.set[k].kind; st.r = ss.set[k].r; st.items = ss.set[k].items; st.perm = base;
        st.block0 = ss.set[k].block0;
        if (st.kind == bp::SS_STAGE0 && !d.perm0) d.perm0 = base;
        else if (st.kind == bp::SS_ROUND) d.permr[st.r] = base;
        else d.perm_ft = base;
        base += st.items;
    }
    plan.count = ss.count;
    plan.blocks = ss.blocks;
    plan.slot = slots_dev + idx;
    return hipSuccess;
}

hipError_t Pipeline::carve(Slot& sl, size_t B, size_t Lb) {
    using namespace bp;   // the table's ids and types
    size_t sz[B_COUNT];
    verify_sizes(B, (size_t)n, Lb, range_mode, sz);
    Buf(&b)[B_COUNT] = sl.b;
    hipError_t r = need_all(b, sz);
    if (r != hipSuccess) return r;
    bp::VerifyWs& w = sl.dev.ws;   // (the mode-2 fields stay null in the other modes: never allocated)
    BP_VERIFY_BUFS(BP_BUF_FIELD)
    return hipSuccess;
}

int Pipeline::push(const hipbp_proof_batch* b, const ge25519* P_in, uint8_t* ok, ge25519* P_out, ge25519* chk,
                   uint8_t* flags_out, ge25519* poly_out) {
    EventTimer* tm = e->timer.on ? &e->timer : nullptr;
    bool has = b && b->count > 0;
    Slot& nw = slots[head];
    if (has) {
        int rc = check_batch(b, range_mode);
        if (rc != HIPBP_OK) return rc;
        if ((int)b->n != n) { g_err = "batch n differs from the pipeline's"; return HIPBP_ERR_ARG; }
        if (ring[head].active) { g_err = "pipeline slot busy (internal)"; return HIPBP_ERR_ARG; }
        // admission before anything is staged: a refused push leaves the pipeline as it was
        const int defer = (defer_msm && bp::batch_defers(cfg, (int)b->L_len)) ? 1 : 0;
        const bp::PlanError adm = bp::push_admits(cfg, ring, D, head, b->count, (int)b->L_len, defer);
        if (adm != bp::PLAN_OK && !busy()) {
            g_err = "pipeline tick exceeds 2^32 lanes (batch too large for n)";
            return HIPBP_ERR_ARG;
        }
        if (adm != bp::PLAN_OK) {
            g_err = adm == bp::PLAN_OVERFLOW
                        ? "push refused: with the batches in flight a tick would exceed the region list; run a drain "
                          "tick (push(NULL)) and retry"
                        : "push refused: with the batches in flight a tick would exceed 2^32 lanes; run a drain tick "
                          "(push(NULL)) and retry";
            return HIPBP_ERR_ARG;
        }
        BP_RET_ON(carve(nw, b->count, b->L_len));
        nw.dev.bv = view_of(b);
        nw.dev.ok = ok;
        nw.dev.P_out = (bp::ge*)P_out;
        nw.dev.chk_out = (bp::ge*)chk;
        nw.dev.flags_out = flags_out;
        nw.dev.poly_out = (bp::ge*)poly_out;
        nw.dev.range_mode = range_mode;
        nw.dev.lane_tree = cfg.lane_tree ? 1 : 0;
        nw.dev.ptab = pbits ? tables() : nullptr;
        nw.dev.pbits = pbits;
        nw.dev.defer = defer;
        BP_RET_ON(plan_sort(nw, head));
        BP_RET_ON(hipEventSynchronize(nw.copied));   // staging slot free again
        host_dev[head] = nw.dev;
        BP_RET_ON(hipMemcpyAsync(slots_dev + head, host_dev + head, sizeof(bp::SlotDev), hipMemcpyHostToDevice, s));
        BP_RET_ON(hipEventRecord(nw.copied, s));
        if (!range_mode)
            BP_RET_ON(hipMemcpyAsync(nw.dev.ws.Pin, P_in, b->count * sizeof(ge25519), hipMemcpyDeviceToDevice, s));
        ring[head] = bp::PlanSlot{true, 0, b->count, (int)b->L_len, nw.dev.defer};
    }
    bp::TickPlan tick;
    const bp::PlanError pe = bp::plan_tick(cfg, ring, D, head, tick);
    if (pe == bp::PLAN_OVERFLOW) { g_err = "pipeline region list overflow (internal)"; return HIPBP_ERR_ARG; }
    if (pe == bp::PLAN_TOO_LARGE) { g_err = "pipeline tick exceeds 2^32 lanes (batch too large for n)"; return HIPBP_ERR_ARG; }
    if (tm) tm->mark(bp::KT_TERMS, false, s);
    bp::launch_terms(tick.rl, slots_dev, G, H, g ? g : h, h, e->dtab, e->two_i, s, tick.ql);
    if (tm) tm->mark(bp::KT_TERMS, true, s);
    BP_RET_ON(hipGetLastError());
    if (has && plan.count) {   // the new batch's scalars exist now (its RK_PREP ran): order its lanes
        bp::launch_lane_sort(plan, sort_bins.as<unsigned>(), sort_offs.as<unsigned>(), s);
        BP_RET_ON(hipGetLastError());
    }
    bp::advance_ring(cfg, ring, D, head);
    return HIPBP_OK;
}
int Pipeline::flush() {
    while (busy()) {
        int rc = push(nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != HIPBP_OK) return rc;
    }
    return HIPBP_OK;
}

hipError_t msm_run(Engine& e, bp::ge* results, const bp::fe* scalars, const bp::ge* points, size_t n, size_t count,
                   hipStream_t s, const bp::ge* ptab, int K) {
    Buf(&w)[bp::MB_COUNT] = e.streams[s].msm;
    size_t sz[bp::MB_COUNT];
    bp::msm_sizes(n, count, sz);
    hipError_t err = need_all(w, sz);
    if (err != hipSuccess) return err;
    bp::launch_msm_full(results, scalars, points, n, w[bp::MB_TERMS].as<bp::ge>(), w[bp::MB_ROOT0].as<bp::ge>(),
                        w[bp::MB_ROOT1].as<bp::ge>(), w[bp::MB_ORDER].as<uint32_t>(), w[bp::MB_BINS].as<unsigned>(),
                        e.dtab, s, count, ptab, K);
    return hipGetLastError();
}

// Frees everything the stream owns; every pointer is dropped even if a hipFree fails (none is left
// for a later call to reuse or free twice).  Returns `first`, or the first error met if it had none.
hipError_t StreamWs::release(hipError_t first) {
    auto keep = [&first](hipError_t r) { if (first == hipSuccess) first = r; };
    for (auto& b : msm) keep(b.release());
    for (auto& b : prove) keep(b.release());
    keep(seed_keys.release());
    keep(seed_scal.release());
    for (auto& b : accept) keep(b.release());
    keep(accept_cnt.release());
    for (auto& b : commit) keep(b.release());
    for (auto& b : codec) keep(b.release());
    for (auto& b : ids) keep(b.release());
    if (ipa_side) keep(hipStreamSynchronize(ipa_side));
    for (auto& half : ipa)
        for (auto& b : half) keep(b.release());
    for (hipEvent_t ev : ipa_ev)
        if (ev) keep(hipEventDestroy(ev));
    if (ipa_side) keep(hipStreamDestroy(ipa_side));
    if (pip.side) keep(hipStreamSynchronize(pip.side));
    for (auto* part : {&pip.hi, &pip.lo})
        for (auto& b : *part) keep(b.release());
    for (hipEvent_t ev : pip.ev)
        if (ev) keep(hipEventDestroy(ev));
    if (pip.side) keep(hipStreamDestroy(pip.side));
    for (auto& kv : pipes) {
        kv.second->release();
        delete kv.second;
    }
    pipes.clear();
    return first;
}

int pipeline_for(Engine& e, hipStream_t s, size_t max_batch, int n, int range_mode, Pipeline** out) {
    auto& pipes = e.streams[s].pipes;
    auto key = std::make_pair(n, range_mode);
    auto it = pipes.find(key);
    if (it != pipes.end()) {
        *out = it->second;
        return HIPBP_OK;
    }
    Pipeline* pl = new Pipeline();
    hipError_t ierr = pl->init(&e, s, n, range_mode);
    if (ierr != hipSuccess) {
        pl->release();
        delete pl;
        BP_RET_ON(ierr);
    }
    pipes[key] = pl;
    *out = pl;
    return HIPBP_OK;
}

int run_verify(Engine& e, const hipbp_proof_batch* batch, const ge25519* P_in, const GenView& gv, uint8_t* ok,
               ge25519* P_out, ge25519* chk_out, int range_mode, hipStream_t s, uint8_t* flags_out,
               ge25519* poly_out) {
    int rc = check_batch(batch, range_mode);
    if (rc != HIPBP_OK || batch->count == 0) return rc;
    if (range_mode) BP_RET_ON(e.ensure_two((int)batch->n));
    Pipeline* pl = nullptr;
    if ((rc = pipeline_for(e, s, batch->count, (int)batch->n, range_mode, &pl)) != HIPBP_OK) return rc;
    TableLoan loan(gv, pl);
    rc = pl->push(batch, P_in, ok, P_out, chk_out, flags_out, poly_out);
    if (rc == HIPBP_OK) rc = pl->flush();
    return rc;
}

// What hipbp_gens_create and hipbp_gens_create_seeded share: the checks (sources_ok: the caller's own
// pointers are all there), the set and its snapshot buffer, the prefix tables, the sync and the failure
// path.  fill(d, s) enqueues on s whatever writes the 2n + 2 points at d, in place; its error is
// reported under fill_what.
template <class Fill>
void* gens_build(size_t n, bool sources_ok, int prefix_bits, void* stream, const Fill& fill, const char* fill_what) {
    hipError_t err;
    Engine* e = engine_or_null(&err);
    if (!e) { g_err = std::string("engine: ") + hipGetErrorString(err); return nullptr; }
    if (!is_pow2(n) || n > MAX_N || !sources_ok) { g_err = "gens: bad n or null generator"; return nullptr; }
    if (prefix_bits < 0 || prefix_bits > bp::PREFIX_MAX_BITS) { g_err = "gens: prefix bits must be 0..24"; return nullptr; }
    Gens* gs = new Gens();
    gs->device = e->device;
    gs->n = n;
    hipStream_t s = pick(stream);
    auto fail = [&](hipError_t er, const char* what) -> void* {
        g_err = std::string(what) + ": " + hipGetErrorString(er);
        gs->release();
        delete gs;
        return nullptr;
    };
    if ((err = gs->gen.need(bp::gens_bytes(n))) != hipSuccess) return fail(err, "gens alloc");
    const GenView d = GenView::at(gs->gen.p, n);   // the snapshot, in the packed order
    if ((err = fill(d, s)) != hipSuccess) return fail(err, fill_what);
    if (prefix_bits) {
        if ((err = gs->tab.need(bp::gens_bytes(n) << prefix_bits)) != hipSuccess) return fail(err, "gens tables");
        bp::launch_prefix_tables(gs->tab.as<bp::ge>(), d.G, d.H, d.h, d.g, (int)n, prefix_bits, s);
        if ((err = hipGetLastError()) != hipSuccess) return fail(err, "gens tables");
        gs->bits = prefix_bits;
    }
    if ((err = hipStreamSynchronize(s)) != hipSuccess) return fail(err, "gens sync");
    return gs;
}

// null pointers and the index range of a derive call (bp_gens_derive.h: first + count <= 2^32)
int derive_check(const void* out, const uint8_t* seed32, uint64_t first, size_t count) {
    if (!out || !seed32) { g_err = "derive: null output or seed"; return HIPBP_ERR_ARG; }
    if (first > bp::GENS_INDEX_END || count > bp::GENS_INDEX_END - first) {
        g_err = "derive: first + count must be <= 2^32 (the index is hashed as 32 bits)";
        return HIPBP_ERR_ARG;
    }
    return HIPBP_OK;
}

}  // namespace bpe

using namespace bpe;

extern "C" {

const char* hipbp_last_error(void) { return g_err.c_str(); }

int hipbp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hipbp_sync(void* stream) {
    BP_ENGINE_OR_RET(e);
    BP_RET_ON(hipStreamSynchronize(pick(stream)));
    return HIPBP_OK;
}

static const char* kKernelNames[bp::KT_COUNT] = {"k_prep", "k_terms", "k_tree", "k_combine"};

int hipbp_timing_enable(int on) {
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(e->timer.collect());
    e->timer.reset();
    e->timer.on = on != 0;
    return HIPBP_OK;
}

int hipbp_timing_collect(double* total_ms, uint64_t* launches) {
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(e->timer.collect());
    for (int i = 0; i < bp::KT_COUNT; i++) {
        if (total_ms) total_ms[i] = e->timer.total_ms[i];
        if (launches) launches[i] = e->timer.count[i];
    }
    return HIPBP_OK;
}

int hipbp_kernel_count(void) { return bp::KT_COUNT; }

const char* hipbp_kernel_name(int kind) { return (kind >= 0 && kind < bp::KT_COUNT) ? kKernelNames[kind] : ""; }

// Frees every per-stream workspace the engine keeps for `stream` on the current device (canonical
// MSM / point-tree buffers, prover buffers, commitment terms, IPA prover pair, Pippenger pair, one-shot
// verify pipelines):
// the stream's one record, after waiting for the stream (and, in the record's release, for the two
// pairs' side streams).  A later call on that stream builds them again.
int hipbp_release_stream_workspaces(void* stream) {
    BP_ENGINE_OR_RET(e);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(e->mu);
    // the stream's record is freed and removed even if a hipFree fails; the first error is returned
    hipError_t first = hipStreamSynchronize(s);
    auto it = e->streams.find(s);
    if (it != e->streams.end()) {
        first = it->second.release(first);
        e->streams.erase(it);
    }
    if (first != hipSuccess) {
        g_err = std::string("release_stream_workspaces: ") + hipGetErrorString(first);
        return HIPBP_ERR_DEVICE;
    }
    return HIPBP_OK;
}

void* hipbp_gens_create(size_t n, const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                        int prefix_bits, void* stream) {
    return gens_build(n, G && H && g && h, prefix_bits, stream, [&](const GenView& d, hipStream_t s) {
        const void* const to[4] = {d.G, d.H, d.h, d.g};
        const void* const from[4] = {G, H, h, g};
        for (int k = 0; k < 4; k++)
            if (hipError_t er = hipMemcpyAsync((void*)to[k], from[k], (k < 2 ? n : 1) * bp::GE, hipMemcpyDeviceToDevice, s))
                return er;
        return hipSuccess;
    }, "gens copy");
}

void* hipbp_gens_create_seeded(size_t n, const uint8_t seed_G[32], const uint8_t seed_H[32], const uint8_t seed_g[32],
                               const uint8_t seed_h[32], int prefix_bits, void* stream) {
    return gens_build(n, seed_G && seed_H && seed_g && seed_h, prefix_bits, stream, [&](const GenView& d, hipStream_t s) {
        bp::launch_derive_base_points((bp::ge*)d.G, bp::gens_seed_words(seed_G), 0, n, s);
        bp::launch_derive_base_points((bp::ge*)d.H, bp::gens_seed_words(seed_H), 0, n, s);
        bp::launch_derive_single_point((bp::ge*)d.h, bp::gens_seed_words(seed_h), s);
        bp::launch_derive_single_point((bp::ge*)d.g, bp::gens_seed_words(seed_g), s);
        return hipGetLastError();
    }, "gens derive");
}

int hipbp_gens_copy_points(void* gens, ge25519* G, ge25519* H, ge25519* g, ge25519* h, size_t* n, int* prefix_bits,
                           void* stream) {
    const Gens* gs = (const Gens*)gens;
    if (int rc = gens_check(gs, 0, nullptr)) return rc;
    const GenView d = gs->view();
    void* const to[4] = {G, H, h, g};
    const void* const from[4] = {d.G, d.H, d.h, d.g};
    for (int k = 0; k < 4; k++)
        if (to[k]) BP_RET_ON(hipMemcpyAsync(to[k], from[k], (k < 2 ? gs->n : 1) * bp::GE, hipMemcpyDeviceToDevice, pick(stream)));
    if (n) *n = gs->n;
    if (prefix_bits) *prefix_bits = gs->bits;
    return HIPBP_OK;
}

int hipbp_derive_base_points(ge25519* out, const uint8_t seed32[32], uint64_t first, size_t count, void* stream) {
    if (int rc = derive_check(out, seed32, first, count)) return rc;
    if (count == 0) return HIPBP_OK;
    bp::launch_derive_base_points((bp::ge*)out, bp::gens_seed_words(seed32), first, count, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_derive_single_point(ge25519* out, const uint8_t seed32[32], void* stream) {
    if (int rc = derive_check(out, seed32, 0, 1)) return rc;
    bp::launch_derive_single_point((bp::ge*)out, bp::gens_seed_words(seed32), pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_derive_base_points_host(ge25519* out, const uint8_t seed32[32], uint64_t first, size_t count) {
    if (int rc = derive_check(out, seed32, first, count)) return rc;
    const bp::GenSeed seed = bp::gens_seed_words(seed32);
    for (size_t k = 0; k < count; k++) {
        const bp::ge p = bp::derive_base_point(seed, (uint32_t)(first + k));
        memcpy(out + k, &p, sizeof p);
    }
    return HIPBP_OK;
}

int hipbp_derive_single_point_host(ge25519* out, const uint8_t seed32[32]) {
    if (int rc = derive_check(out, seed32, 0, 1)) return rc;
    const bp::ge p = bp::derive_single_point(bp::gens_seed_words(seed32));
    memcpy(out, &p, sizeof p);
    return HIPBP_OK;
}

void hipbp_gens_destroy(void* gens) {
    Gens* gs = (Gens*)gens;
    if (!gs) return;
    gs->release();
    delete gs;
}

int hipbp_batch_range_proof_verify(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                   const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                   ge25519* check_out, void* stream) {
    (void)g;   // g is not read by cuda_range_proof_verify (crv:82-127)
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!G || !H || !h || !ok) { g_err = "null generator/output"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, nullptr, GenView(G, H, nullptr, h), ok, P_out, check_out, 1, pick(stream));
}

int hipbp_batch_range_proof_verify_std(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                       const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                       ge25519* check_out, uint8_t* flags_out, ge25519* poly_out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!G || !H || !g || !h || !ok) { g_err = "null generator/output"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, nullptr, GenView(G, H, g, h), ok, P_out, check_out, 2, pick(stream), flags_out,
                      poly_out);
}

int hipbp_batch_range_proof_verify_gens(const hipbp_proof_batch* batch, void* gens, uint8_t* ok, ge25519* P_out,
                                        ge25519* check_out, void* stream) {
    Gens* gs = (Gens*)gens;
    if (!gs) { g_err = "null gens"; return HIPBP_ERR_ARG; }
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!ok) { g_err = "null output"; return HIPBP_ERR_ARG; }
    if (int rc = gens_check(gs, batch ? batch->n : 0, batch ? "batch n differs from the generator set's" : nullptr))
        return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, nullptr, gs->view().without_g(), ok, P_out, check_out, 1, pick(stream));
}

int hipbp_batch_inner_product_verify(const hipbp_proof_batch* batch, const ge25519* P, const ge25519* G,
                                     const ge25519* H, const ge25519* Q, uint8_t* ok, ge25519* check_out,
                                     void* stream) {
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!P || !G || !H || !Q || !ok) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, P, GenView(G, H, nullptr, Q), ok, nullptr, check_out, 0, pick(stream));
}

void* hipbp_pipeline_create(size_t max_batch, size_t n, int range_mode, const ge25519* G, const ge25519* H,
                            const ge25519* g, const ge25519* h, void* stream) {
    hipError_t err;
    Engine* e = engine_or_null(&err);
    if (!e) { g_err = std::string("engine: ") + hipGetErrorString(err); return nullptr; }
    if (!is_pow2(n) || n > MAX_N || !G || !H || !h) { g_err = "pipeline: bad n or null generator"; return nullptr; }
    if (range_mode < 0 || range_mode > 2 || (range_mode == 2 && !g)) { g_err = "pipeline: bad mode or null g"; return nullptr; }
    if (range_mode) {
        std::lock_guard<std::mutex> lk(e->mu);
        if ((err = e->ensure_two((int)n)) != hipSuccess) {
            g_err = std::string("pipeline tables: ") + hipGetErrorString(err);
            return nullptr;
        }
    }
    Pipeline* pl = new Pipeline();
    err = pl->init(e, pick(stream), (int)n, range_mode);
    if (err != hipSuccess) {
        g_err = std::string("pipeline init: ") + hipGetErrorString(err);
        pl->release();
        delete pl;
        return nullptr;
    }
    pl->set_gens(GenView(G, H, g, h));
    return pl;
}

int hipbp_pipeline_push(void* handle, const hipbp_proof_batch* batch, const ge25519* P_in, uint8_t* ok,
                        ge25519* P_out, ge25519* check_out, uint8_t* flags_out, ge25519* poly_out) {
    Pipeline* pl = (Pipeline*)handle;
    if (!pl) { g_err = "null pipeline"; return HIPBP_ERR_ARG; }
    if (batch && batch->count && (!ok || (!pl->range_mode && !P_in))) { g_err = "null output/P"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(pl->e->mu);
    return pl->push(batch, P_in, ok, P_out, check_out, flags_out, poly_out);
}

int hipbp_pipeline_flush(void* handle) {
    Pipeline* pl = (Pipeline*)handle;
    if (!pl) { g_err = "null pipeline"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(pl->e->mu);
    return pl->flush();
}

int hipbp_pipeline_prefix_tables(void* handle, int bits) {
    Pipeline* pl = (Pipeline*)handle;
    if (!pl) { g_err = "null pipeline"; return HIPBP_ERR_ARG; }
    if (bits < 0 || bits > bp::PREFIX_MAX_BITS) { g_err = "prefix bits must be 0..24"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(pl->e->mu);
    if (pl->busy()) { g_err = "prefix tables: pipeline has batches in flight (flush first)"; return HIPBP_ERR_ARG; }
    BP_RET_ON(hipStreamSynchronize(pl->s));
    pl->pbits = 0;
    pl->ext_tab = nullptr;
    BP_RET_ON(pl->ptab.release());
    if (!bits) return HIPBP_OK;
    BP_RET_ON(pl->ptab.need(bp::gens_bytes((size_t)pl->n) << bits));
    bp::launch_prefix_tables(pl->ptab.as<bp::ge>(), pl->G, pl->H, pl->h, pl->g, pl->n, bits, pl->s);
    BP_RET_ON(hipGetLastError());
    BP_RET_ON(hipStreamSynchronize(pl->s));
    pl->pbits = bits;
    return HIPBP_OK;
}

int hipbp_pipeline_depth(void* handle) { return handle ? ((Pipeline*)handle)->D : 0; }

void hipbp_pipeline_destroy(void* handle) {
    Pipeline* pl = (Pipeline*)handle;
    if (!pl) return;
    pl->release();
    delete pl;
}

int hipbp_pipeline_use_gens(void* handle, void* gens) {
    Pipeline* pl = (Pipeline*)handle;
    Gens* gs = (Gens*)gens;
    if (!pl || !gs) { g_err = "null pipeline or gens"; return HIPBP_ERR_ARG; }
    if ((int)gs->n != pl->n) { g_err = "pipeline n differs from the generator set's"; return HIPBP_ERR_ARG; }
    if (gs->device != pl->e->device) { g_err = "gens: created on another device"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(pl->e->mu);
    if (pl->busy()) { g_err = "use_gens: pipeline has batches in flight (flush first)"; return HIPBP_ERR_ARG; }
    BP_RET_ON(hipStreamSynchronize(pl->s));
    BP_RET_ON(pl->ptab.release());   // its own tables (hipbp_pipeline_prefix_tables) give way to the set's
    const GenView gv = gs->view();
    pl->set_gens(gv);
    pl->lend_tables(gv.tab, gv.bits);   // for good: nothing takes these back (ptab: released above)
    return HIPBP_OK;
}

int hipbp_pipeline_defer_msm(void* handle, int on) {
    Pipeline* pl = (Pipeline*)handle;
    if (!pl) { g_err = "null pipeline"; return HIPBP_ERR_ARG; }
    if (on && !bp::defer_ok(pl->cfg)) {
        g_err = "defer_msm: needs cuda_range_proof_verify / range_proof_verify semantics, 4 <= n <= the lane-tree limit "
                "and n <= 512 (a split tick's region list)";
        return HIPBP_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(pl->e->mu);
    pl->defer_msm = on != 0;   // applies to the batches pushed from now on
    return HIPBP_OK;
}

int hipbp_msm(ge25519* result, const fe25519* scalars, const ge25519* points, size_t n, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (n == 0) return HIPBP_OK;
    if (!result || !scalars || !points) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(msm_run(*e, (bp::ge*)result, (const bp::fe*)scalars, (const bp::ge*)points, n, 1, pick(stream)));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_msm_batch(ge25519* results, const fe25519* scalars, const ge25519* points, size_t n, size_t count,
                    void* stream) {
    BP_ENGINE_OR_RET(e);
    if (n == 0 || count == 0) return HIPBP_OK;
    if (!results || !scalars || !points) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (count > 0x7FFFFFFFull || n * count > 0xFFFFFFFFull) { g_err = "msm_batch: too many items"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(msm_run(*e, (bp::ge*)results, (const bp::fe*)scalars, (const bp::ge*)points, n, count, pick(stream)));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_msm_batch_gens(ge25519* results, const fe25519* scalars, const void* gens, size_t count, void* stream) {
    BP_ENGINE_OR_RET(e);
    const Gens* gs = (const Gens*)gens;
    if (!gs) { g_err = "null gens"; return HIPBP_ERR_ARG; }
    if (count == 0 || gs->n == 0) return HIPBP_OK;
    if (!results || !scalars) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (int rc = gens_check(gs, 0, nullptr)) return rc;
    const GenView gv = gs->view();   // the MSM's 2n points: G | H, the tables' first 2n bases
    const size_t n = 2 * gv.n;
    if (count > 0x7FFFFFFFull || n * count > 0xFFFFFFFFull) { g_err = "msm_batch_gens: too many items"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(msm_run(*e, (bp::ge*)results, (const bp::fe*)scalars, gv.G, n, count, pick(stream), gv.tab, gv.bits));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_msm_pippenger_batch(ge25519* results, const fe25519* scalars, const ge25519* points, size_t n,
                              size_t count, int window_bits, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (n == 0 || count == 0) return HIPBP_OK;
    if (!results || !scalars || !points) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (window_bits < 4 || window_bits > 12) { g_err = "pippenger: window_bits must be 4..12"; return HIPBP_ERR_ARG; }
    if (count > 0xFFFFu || n * count * ((256 + window_bits - 1) / window_bits) > 0x7FFFFFFFull) {
        g_err = "pippenger: n * count too large";
        return HIPBP_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(bp::msm_pippenger(e->streams[pick(stream)].pip, (bp::ge*)results, (const bp::fe*)scalars,
                                (const bp::ge*)points, n, count, window_bits, e->dtab, pick(stream)));
    return HIPBP_OK;
}

int hipbp_msm_pippenger(ge25519* result, const fe25519* scalars, const ge25519* points, size_t n, int window_bits,
                        void* stream) {
    return hipbp_msm_pippenger_batch(result, scalars, points, n, 1, window_bits, stream);
}

int hipbp_msm_pippenger_windows(ge25519* window_sums, const fe25519* scalars, const ge25519* points, size_t n,
                                int window_bits, int w_begin, int w_end, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (window_bits < 4 || window_bits > 12) { g_err = "pippenger: window_bits must be 4..12"; return HIPBP_ERR_ARG; }
    const int W = (256 + window_bits - 1) / window_bits;
    if (w_begin < 0 || w_end > W || w_begin > w_end) { g_err = "pippenger_windows: need 0 <= w_begin <= w_end <= W"; return HIPBP_ERR_ARG; }
    if (n == 0 || w_begin == w_end) return HIPBP_OK;
    if (!window_sums || !scalars || !points) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (n * (size_t)(w_end - w_begin) > 0x7FFFFFFFull) { g_err = "pippenger: n * windows too large"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(bp::msm_pippenger_windows(e->streams[pick(stream)].pip, (bp::ge*)window_sums, (const bp::fe*)scalars,
                                        (const bp::ge*)points, n, window_bits, w_begin, w_end, e->dtab, pick(stream)));
    return HIPBP_OK;
}

int hipbp_msm_pippenger_horner(ge25519* results, const ge25519* window_sums, size_t count, int window_bits,
                               void* stream) {
    BP_ENGINE_OR_RET(e);
    if (window_bits < 4 || window_bits > 12) { g_err = "pippenger: window_bits must be 4..12"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    if (!results || !window_sums) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (count > 0xFFFFu) { g_err = "pippenger_horner: count <= 65535"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(bp::pippenger_horner((bp::ge*)results, (const bp::ge*)window_sums, count, window_bits,
                                   pick(stream)));
    return HIPBP_OK;
}

int hipbp_point_tree(ge25519* result, const ge25519* points, size_t n, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (n == 0) return HIPBP_OK;
    if (!result || !points) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = pick(stream);
    Buf(&w)[bp::MB_COUNT] = e->streams[s].msm;
    size_t sz[bp::MB_COUNT];
    bp::tree_sizes(n, sz);
    BP_RET_ON(need_all(w, sz));
    bp::launch_tree_full((bp::ge*)result, (const bp::ge*)points, n, w[bp::MB_TREE0].as<bp::ge>(),
                         w[bp::MB_TREE1].as<bp::ge>(), s);
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_field_op(int op, fe25519* r, const fe25519* a, const fe25519* b, size_t count, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (op < 0 || op > 27) { g_err = "bad op"; return HIPBP_ERR_ARG; }
    if (!a || (!b && op != 3 && op != 5 && op != 7 && op != 11 && op != 12 && op != 26)) { g_err = "null operand"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    hipStream_t s = pick(stream);
    if (op == 5)
        bp::launch_invert((bp::fe*)r, (const bp::fe*)a, count, s);
    else
        bp::launch_field_op(op, (bp::fe*)r, (const bp::fe*)a, (const bp::fe*)b, count, s);
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_sm_probe(int force, ge25519* out, const fe25519* scalars, const ge25519* points, size_t count, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (!out || !scalars || !points) { g_err = "null operand"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    bp::launch_sm_probe(force != 0, (bp::ge*)out, (const bp::fe*)scalars, (const bp::ge*)points, count, e->dtab,
                        pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_sm_form_probe(int form, int force, ge25519* out, const fe25519* scalars, const ge25519* points, size_t count,
                        void* stream) {
    BP_ENGINE_OR_RET(e);
    if (form < 1 || form > 3) { g_err = "sm_form_probe: form must be 1 (quads), 2 (pairs) or 3 (rows)"; return HIPBP_ERR_ARG; }
    if (force != 0 && force != 1) { g_err = "sm_form_probe: force must be 0 or 1"; return HIPBP_ERR_ARG; }
    if (force && form != 3) { g_err = "sm_form_probe: force = 1 needs form 3 (only the row form has a recompute)"; return HIPBP_ERR_ARG; }
    if (count > ((size_t)1 << 31)) { g_err = "sm_form_probe: count above 2^31"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    if (!out || !scalars || !points) { g_err = "null operand"; return HIPBP_ERR_ARG; }
    bp::launch_sm_form_probe(form, force != 0, (bp::ge*)out, (const bp::fe*)scalars, (const bp::ge*)points, count, e->dtab,
                             pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_sha_probe(int kind, fe25519* out, const fe25519* in, size_t count, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (kind < 0 || kind > 5) { g_err = "bad sha probe kind"; return HIPBP_ERR_ARG; }
    if (!out || !in) { g_err = "null operand"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    bp::launch_sha_probe(kind, (bp::fe*)out, (const bp::fe*)in, count, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

}  // extern "C"

// bp_capi.hip — the C ABI of libcudabulletproof_hip.so (include/cudabulletproof_hip.h).
//
// Part 1 keeps the reference's cuda_bulletproof.h conventions: host buffers in, result
// out, synchronous, stderr message + early return on a length mismatch, stderr message
// + exit(EXIT_FAILURE) on a device error (CUDA_CHECK, cuda_bulletproof_kernels.cu:13-21).
// Unlike the reference it does not cudaMalloc/cudaFree per call: a per-process engine
// keeps grow-only device buffers, the identity-doubling and 2^i tables, and one stream.
#include <hip/hip_runtime.h>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <thread>

#include "../../include/cudabulletproof_hip.h"
#include "bp_tick_plan.h"
#include "bp_buf.h"
#include "bp_host_prove.h"
#include "ge25519_dev.h"
#include "bp_prove_seed.h"
#include "bp_codec.h"
#include "bp_ids.h"

static_assert(sizeof(fe25519) == 32, "fe25519 layout");
static_assert(sizeof(ge25519) == 128, "ge25519 layout");
static_assert(sizeof(bp::fe) == 32 && sizeof(bp::ge) == 128, "device layout");
static_assert(sizeof(InnerProductProof) == 144, "InnerProductProof layout (SURVEY 8b)");
static_assert(sizeof(RangeProof) == 880, "RangeProof layout (SURVEY 8b)");

namespace {

thread_local std::string g_err;

#define BP_EXIT_ON(call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "HIP error at %s:%d - %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(EXIT_FAILURE);                                                               \
        }                                                                                     \
    } while (0)

#define BP_RET_ON(call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return HIPBP_ERR_DEVICE;                                                          \
        }                                                                                     \
    } while (0)

using bp::Buf;
using bp::PinnedBuf;
using bp::need_all;

// HIP-event timing of the verify pipeline's kernels (bench.py's live roofline numbers).
struct EventTimer {
    struct Rec {
        int kind;
        hipEvent_t a, b;
    };
    bool on = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<Rec> pending;
    hipEvent_t open[bp::KT_COUNT] = {};
    double total_ms[bp::KT_COUNT] = {};
    uint64_t count[bp::KT_COUNT] = {};

    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
    void mark(int kind, bool end, hipStream_t s) {
        hipEvent_t e = get();
        if (!e) return;
        (void)hipEventRecord(e, s);
        if (!end)
            open[kind] = e;
        else
            pending.push_back(Rec{kind, open[kind], e});
    }
    hipError_t collect() {
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
    void reset() {
        pending.clear();
        used = 0;
        for (int i = 0; i < bp::KT_COUNT; i++) { total_ms[i] = 0; count[i] = 0; }
    }
};

struct Pipeline;

// Everything the engine keeps for one caller stream (buffer names and sizes: bp_layout.h), built on
// first use, freed by hipbp_release_stream_workspaces.  The Part-2 calls run asynchronously on the
// caller's stream: calls on two streams never share a buffer, and batches on two streams overlap.
struct StreamWs {
    Buf msm[bp::MB_COUNT];       // canonical MSM / point tree
    Buf prove[bp::PB_COUNT];     // prover (hipbp_batch_generate_range_proof)
    // seeded prover (hipbp_batch_generate_range_proof_seeded): the per-proof keys and the derived
    // scalars of a batch, rnd | sL | sR
    Buf seed_keys, seed_scal;
    // accepted prover (hipbp_batch_generate_range_proof_accepted): the retry loop's buffers and the
    // pinned word its rejected count is read back into; guarded by seed_mu, held for the whole call
    Buf accept[bp::AB_COUNT];
    PinnedBuf accept_cnt;
    // stand-alone IPA prover (hipbp_batch_inner_product_prove): two chunk workspaces, the second run
    // on an internal side stream so one chunk's latency-bound chains run under the other's scalar
    // multiplications (the Pippenger path's scheme)
    Buf ipa[2][bp::IB_COUNT];
    hipStream_t ipa_side = nullptr;
    hipEvent_t ipa_ev[2] = {};   // [0] the caller's stream at entry, [1] the side stream's last chunk done
    bp::PipPair pip;             // Pippenger MSM (hipbp_msm_pippenger*): both parts' buffers and its side stream
    Buf commit[bp::CB_COUNT];    // Pedersen commitments (hipbp_batch_pedersen_commit*): one chunk's terms
    Buf codec[bp::CDB_COUNT];    // proof blob encoder (hipbp_batch_proof_encode): the block counts
    Buf ids[bp::IDB_COUNT];      // proof ids and Merkle roots (hipbp_merkle_root, hipbp_blob_proof_ids): levels, bad counts
    std::map<std::pair<int, int>, Pipeline*> pipes;   // one-shot verify pipelines, per (n, mode)
    hipError_t release(hipError_t first);
};

// Per-device state. The identity-doubling and power-of-two tables are built on first use and cached.
struct Engine {
    EventTimer timer;
    int device = -1;
    hipStream_t stream = nullptr;
    bp::ge* dtab = nullptr;
    bp::fe* two_i = nullptr;
    int two_cap = 0;
    // single-call staging (Part 1: the engine's own stream, synchronous calls): two operand arrays and
    // the result of the reference-surface calls, launch_ip_grid's partial sums, and
    // hipbp_inner_product_prove_host's inputs and outputs
    Buf op_a, op_b, op_out, ip_part, ipa_stage;
    // ... of a single-proof verify: the staged proof, G | H | h | P and the verdict.  single_gens: the
    // G | H | h last uploaded to gens1, as host bytes: a call with the same bytes (the reference's
    // caller passes one generator set call after call) skips their three pageable copies
    Buf proof1, gens1, ok1;
    std::vector<uint8_t> single_gens;
    const void* single_gens_dev = nullptr;
    // ... and its pinned host staging (a pageable source of an async copy must outlive the copy; this
    // one does, and the stream is synced after use): drained of the engine stream's work before it grows
    PinnedBuf pinned;
    hipError_t need_pinned(size_t bytes) {
        hipError_t r;
        if (bytes > pinned.cap && pinned.p && (r = hipStreamSynchronize(stream)) != hipSuccess) return r;
        return pinned.need(bytes);
    }
    // hipbp_batch_range_proof_verify_host: a second stream (chunks alternate over two pipelines)
    // and grow-only staging (pinned host + device), reused across calls
    hipStream_t stream2 = nullptr;
    Buf host_dev;
    PinnedBuf host_pinned;
    // ... and the fixed-base prefix tables of the last generator set it saw (G | H | h, h standing
    // in for g, which cuda_range_proof_verify does not read), kept across calls: a caller verifying
    // batch after batch against one generator set builds them once.  Keyed by the generators' bytes
    // (an exact compare of the host copy).  HIPBP_HOST_PREFIX_BITS: 16 by default (1.1 GB at n = 64,
    // built in ~10 ms; fewer bits for larger n, at most 1.25 GB), 0 turns the tables off.
    std::vector<uint8_t> host_gens_key;
    Buf host_gens, host_tab;
    int host_tab_bits = 0;
    // the host provers (hipbp_batch_generate_range_proof_host_sharded / _accepted_host): their own
    // staging (pinned host: two slots and the generators; device: the seeded prover's two chunk slots
    // or the accepted prover's one chunk, and the generators), grow-only, guarded by prove_host_mu
    // (taken before seed_mu and mu), which a shard holds from its first chunk to its last
    Buf prove_host_dev;
    PinnedBuf prove_host_pinned;
    std::mutex prove_host_mu;
    // the per-stream workspaces (guarded by mu).  seed_mu is held from the seeded prover's derive
    // launches to the end of the prover's enqueue (taken before `mu`), so two host threads on one
    // stream cannot interleave a derivation between another's derivation and its prover; the
    // accepted prover, whose retry rounds read the batch's keys again, holds it for its whole call.
    std::map<hipStream_t, StreamWs> streams;
    std::mutex seed_mu;
    std::mutex mu;

    hipError_t init() {
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
    hipError_t upload(void* dst, const void* src, size_t bytes) {
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
    std::vector<bp::fe> two_host;
    std::vector<bp::fe*> two_retired;
    hipError_t ensure_two(int n) {
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
};

Engine* engines[64] = {};
std::mutex engines_mu;

Engine* engine_or_null(hipError_t* err) {
    int dev = 0;
    *err = hipGetDevice(&dev);
    if (*err != hipSuccess) return nullptr;
    if (dev < 0 || dev >= 64) {
        *err = hipErrorInvalidDevice;
        return nullptr;
    }
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

// How an entry point begins: the current device's engine as `e` (and `err`, for its own HIP calls),
// or HIPBP_ERR_DEVICE with the runtime's message.
#define BP_ENGINE_OR_RET(e)           \
    hipError_t err;                   \
    Engine* e = engine_or_null(&err); \
    BP_RET_ON(err)

// Part-2 entry points run on the caller's stream; NULL is the default (null) stream, as for a
// kernel launch — the stream torch reports as 0 — so work stays ordered with the caller's.
inline hipStream_t pick(void* s) { return (hipStream_t)s; }

bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

constexpr size_t MAX_N = size_t(1) << 16;   // generators per proof (range bits / IPA length)

int log2i(size_t n) {
    int k = 0;
    while ((size_t(1) << k) < n) k++;
    return k;
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
    bp::BatchView v;
    v.B = (int)b->count;
    v.n = (int)b->n;
    v.ab_len = (int)b->ab_len;
    v.L_len = (int)b->L_len;
    v.V = (const bp::ge*)b->V; v.A = (const bp::ge*)b->A; v.S = (const bp::ge*)b->S;
    v.T1 = (const bp::ge*)b->T1; v.T2 = (const bp::ge*)b->T2;
    v.t = (const bp::fe*)b->t; v.a = (const bp::fe*)b->a; v.b = (const bp::fe*)b->b;
    v.c = (const bp::fe*)b->c; v.x = (const bp::fe*)b->x;
    v.L = (const bp::ge*)b->L; v.R = (const bp::ge*)b->R;
    v.taux = (const bp::fe*)b->taux; v.mu = (const bp::fe*)b->mu; v.Vp = (const bp::ge*)b->Vp;
    return v;
}

// A generator set (hipbp_gens_create): a device snapshot of G[n] | H[n] | h | g and, optionally,
// their fixed-base prefix tables (bp::launch_prefix_tables, same base order).
struct Gens {
    int device = -1;
    size_t n = 0;
    Buf gen, tab;
    int bits = 0;
    const bp::ge* G() const { return gen.as<bp::ge>(); }
    const bp::ge* H() const { return gen.as<bp::ge>() + n; }
    const bp::ge* h() const { return gen.as<bp::ge>() + 2 * n; }
    const bp::ge* g() const { return gen.as<bp::ge>() + 2 * n + 1; }
    void release() { (void)gen.release(); (void)tab.release(); }
};

// What every _gens entry point checks of its generator set: that it is there, that it holds the
// call's n (`what` is the entry point's own message; null: the call brings no n) and that it was
// created on the current device.
int gens_check(const void* gens, size_t n, const char* what) {
    const Gens* gs = (const Gens*)gens;
    if (!gs) { g_err = "null gens"; return HIPBP_ERR_ARG; }
    if (what && n != gs->n) { g_err = what; return HIPBP_ERR_ARG; }
    int dev = -1;
    BP_RET_ON(hipGetDevice(&dev));
    if (dev != gs->device) { g_err = "gens: created on another device"; return HIPBP_ERR_ARG; }
    return HIPBP_OK;
}

// Drain-tick thresholds (bp::plan_tick): ticks with at most this many scalar-multiplication items
// run them on lane quads, up to PAIR_MAX_ITEMS on lane pairs.  The cost model (tools/ubench_issue.hip
// with -DLAT: one wave alone issues one instruction per ~9 cycles, the SIMD one per ~4.4): a tick
// lasts about (instructions per wave) x max(9, 4.4 w) cycles for w waves per SIMD, counting the other
// pipeline's concurrent tick (they drain side by side).  Quads cut the instructions per wave of a
// point operation from ~1700 to ~750 for 4x the lanes, pairs to ~1140 for 2x: with both pipelines'
// drains together, a 65,536-item tick is fastest on lanes, 32,768 on pairs, 16,384 on quads
// (configs[4] shard: 173.8 K verifies/s vs 172.1 K with the round-3 bounds 49,152 / 98,304).
// 16-lane rows (sm_row) up to this many items: a one-proof call's ticks (r04b, one MI355X, warm
// cuda_range_proof_verify: n = 16 4.9 -> 4.0 ms, n = 64 6.7 -> 5.5 ms)
constexpr unsigned long long ROW_MAX_ITEMS = 2048;
constexpr unsigned long long QUAD_MAX_ITEMS = 16384;
constexpr unsigned long long PAIR_MAX_ITEMS = 32768;

// The verify pipeline: a ring of D batch slots, one tick per push (the stage table, the tick's
// layout and its form: bp_tick_plan.h).
struct Pipeline {
    Engine* e = nullptr;
    hipStream_t s = nullptr;
    int n = 0, D = 0;
    int range_mode = 1;   // 0 inner product only, 1 cuda_range_proof_verify, 2 range_proof_verify
    const bp::ge *G = nullptr, *H = nullptr, *g = nullptr, *h = nullptr;
    // a slot's device buffers (bp::VerifyBuf): the verify workspace, its mode-2 part, the lane orders
    struct Slot {
        Buf b[bp::B_COUNT];
        bp::SlotDev dev{};
        hipEvent_t copied = nullptr;
    };
    std::vector<Slot> slots;
    bp::PlanSlot ring[bp::MAX_DEPTH];   // the slots' planning state (active, stage, B, L, defer)
    bp::SlotDev* slots_dev = nullptr;   // device copies [D]
    bp::SlotDev* host_dev = nullptr;    // pinned staging [D]
    int head = 0;
    // Layout switches (defaults = the measured best on MI355X): HIPBP_LANE_TREE_MAX (lane trees for
    // n <= it; 138.7K verifies/s vs 137.9K block trees); the tick forms: HIPBP_QUAD forces lanes (0) /
    // quads (1) / pairs (2) / rows (3) on every tick, HIPBP_ROW_MAX_ITEMS / HIPBP_QUAD_MAX_ITEMS /
    // HIPBP_PAIR_MAX_ITEMS move the size bounds; HIPBP_LANE_SORT (bp::lane_sort_sets' mask, 0: off)
    bp::PlanConfig cfg;
    // Split stage 0 ("deferred MSM terms", hipbp_pipeline_defer_msm / HIPBP_DEFER_MSM=1) for the
    // batches pushed from now on, where bp::batch_defers allows it (lane trees, L >= 2)
    bool defer_msm = false;
    Buf sort_bins, sort_offs;
    bp::LaneSortPlan plan{};
    // fixed-base prefix tables of G, H, h, g (hipbp_pipeline_prefix_tables: ptab, owned; or a
    // generator set's, hipbp_pipeline_use_gens: ext_tab, borrowed); pbits = 0: none
    Buf ptab;
    const bp::ge* ext_tab = nullptr;
    int pbits = 0;
    const bp::ge* tables() const { return ext_tab ? ext_tab : ptab.as<bp::ge>(); }
    void set_gens(const void* G_, const void* H_, const void* g_, const void* h_) {
        G = (const bp::ge*)G_; H = (const bp::ge*)H_; g = (const bp::ge*)g_; h = (const bp::ge*)h_;
    }
    hipError_t init(Engine* eng, hipStream_t st, int nn, int range) {
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
    void release() {
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
    // The batch's lane-order buffers and sort plan (its per-lane item sets: bp::lane_sort_sets).
    hipError_t plan_sort(Slot& sl, int idx) {
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
    bool busy() const {
        for (int k = 0; k < D; k++) if (ring[k].active) return true;
        return false;
    }
    hipError_t carve(Slot& sl, size_t B, size_t Lb) {
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
    // One tick; `b` may be null (drain).  Outputs of `b` are written when it completes.
    int push(const hipbp_proof_batch* b, const ge25519* P_in, uint8_t* ok, ge25519* P_out, ge25519* chk,
             uint8_t* flags_out = nullptr, ge25519* poly_out = nullptr) {
        EventTimer* tm = e->timer.on ? &e->timer : nullptr;
        bool has = b && b->count > 0;
        Slot& nw = slots[head];
        if (has) {
            int rc = check_batch(b, range_mode);
            if (rc != HIPBP_OK) return rc;
            if ((int)b->n != n) { g_err = "batch n differs from the pipeline's"; return HIPBP_ERR_ARG; }
            if (ring[head].active) { g_err = "pipeline slot busy (internal)"; return HIPBP_ERR_ARG; }
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
            nw.dev.defer = (defer_msm && bp::batch_defers(cfg, (int)b->L_len)) ? 1 : 0;
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
    int flush() {
        while (busy()) {
            int rc = push(nullptr, nullptr, nullptr, nullptr, nullptr);
            if (rc != HIPBP_OK) return rc;
        }
        return HIPBP_OK;
    }
};

// `count` canonical-tree MSMs of n points each on stream s, in s's own workspace.
hipError_t msm_run(Engine& e, bp::ge* results, const bp::fe* scalars, const bp::ge* points, size_t n, size_t count,
                   hipStream_t s, const bp::ge* ptab = nullptr, int K = 0) {
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

// The engine's cached one-shot pipeline for (stream, n, mode); created on first use.  Cached only
// once fully initialised (a failed init is released, never reused).
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

// One-shot verify of a whole batch on `s` (push + drain of a cached pipeline).
int run_verify(Engine& e, const hipbp_proof_batch* batch, const ge25519* P_in, const ge25519* G, const ge25519* H,
               const ge25519* h, uint8_t* ok, ge25519* P_out, ge25519* chk_out, int range_mode, hipStream_t s,
               const ge25519* g = nullptr, uint8_t* flags_out = nullptr, ge25519* poly_out = nullptr,
               const bp::ge* tab = nullptr, int tab_bits = 0) {
    int rc = check_batch(batch, range_mode);
    if (rc != HIPBP_OK || batch->count == 0) return rc;
    if (range_mode) BP_RET_ON(e.ensure_two((int)batch->n));
    Pipeline* pl = nullptr;
    if ((rc = pipeline_for(e, s, batch->count, (int)batch->n, range_mode, &pl)) != HIPBP_OK) return rc;
    pl->set_gens(G, H, g, h);
    // a generator set's prefix tables, lent for this call only (the cached pipeline is shared with
    // the calls that have none): the ticks' slot records take the pointer at push
    pl->ext_tab = tab_bits ? tab : nullptr;
    pl->pbits = tab_bits ? tab_bits : 0;
    rc = pl->push(batch, P_in, ok, P_out, chk_out, flags_out, poly_out);
    if (rc == HIPBP_OK) rc = pl->flush();
    pl->ext_tab = nullptr;
    pl->pbits = 0;
    return rc;
}

// ---- host staging for the single-proof reference entry points
struct HostProofStage {
    std::vector<fe25519> a, b;
    std::vector<ge25519> L, R;
};

// ---- the host-data entry points' shards on their devices (the contract: bp_host_prove.h, DESIGN
// §15).  open() reads num_gpus and HIPBP_HOST_SHARDS for a call of `count` items and notes the
// caller's device; run() cuts M items into the shards' blocks and calls shard(device, block, stop)
// for each, shard d for device (dev0 + d) % ndev, so num_gpus = 1 stays on the caller's (one rank per
// GPU in a process group).  A shard leaves its message in g_err; the first failure is reported as
// "device d: ..." and the caller's device is restored.
struct HostFan {
    int ndev = 0, dev0 = 0, ng = 0;
    int open(size_t count, int num_gpus) {
        BP_RET_ON(hipGetDeviceCount(&ndev));
        if (int rc = bp::resolve_host_shards(num_gpus, ndev, getenv("HIPBP_HOST_SHARDS"), count, &ng, &g_err)) return rc;
        BP_RET_ON(hipGetDevice(&dev0));
        return HIPBP_OK;
    }
    template <class F>
    int run(size_t M, F shard) {
        const std::vector<bp::HostShard> shards = bp::plan_host_shards(M, ng);
        const bp::HostFanFailure f =
            bp::host_fanout(shards, [&](const bp::HostShard& sh, const bp::HostStop& stop, std::string& err) {
                const int rc = shard((dev0 + sh.d) % ndev, sh, stop);
                if (rc != HIPBP_OK) err = g_err;
                return rc;
            });
        if (f.k != shards.size()) {
            g_err = "device " + std::to_string(shards[f.k].d) + ": " + f.err;
            (void)hipSetDevice(dev0);
            return f.rc;
        }
        BP_RET_ON(hipSetDevice(dev0));
        return HIPBP_OK;
    }
};

}  // namespace

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

int hipbp_batch_range_proof_verify(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                   const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                   ge25519* check_out, void* stream) {
    (void)g;   // g is not read by cuda_range_proof_verify (crv:82-127)
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!G || !H || !h || !ok) { g_err = "null generator/output"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, nullptr, G, H, h, ok, P_out, check_out, 1, pick(stream));
}

int hipbp_batch_range_proof_verify_std(const hipbp_proof_batch* batch, const ge25519* G, const ge25519* H,
                                       const ge25519* g, const ge25519* h, uint8_t* ok, ge25519* P_out,
                                       ge25519* check_out, uint8_t* flags_out, ge25519* poly_out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!G || !H || !g || !h || !ok) { g_err = "null generator/output"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, nullptr, G, H, h, ok, P_out, check_out, 2, pick(stream), g, flags_out,
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
    return run_verify(*e, batch, nullptr, (const ge25519*)gs->G(), (const ge25519*)gs->H(), (const ge25519*)gs->h(),
                      ok, P_out, check_out, 1, pick(stream), nullptr, nullptr, nullptr,
                      gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits);
}

int hipbp_batch_inner_product_verify(const hipbp_proof_batch* batch, const ge25519* P, const ge25519* G,
                                     const ge25519* H, const ge25519* Q, uint8_t* ok, ge25519* check_out,
                                     void* stream) {
    BP_ENGINE_OR_RET(e);
    if (batch && batch->count == 0) return HIPBP_OK;   // nothing read or written: empty outputs may be null
    if (!P || !G || !H || !Q || !ok) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    return run_verify(*e, batch, P, G, H, Q, ok, nullptr, check_out, 0, pick(stream));
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
    pl->set_gens(G, H, g, h);
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
    const size_t bytes = ((size_t)(2 * pl->n + 2) << bits) * sizeof(bp::ge);
    BP_RET_ON(pl->ptab.need(bytes));
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
    const size_t n = 2 * gs->n;
    if (count > 0x7FFFFFFFull || n * count > 0xFFFFFFFFull) { g_err = "msm_batch_gens: too many items"; return HIPBP_ERR_ARG; }
    std::lock_guard<std::mutex> lk(e->mu);
    BP_RET_ON(msm_run(*e, (bp::ge*)results, (const bp::fe*)scalars, gs->G(), n, count, pick(stream),
                      gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits));
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

static int prove_run(const hipbp_prove_input* in, const ge25519* G, const ge25519* H, const ge25519* g,
                     const ge25519* h, const bp::ge* ptab, int pbits, hipbp_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (!in || !out || !G || !H || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
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
    bp::ProveOut po{(bp::ge*)out->V, (bp::ge*)out->A, (bp::ge*)out->S, (bp::ge*)out->T1, (bp::ge*)out->T2,
                    (bp::fe*)out->taux, (bp::fe*)out->mu, (bp::fe*)out->t, (bp::fe*)out->c, (bp::fe*)out->x,
                    (bp::fe*)out->a, (bp::fe*)out->b, (bp::ge*)out->L, (bp::ge*)out->R, out->valid};
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
    w.ptab = ptab; w.pbits = ptab ? pbits : 0;
    auto run = [&](int stage, int r) {
        bp::launch_prove(stage, r, pin, w, po, (const bp::ge*)G, (const bp::ge*)H, (const bp::ge*)g,
                         (const bp::ge*)h, e->dtab, e->two_i, s);
    };
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

int hipbp_batch_generate_range_proof(const hipbp_prove_input* in, const ge25519* G, const ge25519* H,
                                     const ge25519* g, const ge25519* h, hipbp_proof_out* out, void* stream) {
    return prove_run(in, G, H, g, h, nullptr, 0, out, stream);
}

void* hipbp_gens_create(size_t n, const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                        int prefix_bits, void* stream) {
    hipError_t err;
    Engine* e = engine_or_null(&err);
    if (!e) { g_err = std::string("engine: ") + hipGetErrorString(err); return nullptr; }
    if (!is_pow2(n) || n > MAX_N || !G || !H || !g || !h) { g_err = "gens: bad n or null generator"; return nullptr; }
    if (prefix_bits < 0 || prefix_bits > bp::PREFIX_MAX_BITS) { g_err = "gens: prefix bits must be 0..24"; return nullptr; }
    Gens* gs = new Gens();
    gs->device = e->device;
    gs->n = n;
    hipStream_t s = pick(stream);
    const size_t GE = sizeof(ge25519);
    auto fail = [&](hipError_t er, const char* what) -> void* {
        g_err = std::string(what) + ": " + hipGetErrorString(er);
        gs->release();
        delete gs;
        return nullptr;
    };
    if ((err = gs->gen.need((2 * n + 2) * GE)) != hipSuccess) return fail(err, "gens alloc");
    uint8_t* d = gs->gen.as<uint8_t>();   // snapshot: G | H | h | g (the table base order)
    if ((err = hipMemcpyAsync(d, G, n * GE, hipMemcpyDeviceToDevice, s)) != hipSuccess) return fail(err, "gens copy");
    if ((err = hipMemcpyAsync(d + n * GE, H, n * GE, hipMemcpyDeviceToDevice, s)) != hipSuccess) return fail(err, "gens copy");
    if ((err = hipMemcpyAsync(d + 2 * n * GE, h, GE, hipMemcpyDeviceToDevice, s)) != hipSuccess) return fail(err, "gens copy");
    if ((err = hipMemcpyAsync(d + (2 * n + 1) * GE, g, GE, hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return fail(err, "gens copy");
    if (prefix_bits) {
        if ((err = gs->tab.need(((2 * n + 2) << prefix_bits) * GE)) != hipSuccess) return fail(err, "gens tables");
        bp::launch_prefix_tables(gs->tab.as<bp::ge>(), gs->G(), gs->H(), gs->h(), gs->g(), (int)n, prefix_bits, s);
        if ((err = hipGetLastError()) != hipSuccess) return fail(err, "gens tables");
        gs->bits = prefix_bits;
    }
    if ((err = hipStreamSynchronize(s)) != hipSuccess) return fail(err, "gens sync");
    return gs;
}

void hipbp_gens_destroy(void* gens) {
    Gens* gs = (Gens*)gens;
    if (!gs) return;
    gs->release();
    delete gs;
}

int hipbp_batch_generate_range_proof_gens(const hipbp_prove_input* in, void* gens, hipbp_proof_out* out,
                                          void* stream) {
    Gens* gs = (Gens*)gens;   // (a set's n is never 0: a null `in` fails the n check)
    if (int rc = gens_check(gs, in ? in->n : 0, "prover: input n differs from the generator set's")) return rc;
    return prove_run(in, (const ge25519*)gs->G(), (const ge25519*)gs->H(), (const ge25519*)gs->g(),
                     (const ge25519*)gs->h(), gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits, out, stream);
}

// ---- seeded prover (bp_prove_seed.h / .hip): the prover's random scalars derived on the device
// from a 32-byte seed.  seed_check: the shape limits of prove_run, checked before anything is
// enqueued (the derive kernels index with them).
static int seed_check(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, size_t count, size_t n) {
    if (!seed32) { g_err = "seeded prover: null seed"; return HIPBP_ERR_ARG; }
    if (!is_pow2(n) || n > 128) { g_err = "prover: n must be a power of two <= 128"; return HIPBP_ERR_ARG; }
    if (count > ((size_t)1 << 22)) { g_err = "prover: batch too large"; return HIPBP_ERR_ARG; }
    if (!v || !gamma) { g_err = "prover: null input"; return HIPBP_ERR_ARG; }
    return HIPBP_OK;
}

// the key workspace of stream s (e.mu held by the caller), grown to B keys
static int seed_keys(Engine& e, hipStream_t s, size_t B, StreamWs** out) {
    *out = &e.streams[s];
    BP_RET_ON((*out)->seed_keys.need(B * sizeof(bp::fe)));
    return HIPBP_OK;
}

int hipbp_derive_prover_scalars(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                size_t count, size_t n, fe25519* sL, fe25519* sR, fe25519* rnd, void* stream) {
    BP_ENGINE_OR_RET(e);
    int rc = seed_check(seed32, v, gamma, count, n);
    if (rc != HIPBP_OK) return rc;
    if (!sL || !sR || !rnd) { g_err = "derive: null output"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    hipStream_t s = pick(stream);
    std::lock_guard<std::mutex> slk(e->seed_mu);   // (the stream's keys: an accepted call may still need its own)
    std::lock_guard<std::mutex> lk(e->mu);
    StreamWs* sb = nullptr;
    if ((rc = seed_keys(*e, s, count, &sb)) != HIPBP_OK) return rc;
    bp::launch_seed_derive(bp::seed_words(seed32), (const bp::fe*)v, (const bp::fe*)gamma, index_base, (uint32_t)count,
                           (uint32_t)n, sb->seed_keys.as<bp::fe>(), (bp::fe*)sL, (bp::fe*)sR, (bp::fe*)rnd, s);
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

// The derivation of chosen attempts: proof p's scalars under key_{p, attempt[p]}.  The
// try keys go through the accepted prover's key buffer, so this call takes seed_mu as that one does.
int hipbp_derive_prover_scalars_at(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, uint64_t index_base,
                                   const uint8_t* attempt, size_t count, size_t n, fe25519* sL, fe25519* sR,
                                   fe25519* rnd, void* stream) {
    if (!attempt) return hipbp_derive_prover_scalars(seed32, v, gamma, index_base, count, n, sL, sR, rnd, stream);
    BP_ENGINE_OR_RET(e);
    int rc = seed_check(seed32, v, gamma, count, n);
    if (rc != HIPBP_OK) return rc;
    if (!sL || !sR || !rnd) { g_err = "derive: null output"; return HIPBP_ERR_ARG; }
    if (count == 0) return HIPBP_OK;
    hipStream_t s = pick(stream);
    std::lock_guard<std::mutex> slk(e->seed_mu);
    std::lock_guard<std::mutex> lk(e->mu);
    StreamWs* sb = nullptr;
    if ((rc = seed_keys(*e, s, count, &sb)) != HIPBP_OK) return rc;
    BP_RET_ON(sb->accept[bp::AB_KEYS].need(count * sizeof(bp::fe)));
    bp::fe *keys = sb->seed_keys.as<bp::fe>(), *tkeys = sb->accept[bp::AB_KEYS].as<bp::fe>();
    bp::launch_seed_keys(bp::seed_words(seed32), (const bp::fe*)v, (const bp::fe*)gamma, index_base, (uint32_t)count,
                         (uint32_t)n, keys, s);
    bp::launch_try_keys_at(keys, attempt, (uint32_t)count, tkeys, s);
    bp::launch_seed_scalars(tkeys, (uint32_t)count, (uint32_t)n, (bp::fe*)sL, (bp::fe*)sR, (bp::fe*)rnd, s);
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

// what the seeded and the accepted prover check of their arguments before anything is enqueued
static int prove_seeded_check(const hipbp_prove_input* in, const uint8_t* seed32, const ge25519* G, const ge25519* H,
                              const ge25519* g, const ge25519* h, const hipbp_proof_out* out) {
    if (!in || !out || !G || !H || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (in->sL || in->sR || in->rnd) {
        g_err = "seeded prover: sL, sR and rnd must be NULL (the scalars are derived from the seed)";
        return HIPBP_ERR_ARG;
    }
    return seed_check(seed32, in->v, in->gamma, in->count, in->n);
}

// the seeded prover's derive launches and prover enqueue: arguments checked, count > 0, seed_mu held
static int prove_seeded_locked(Engine* e, const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                               const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                               const bp::ge* ptab, int pbits, hipbp_proof_out* out, void* stream) {
    int rc;
    const size_t B = in->count, n = in->n;
    hipStream_t s = pick(stream);
    bp::fe* scal = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        StreamWs* sb = nullptr;
        if ((rc = seed_keys(*e, s, B, &sb)) != HIPBP_OK) return rc;
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
    return prove_run(&full, G, H, g, h, ptab, pbits, out, stream);
}

static int prove_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, const ge25519* G,
                        const ge25519* H, const ge25519* g, const ge25519* h, const bp::ge* ptab, int pbits,
                        hipbp_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    int rc = prove_seeded_check(in, seed32, G, H, g, h, out);
    if (rc != HIPBP_OK) return rc;
    if (in->count == 0) return HIPBP_OK;
    std::lock_guard<std::mutex> slk(e->seed_mu);
    return prove_seeded_locked(e, in, seed32, index_base, G, H, g, h, ptab, pbits, out, stream);
}

int hipbp_batch_generate_range_proof_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                            const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                                            hipbp_proof_out* out, void* stream) {
    return prove_seeded(in, seed32, index_base, G, H, g, h, nullptr, 0, out, stream);
}

int hipbp_batch_generate_range_proof_seeded_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                 uint64_t index_base, void* gens, hipbp_proof_out* out, void* stream) {
    Gens* gs = (Gens*)gens;
    if (int rc = gens_check(gs, in ? in->n : 0, "prover: input n differs from the generator set's")) return rc;
    return prove_seeded(in, seed32, index_base, (const ge25519*)gs->G(), (const ge25519*)gs->H(),
                        (const ge25519*)gs->g(), (const ge25519*)gs->h(), gs->bits ? gs->tab.as<bp::ge>() : nullptr,
                        gs->bits, out, stream);
}

// ---- accepted prover: the seeded prover, the one-shot verify of its proofs, and up to
// max_attempts - 1 retry rounds over the proofs the verifier rejected, each with the scalars of
// the next try key.  What the last call on this thread did, for tools/bench_prove_accepted.py:
// the proofs proved per round and, with HIPBP_ACCEPT_TIMING=1, the loop's own kernels' times.
enum { AK_TRY_KEYS, AK_SELECT, AK_SCATTER, AK_COUNT };
struct AcceptStats {
    int rounds = 0;
    uint32_t m[16] = {};
    float ms[AK_COUNT] = {};
    void add(const AcceptStats& s) {   // another call's, of other proofs: the rounds of the longer one
        rounds = std::max(rounds, s.rounds);
        for (int r = 0; r < 16; r++) m[r] += s.m[r];
        for (int q = 0; q < AK_COUNT; q++) ms[q] += s.ms[q];
    }
};
static thread_local AcceptStats g_accept_stats;

// HIP events round the loop's own launches, read after the call's last synchronise
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
    void end() {
        if (on && !recs.empty()) (void)hipEventRecord(recs.back().b, s);
    }
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

static bp::ProveOut prove_out_of(const hipbp_proof_out& o) {
    return bp::ProveOut{(bp::ge*)o.V, (bp::ge*)o.A, (bp::ge*)o.S, (bp::ge*)o.T1, (bp::ge*)o.T2,
                        (bp::fe*)o.taux, (bp::fe*)o.mu, (bp::fe*)o.t, (bp::fe*)o.c, (bp::fe*)o.x,
                        (bp::fe*)o.a, (bp::fe*)o.b, (bp::ge*)o.L, (bp::ge*)o.R, o.valid};
}

// vtab, vbits: a generator set's prefix tables for the verify (check 1: the one-shot verify takes
// them there, hipbp_batch_range_proof_verify_gens); ptab, pbits: for the prover.
static int prove_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, int max_attempts,
                          int check, const ge25519* G, const ge25519* H, const ge25519* g, const ge25519* h,
                          const bp::ge* ptab, int pbits, hipbp_proof_out* out, uint8_t* attempts, void* stream) {
    using namespace bp;   // the table's ids and types
    BP_ENGINE_OR_RET(e);
    int rc = prove_seeded_check(in, seed32, G, H, g, h, out);
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
    if ((rc = prove_seeded_locked(e, in, seed32, index_base, G, H, g, h, ptab, pbits, out, stream)) != HIPBP_OK) return rc;
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
            hipbp_proof_batch bv{};
            bv.count = m; bv.n = n; bv.ab_len = 1; bv.L_len = Lr;
            bv.V = cur.V; bv.A = cur.A; bv.S = cur.S; bv.T1 = cur.T1; bv.T2 = cur.T2;
            bv.t = cur.t; bv.a = cur.a; bv.b = cur.b; bv.c = cur.c; bv.x = cur.x; bv.L = cur.L; bv.R = cur.R;
            bv.taux = cur.taux; bv.mu = cur.mu;
            const bool tabs = check == 1 && ptab;
            if ((rc = run_verify(*e, &bv, nullptr, G, H, h, w.ok, nullptr, nullptr, check, s, check == 2 ? g : nullptr,
                                 nullptr, nullptr, tabs ? ptab : nullptr, tabs ? pbits : 0)) != HIPBP_OK)
                return rc;
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
        if ((rc = prove_run(&cin, G, H, g, h, ptab, pbits, &cur, stream)) != HIPBP_OK) return rc;
        m = r;
    }
    clk.collect(g_accept_stats.ms);
    return HIPBP_OK;
}

int hipbp_batch_generate_range_proof_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base,
                                              int max_attempts, int check, const ge25519* G, const ge25519* H,
                                              const ge25519* g, const ge25519* h, hipbp_proof_out* out,
                                              uint8_t* attempts, void* stream) {
    return prove_accepted(in, seed32, index_base, max_attempts, check, G, H, g, h, nullptr, 0, out, attempts, stream);
}

int hipbp_batch_generate_range_proof_accepted_gens(const hipbp_prove_input* in, const uint8_t* seed32,
                                                   uint64_t index_base, int max_attempts, int check, void* gens,
                                                   hipbp_proof_out* out, uint8_t* attempts, void* stream) {
    Gens* gs = (Gens*)gens;
    if (int rc = gens_check(gs, in ? in->n : 0, "prover: input n differs from the generator set's")) return rc;
    return prove_accepted(in, seed32, index_base, max_attempts, check, (const ge25519*)gs->G(), (const ge25519*)gs->H(),
                          (const ge25519*)gs->g(), (const ge25519*)gs->h(), gs->bits ? gs->tab.as<bp::ge>() : nullptr,
                          gs->bits, out, attempts, stream);
}

int hipbp_accepted_last_stats(int* rounds, uint32_t* proved, float* kernel_ms) {
    if (rounds) *rounds = g_accept_stats.rounds;
    if (proved) memcpy(proved, g_accept_stats.m, sizeof g_accept_stats.m);
    if (kernel_ms) memcpy(kernel_ms, g_accept_stats.ms, sizeof g_accept_stats.ms);
    return HIPBP_OK;
}

// ---- the provers on host data.  A call is cut into shards (one host thread and one
// device each) and every shard into chunks, by bp_host_prove.h's plan; the shards' results go to
// the caller through its ProofOwner, which also undoes them all if any shard fails.
struct HostProveCall {
    const fe25519 *v, *gamma;
    size_t n;
    const PointVector *G, *H;
    const ge25519 *g, *h;
    const uint8_t* seed32;
    int max_attempts, check;      // the accepted prover's (max_attempts = 0: the seeded prover)
    size_t piece;                 // ... and the proofs per piece of a chunk's way back to the host
    bp::ProofOwner* own;
};

// A shard's hold on its device's prove-host staging: the engine's two streams, the pinned and the
// device buffer grown to hold the generators G | H | g | h at their offsets (the shard's slots lie in
// front of them), the generators uploaded on stream 0 and stream 1 made to wait for them.  It keeps
// prove_host_mu until it goes out of scope: shards and calls on one device run one after another,
// and each leaves both streams drained of its work, so nothing still reads the staging when it grows.
struct HostStage {
    Engine* e = nullptr;
    std::unique_lock<std::mutex> hold;
    hipStream_t st[2] = {nullptr, nullptr};
    bool streams = false;
    uint8_t *host = nullptr, *dbuf = nullptr;
    const ge25519* dG = nullptr;
    hipEvent_t gens_ready = nullptr;

    int open(int dev, const HostProveCall& c, size_t host_gen_off, size_t dev_gen_off) {
        BP_RET_ON(hipSetDevice(dev));
        BP_ENGINE_OR_RET(eng);
        e = eng;
        hold = std::unique_lock<std::mutex>(e->prove_host_mu);
        {
            std::lock_guard<std::mutex> lk(e->mu);
            if (!e->stream2) BP_RET_ON(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
            st[0] = e->stream;
            st[1] = e->stream2;
            streams = true;
        }
        const size_t n = c.n, GE = bp::GE, gb = (2 * n + 2) * GE;
        BP_RET_ON(e->prove_host_pinned.need(host_gen_off + gb));
        BP_RET_ON(e->prove_host_dev.need(dev_gen_off + gb));
        host = e->prove_host_pinned.as<uint8_t>();
        dbuf = e->prove_host_dev.as<uint8_t>();
        uint8_t* hg = host + host_gen_off;
        memcpy(hg, c.G->elements, n * GE);
        memcpy(hg + n * GE, c.H->elements, n * GE);
        memcpy(hg + 2 * n * GE, c.g, GE);
        memcpy(hg + (2 * n + 1) * GE, c.h, GE);
        dG = (const ge25519*)(dbuf + dev_gen_off);
        BP_RET_ON(hipMemcpyAsync(dbuf + dev_gen_off, hg, gb, hipMemcpyHostToDevice, st[0]));
        BP_RET_ON(hipEventCreateWithFlags(&gens_ready, hipEventDisableTiming));
        BP_RET_ON(hipEventRecord(gens_ready, st[0]));
        BP_RET_ON(hipStreamWaitEvent(st[1], gens_ready, 0));
        return HIPBP_OK;
    }
    void drain() {   // nothing in flight reads the staging any more
        if (!streams) return;
        (void)hipStreamSynchronize(st[0]);
        (void)hipStreamSynchronize(st[1]);
    }
    ~HostStage() {
        if (gens_ready) (void)hipEventDestroy(gens_ready);
    }
};

// One shard of the seeded prover.  Its chunks alternate over the engine's two streams and two staging
// slots: a slot's previous chunk is unpacked into the caller's structs (after its stream is drained)
// before the slot's next chunk is staged, so one chunk's copies and unpacking run under the other's
// kernels.  Slot layout (pinned host and device alike):
// v | gamma [c] | V A S T1 T2 [c] | taux mu t c x a b [c] | L R [c Lr] | valid [c].
static int prove_host_seeded_shard(int dev, const HostProveCall& c, const std::vector<bp::HostChunk>& chunks,
                                   const bp::HostStop& stop) {
    const size_t n = c.n, FE = bp::FE, Lr = (size_t)log2i(n), nch = chunks.size();
    const size_t CH = chunks[0].c;   // (the plan's chunks are all of this size but for a shorter last one)
    // a slot: v | gamma [CH], then the proof-output layout (bp::OutLayout)
    const size_t slot_bytes = bp::OutLayout{CH, CH, Lr, 2 * CH * FE}.slot_bytes();
    HostStage sg;
    int rc = sg.open(dev, c, 2 * slot_bytes, 2 * slot_bytes);
    std::string what = g_err;
    hipError_t err;
    for (size_t ch = 0; ch < nch + 2 && rc == HIPBP_OK; ch++) {
        const int k = (int)(ch & 1);
        uint8_t* hs = sg.host + k * slot_bytes;
        uint8_t* ds = sg.dbuf + k * slot_bytes;
        if (ch >= 2) {   // the slot's previous chunk: wait for its D2H, hand it to the caller
            const size_t p0 = chunks[ch - 2].c0, pc = chunks[ch - 2].c;
            if ((err = hipStreamSynchronize(sg.st[k])) != hipSuccess) {
                rc = HIPBP_ERR_DEVICE;
                what = std::string("chunk sync: ") + hipGetErrorString(err);
                break;
            }
            const bp::OutLayout lay{CH, pc, Lr, 2 * CH * FE};
            for (size_t q = 0; q < pc && rc == HIPBP_OK; q++)
                if (!c.own->fill(p0 + q, lay, hs, q, n)) {
                    rc = HIPBP_ERR_DEVICE;
                    what = "Failed to allocate memory for a proof's vectors";
                }
            if (rc != HIPBP_OK) break;
        }
        if (ch >= nch) continue;
        if (stop.raised()) {   // another shard failed: no further chunk
            rc = bp::HOST_SHARD_STOPPED;
            break;
        }
        const size_t c0 = chunks[ch].c0, cc = chunks[ch].c;
        memcpy(hs, c.v + c0, cc * FE);
        memcpy(hs + cc * FE, c.gamma + c0, cc * FE);
        if ((err = hipMemcpyAsync(ds, hs, 2 * cc * FE, hipMemcpyHostToDevice, sg.st[k])) != hipSuccess) {
            rc = HIPBP_ERR_DEVICE;
            what = std::string("chunk H2D: ") + hipGetErrorString(err);
            break;
        }
        const bp::OutLayout lay{CH, cc, Lr, 2 * CH * FE};
        hipbp_prove_input in{cc, n, (const fe25519*)ds, (const fe25519*)ds + cc, nullptr, nullptr, nullptr};
        hipbp_proof_out out;
        lay.view(ds, &out);
        const ge25519* dG = sg.dG;
        rc = prove_seeded(&in, c.seed32, chunks[ch].index_base, dG, dG + n, dG + 2 * n, dG + 2 * n + 1, nullptr, 0, &out,
                          sg.st[k]);
        if (rc != HIPBP_OK) { what = g_err; break; }
        // one D2H of the slot's output regions, points .. valid[c) (the regions are sized for a full
        // chunk; a short last chunk's arrays sit packed at the front of each)
        if ((err = hipMemcpyAsync(hs + lay.o_pts(), ds + lay.o_pts(), lay.used(), hipMemcpyDeviceToHost, sg.st[k])) != hipSuccess) {
            rc = HIPBP_ERR_DEVICE;
            what = std::string("chunk D2H: ") + hipGetErrorString(err);
        }
    }
    if (rc != HIPBP_OK) {
        sg.drain();
        g_err = what;
    }
    return rc;
}

// One shard of the accepted prover.  A chunk is ONE accepted device call (the retry rounds' fixed
// cost is per call), so its chunks are large (HIPBP_PROVE_HOST_ACCEPT_CHUNK) and lie whole
// in the device buffer: v | gamma [c] | the output layout of C | attempts [C].  The pinned staging
// stays the seeded prover's two slots of `piece` proofs: the inputs go up through them, and the
// finished chunk comes back in pieces that alternate over the two slots and streams, a piece being
// unpacked into the caller's structs while the next one copies.  The chunks themselves run one
// after another: a chunk's last piece is unpacked before the next chunk's device call begins.
// `total`: the device calls' statistics, summed over the chunks.
static int prove_host_accepted_shard(int dev, const HostProveCall& c, const std::vector<bp::HostChunk>& chunks,
                                     const bp::HostStop& stop, AcceptStats* total) {
    const size_t n = c.n, FE = bp::FE, GE = bp::GE, Lr = (size_t)log2i(n);
    const size_t C = chunks[0].c, P = std::min(c.piece, C);
    const auto up = [](size_t b) { return (b + 127) & ~(size_t)127; };
    const size_t o_att = bp::OutLayout{P, P, Lr, 2 * P * FE}.slot_bytes();   // a slot: the seeded prover's, then attempts [P]
    const size_t slot_bytes = o_att + up(P);
    const size_t d_att = bp::OutLayout{C, C, Lr, 2 * C * FE}.slot_bytes(), d_gen = d_att + up(C);
    HostStage sg;
    int rc = sg.open(dev, c, 2 * slot_bytes, d_gen);
    std::string what = g_err;
    hipError_t err = hipSuccess;
    auto dev_err = [&](const char* w) {
        rc = HIPBP_ERR_DEVICE;
        what = std::string(w) + ": " + hipGetErrorString(err);
    };
    uint8_t* ds = sg.dbuf;
    uint8_t* datt = sg.dbuf + d_att;
    for (size_t ch = 0; ch < chunks.size() && rc == HIPBP_OK; ch++) {
        if (stop.raised()) {   // another shard failed: no further chunk
            rc = bp::HOST_SHARD_STOPPED;
            break;
        }
        const size_t c0 = chunks[ch].c0, cc = chunks[ch].c;
        // v | gamma up on stream 0, as many proofs at a time as a slot holds
        const size_t pin_in = slot_bytes / (2 * FE);
        for (size_t p0 = 0, j = 0; p0 < cc; p0 += pin_in, j++) {
            const size_t pc = std::min(pin_in, cc - p0);
            uint8_t* hs = sg.host + (j & 1) * slot_bytes;
            if (j >= 2 && (err = hipStreamSynchronize(sg.st[0])) != hipSuccess) { dev_err("chunk input sync"); break; }
            memcpy(hs, c.v + c0 + p0, pc * FE);
            memcpy(hs + pc * FE, c.gamma + c0 + p0, pc * FE);
            if ((err = hipMemcpyAsync(ds + p0 * FE, hs, pc * FE, hipMemcpyHostToDevice, sg.st[0])) != hipSuccess ||
                (err = hipMemcpyAsync(ds + (cc + p0) * FE, hs + pc * FE, pc * FE, hipMemcpyHostToDevice, sg.st[0])) != hipSuccess) {
                dev_err("chunk H2D");
                break;
            }
        }
        if (rc != HIPBP_OK) break;
        const bp::OutLayout lay{C, cc, Lr, 2 * C * FE};
        hipbp_prove_input in{cc, n, (const fe25519*)ds, (const fe25519*)ds + cc, nullptr, nullptr, nullptr};
        hipbp_proof_out out;
        lay.view(ds, &out);
        const ge25519* dG = sg.dG;
        rc = prove_accepted(&in, c.seed32, chunks[ch].index_base, c.max_attempts, c.check, dG, dG + n, dG + 2 * n,
                            dG + 2 * n + 1, nullptr, 0, &out, datt, sg.st[0]);
        if (rc != HIPBP_OK) { what = g_err; break; }
        // (the call returned with stream 0 drained: the chunk is complete, the pinned slots are free)
        total->add(g_accept_stats);
        const size_t np = (cc + P - 1) / P;
        for (size_t j = 0; j < np + 2 && rc == HIPBP_OK; j++) {
            const int k = (int)(j & 1);
            uint8_t* hs = sg.host + k * slot_bytes;
            if (j >= 2) {   // the slot's previous piece: wait for its copies, hand it to the caller
                const size_t p0 = (j - 2) * P, pc = std::min(P, cc - p0);
                if ((err = hipStreamSynchronize(sg.st[k])) != hipSuccess) { dev_err("piece sync"); break; }
                const bp::OutLayout pl{P, pc, Lr, 2 * P * FE};
                for (size_t q = 0; q < pc && rc == HIPBP_OK; q++)
                    if (!c.own->fill(c0 + p0 + q, pl, hs, q, n, hs[o_att + q])) {
                        rc = HIPBP_ERR_DEVICE;
                        what = "Failed to allocate memory for a proof's vectors";
                    }
                if (rc != HIPBP_OK) break;
            }
            if (j >= np) continue;
            // rows [p0, p0 + pc) of each of the chunk's arrays, packed at stride pc into the slot
            const size_t p0 = j * P, pc = std::min(P, cc - p0);
            hipbp_proof_out hv;
            bp::OutLayout{P, pc, Lr, 2 * P * FE}.view(hs, &hv);
            err = hipSuccess;
            auto cp = [&](void* dst, const void* src, size_t bytes) {
                if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sg.st[k]);
            };
            ge25519* const hp[5] = {hv.V, hv.A, hv.S, hv.T1, hv.T2};
            ge25519* const dp[5] = {out.V, out.A, out.S, out.T1, out.T2};
            for (int i = 0; i < 5; i++) cp(hp[i], dp[i] + p0, pc * GE);
            fe25519* const hf[7] = {hv.taux, hv.mu, hv.t, hv.c, hv.x, hv.a, hv.b};
            fe25519* const df[7] = {out.taux, out.mu, out.t, out.c, out.x, out.a, out.b};
            for (int i = 0; i < 7; i++) cp(hf[i], df[i] + p0, pc * FE);
            if (Lr) {
                cp(hv.L, out.L + p0 * Lr, pc * Lr * GE);
                cp(hv.R, out.R + p0 * Lr, pc * Lr * GE);
            }
            cp(hv.valid, out.valid + p0, pc);
            cp(hs + o_att, datt + p0, pc);
            if (err != hipSuccess) dev_err("piece D2H");
        }
    }
    if (rc != HIPBP_OK) {
        sg.drain();
        g_err = what;
    }
    return rc;
}

static size_t env_chunk(const char* name, size_t dflt) {   // a chunk size: at most 2^22, the device calls' limit
    size_t ch = dflt;
    if (const char* ce = getenv(name))
        if (atol(ce) > 0) ch = (size_t)atol(ce);
    return std::min(ch, (size_t)1 << 22);
}
static size_t env_commit_chunk(size_t count) {   // HIPBP_COMMIT_CHUNK for a call of `count` (bp::commit_chunk's rule)
    const char* ce = getenv("HIPBP_COMMIT_CHUNK");
    return bp::commit_chunk(count, ce ? atoll(ce) : 0);
}

// Both host provers: the argument checks (nothing written on an error), the shards' threads, the
// merge.  attempts, max_attempts, check: the accepted prover's (max_attempts = 0: the seeded prover).
static int prove_host_run(RangeProof* proofs, uint8_t* valid, uint8_t* attempts, const fe25519* v, const fe25519* gamma,
                          size_t count, size_t n, const PointVector* G, const PointVector* H, const ge25519* g,
                          const ge25519* h, const uint8_t* seed32, uint64_t index_base, bool accepted, int max_attempts,
                          int check, int num_gpus) {
    if (count == 0) return HIPBP_OK;
    if (!proofs || !valid || !G || !H || !g || !h || !G->elements || !H->elements) {
        g_err = "null argument";
        return HIPBP_ERR_ARG;
    }
    int rc = seed_check(seed32, v, gamma, 0, n);
    if (rc != HIPBP_OK) return rc;
    if (G->length != n || H->length != n) { g_err = "prover: G and H must hold n generators"; return HIPBP_ERR_ARG; }
    if (accepted) {
        if (max_attempts < 1 || max_attempts > 16) { g_err = "accepted prover: max_attempts must be 1..16"; return HIPBP_ERR_ARG; }
        if (check != 1 && check != 2) { g_err = "accepted prover: check must be 1 or 2"; return HIPBP_ERR_ARG; }
        if (!attempts) { g_err = "accepted prover: null attempts"; return HIPBP_ERR_ARG; }
    }
    HostFan fan;
    if ((rc = fan.open(count, num_gpus)) != HIPBP_OK) return rc;
    const size_t chunk = accepted ? env_chunk("HIPBP_PROVE_HOST_ACCEPT_CHUNK", 65536) : env_chunk("HIPBP_PROVE_HOST_CHUNK", 16384);
    if (accepted) g_accept_stats = AcceptStats{};

    bp::ProofOwner own(proofs, valid, attempts, count);   // (zeroes the three outputs)
    const HostProveCall call{v, gamma, n, G, H, g, h, seed32, accepted ? max_attempts : 0, check,
                             env_chunk("HIPBP_PROVE_HOST_CHUNK", 16384), &own};
    std::vector<AcceptStats> stats(fan.ng);   // [shard d]: its device calls', carried back from its thread
    // A call of one shard has the caller's thread for it: the proofs' vectors then come from the
    // caller's malloc arena as they always did; from a thread of its own the one-device seeded call
    // measured 190.7 ms against the parent commit's 180.4 (174.3-184.8), DESIGN §15.
    rc = fan.run(count, [&](int dev, const bp::HostShard& sh, const bp::HostStop& stop) {
        const std::vector<bp::HostChunk> chunks = bp::plan_host_chunks(sh, std::min(chunk, sh.hi - sh.lo), index_base);
        return accepted ? prove_host_accepted_shard(dev, call, chunks, stop, &stats[sh.d])
                        : prove_host_seeded_shard(dev, call, chunks, stop);
    });
    if (rc != HIPBP_OK) {
        own.rollback();   // every vector of every shard freed, proofs, valid and attempts zero
        return rc;
    }
    if (accepted) {
        g_accept_stats = AcceptStats{};   // (a shard run on this thread left its last chunk's here)
        for (const AcceptStats& st : stats) g_accept_stats.add(st);
    }
    return HIPBP_OK;
}

int hipbp_batch_generate_range_proof_host_sharded(RangeProof* proofs, uint8_t* valid, const fe25519* v,
                                                  const fe25519* gamma, size_t count, size_t n, const PointVector* G,
                                                  const PointVector* H, const ge25519* g, const ge25519* h,
                                                  const uint8_t seed32[32], uint64_t index_base, int num_gpus) {
    return prove_host_run(proofs, valid, nullptr, v, gamma, count, n, G, H, g, h, seed32, index_base, false, 0, 0,
                          num_gpus);
}

int hipbp_batch_generate_range_proof_host(RangeProof* proofs, uint8_t* valid, const fe25519* v, const fe25519* gamma,
                                          size_t count, size_t n, const PointVector* G, const PointVector* H,
                                          const ge25519* g, const ge25519* h, const uint8_t seed32[32],
                                          uint64_t index_base) {
    return hipbp_batch_generate_range_proof_host_sharded(proofs, valid, v, gamma, count, n, G, H, g, h, seed32,
                                                         index_base, 1);
}

int hipbp_batch_generate_range_proof_accepted_host(RangeProof* proofs, uint8_t* valid, uint8_t* attempts,
                                                   const fe25519* v, const fe25519* gamma, size_t count, size_t n,
                                                   const PointVector* G, const PointVector* H, const ge25519* g,
                                                   const ge25519* h, const uint8_t seed32[32], uint64_t index_base,
                                                   int max_attempts, int check, int num_gpus) {
    return prove_host_run(proofs, valid, attempts, v, gamma, count, n, G, H, g, h, seed32, index_base, true,
                          max_attempts, check, num_gpus);
}

// ---- Pedersen commitments (bp_commit.hip): pedersen_commit over a batch.  commit_run enqueues a whole
// call on `s`: chunks of HIPBP_COMMIT_CHUNK commitments (read at every call; bp::commit_chunk), one
// after another through the stream's one commit workspace (a chunk's launches are ordered behind the
// previous chunk's on the stream, so the terms are never overwritten while still read).  V null:
// out[i] = the commitment; else ok[i] = (V[i] == the commitment).
static int commit_run(Engine& e, ge25519* out, uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma,
                      size_t count, const bp::ge* g, const bp::ge* h, const bp::ge* ptab, int pbits, size_t gens_n,
                      hipStream_t s) {
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
        const CommitIn in{c, (const fe*)v + c0, (const fe*)gamma + c0, g, h, ptab, ptab ? pbits : 0, (int)gens_n};
        launch_commit(in, w, out ? (ge*)out + c0 : nullptr, V ? (const ge*)V + c0 : nullptr, ok ? ok + c0 : nullptr,
                      e.dtab, s);
    }
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_batch_pedersen_commit(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, const ge25519* g,
                                const ge25519* h, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    return commit_run(*e, out, nullptr, nullptr, v, gamma, count, (const bp::ge*)g, (const bp::ge*)h, nullptr, 0, 0,
                      pick(stream));
}

int hipbp_batch_pedersen_commit_gens(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count, void* gens,
                                     void* stream) {
    BP_ENGINE_OR_RET(e);
    const Gens* gs = (const Gens*)gens;
    if (int rc = gens_check(gs, 0, nullptr)) return rc;
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    return commit_run(*e, out, nullptr, nullptr, v, gamma, count, gs->g(), gs->h(),
                      gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits, gs->n, pick(stream));
}

int hipbp_batch_pedersen_open(uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma, size_t count,
                              const ge25519* g, const ge25519* h, void* gens, void* stream) {
    BP_ENGINE_OR_RET(e);
    const Gens* gs = (const Gens*)gens;
    if (gs)
        if (int rc = gens_check(gs, 0, nullptr)) return rc;
    if (count == 0) return HIPBP_OK;
    if (!ok || !V || !v || !gamma || (!gs && (!g || !h))) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    if (gs)
        return commit_run(*e, nullptr, ok, V, v, gamma, count, gs->g(), gs->h(),
                          gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits, gs->n, pick(stream));
    return commit_run(*e, nullptr, ok, V, v, gamma, count, (const bp::ge*)g, (const bp::ge*)h, nullptr, 0, 0,
                      pick(stream));
}

// One shard of the host form on device `dev`: commitments [lo, hi) of the call, in pieces of one
// commit chunk through the device's prove-host staging (v | gamma | g | h | out of a piece; the
// shard keeps prove_host_mu like the host provers' shards, so shards and calls that share a device
// run one after another) on the engine's own stream, each piece drained before the next is staged.
static int commit_host_shard(int dev, ge25519* out, const fe25519* v, const fe25519* gamma, size_t lo, size_t hi,
                             const ge25519* g, const ge25519* h) {
    BP_RET_ON(hipSetDevice(dev));
    BP_ENGINE_OR_RET(e);
    std::unique_lock<std::mutex> hold(e->prove_host_mu);
    const size_t FE = bp::FE, GE = bp::GE;
    const size_t piece = env_commit_chunk(hi - lo);
    hipStream_t s = e->stream;
    BP_RET_ON(hipStreamSynchronize(s));   // (the staging may grow)
    BP_RET_ON(e->prove_host_dev.need(2 * GE + piece * (2 * FE + GE)));
    uint8_t* d = e->prove_host_dev.as<uint8_t>();
    const bp::ge* dg = (const bp::ge*)d;
    const fe25519* dv = (const fe25519*)(d + 2 * GE);
    ge25519* dout = (ge25519*)(d + 2 * GE + 2 * piece * FE);
    BP_RET_ON(hipMemcpyAsync(d, g, GE, hipMemcpyHostToDevice, s));
    BP_RET_ON(hipMemcpyAsync(d + GE, h, GE, hipMemcpyHostToDevice, s));
    for (size_t c0 = lo; c0 < hi; c0 += piece) {
        const size_t c = std::min(piece, hi - c0);
        BP_RET_ON(hipMemcpyAsync((void*)dv, v + c0, c * FE, hipMemcpyHostToDevice, s));
        BP_RET_ON(hipMemcpyAsync((void*)(dv + piece), gamma + c0, c * FE, hipMemcpyHostToDevice, s));
        if (int rc = commit_run(*e, dout, nullptr, nullptr, dv, dv + piece, c, dg, dg + 1, nullptr, 0, 0, s)) return rc;
        BP_RET_ON(hipMemcpyAsync(out + c0, dout, c * GE, hipMemcpyDeviceToHost, s));
        BP_RET_ON(hipStreamSynchronize(s));
    }
    return HIPBP_OK;
}

int hipbp_batch_pedersen_commit_host(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count,
                                     const ge25519* g, const ge25519* h, int num_gpus) {
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    HostFan fan;
    if (int rc = fan.open(count, num_gpus)) return rc;
    return fan.run(count, [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return commit_host_shard(dev, out, v, gamma, sh.lo, sh.hi, g, h);
    });
}

// ---- stand-alone IPA prover (bp_ipa_prove.hip).  The engine's lock is held by the caller.
// `count` is cut into chunks sized from a workspace budget (HIPBP_IPA_WS_MB per workspace, default
// 512: ~1.8 MB per proof at n = 4096) that alternate over two workspaces: even chunks on the
// caller's stream, odd ones on the internal side stream; the caller's stream waits for the side
// stream at the end.  A chunk's chain latency does not depend on its size, so the fewest chunks
// that fit are used (two whenever count >= 2).
static int ipa_enqueue(Engine& e, const hipbp_ipa_prove_input* in, const bp::ge* G, const bp::ge* H, const bp::ge* Q,
                       const bp::ge* ptab, int pbits, const hipbp_ipa_proof_out* out, hipStream_t s) {
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
        w.ptab = ptab; w.pbits = ptab ? pbits : 0;
        bp::launch_ipa_load(w, ia + p0 * n, ibv + p0 * n, itr ? itr + p0 : nullptr, st);
        for (int r = 0; r < Lr; r++) bp::launch_ipa_round(w, r, G, H, Q, e.dtab, st);
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

int hipbp_batch_inner_product_prove(const hipbp_ipa_prove_input* in, const ge25519* G, const ge25519* H,
                                    const ge25519* Q, hipbp_ipa_proof_out* out, void* stream) {
    BP_ENGINE_OR_RET(e);
    if (!G || !H || !Q) { g_err = "ipa prover: null generator"; return HIPBP_ERR_ARG; }
    if (int rc = ipa_check(in, out)) return rc;
    if (in->count == 0) return HIPBP_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    return ipa_enqueue(*e, in, (const bp::ge*)G, (const bp::ge*)H, (const bp::ge*)Q, nullptr, 0, out,
                       pick(stream));
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
    return ipa_enqueue(*e, in, gs->G(), gs->H(), gs->h(), gs->bits ? gs->tab.as<bp::ge>() : nullptr, gs->bits, out,
                       pick(stream));
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
    if (ipa_enqueue(e, &in, (const bp::ge*)dG, (const bp::ge*)dH, (const bp::ge*)dQ, nullptr, 0, &out, s) != HIPBP_OK) {
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
    pl->set_gens(gs->G(), gs->H(), gs->g(), gs->h());
    pl->ext_tab = gs->bits ? gs->tab.as<bp::ge>() : nullptr;
    pl->pbits = gs->bits;
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

// ===================================================================== reference surface

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

static bool verify_single(const InnerProductProof* ip, const RangeProof* rp, const ge25519* V, const ge25519* P,
                          size_t n, const PointVector* G, const PointVector* H, const ge25519* h) {
    Engine& e = engine_or_exit();
    std::lock_guard<std::mutex> lk(e.mu);
    hipbp_proof_batch b;
    memset(&b, 0, sizeof b);
    if (!stage_single(e, ip, rp, V, &b)) return false;
    b.n = n;
    // generators + h + P
    const size_t cap0 = e.gens1.cap;
    BP_EXIT_ON(e.gens1.need(2 * n * sizeof(ge25519) + 3 * sizeof(ge25519)));
    if (e.gens1.cap != cap0) e.single_gens.clear();   // a new buffer (maybe at the old address) holds nothing
    ge25519* dg = e.gens1.as<ge25519>();
    const size_t GB = n * sizeof(ge25519);
    std::vector<uint8_t>& sg = e.single_gens;
    const bool same = e.single_gens_dev == (const void*)dg && sg.size() == 2 * GB + sizeof(ge25519) &&
                      memcmp(sg.data(), G->elements, GB) == 0 && memcmp(sg.data() + GB, H->elements, GB) == 0 &&
                      memcmp(sg.data() + 2 * GB, h, sizeof(ge25519)) == 0;
    if (!same) {   // (every earlier user of dg has finished: each call ends with a stream sync)
        BP_EXIT_ON(hipMemcpyAsync(dg, G->elements, GB, hipMemcpyHostToDevice, e.stream));
        BP_EXIT_ON(hipMemcpyAsync(dg + n, H->elements, GB, hipMemcpyHostToDevice, e.stream));
        BP_EXIT_ON(hipMemcpyAsync(dg + 2 * n, h, sizeof(ge25519), hipMemcpyHostToDevice, e.stream));
        sg.resize(2 * GB + sizeof(ge25519));
        memcpy(sg.data(), G->elements, GB);
        memcpy(sg.data() + GB, H->elements, GB);
        memcpy(sg.data() + 2 * GB, h, sizeof(ge25519));
        e.single_gens_dev = dg;
    }
    if (P) BP_EXIT_ON(hipMemcpyAsync(dg + 2 * n + 1, P, sizeof(ge25519), hipMemcpyHostToDevice, e.stream));
    BP_EXIT_ON(e.ok1.need(64));
    int rc = run_verify(e, &b, P ? dg + 2 * n + 1 : nullptr, dg, dg + n, dg + 2 * n, e.ok1.as<uint8_t>(), nullptr,
                        nullptr, rp != nullptr ? 1 : 0, e.stream);
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

// ---- batch form of cuda_range_proof_verify over the reference's host RangeProof structs
}  // extern "C"

namespace {

// What a shard of the host verifiers takes its 1024-proof chunks from.  host_bytes / dev_bytes: the
// chunk's pinned and device staging; stage: fills the pinned bytes at hc, enqueues on s what leaves the
// flat chunk at dc, and views it as *b (`word`: a zeroed device word of the shard's, summed into by a
// source that counts something); out_index: where proof k of the shard's verdicts goes.
//
// The caller's host structs (hipbp_batch_range_proof_verify_host): packed on the host, copied as they are.
struct StructChunks {
    const RangeProof* proofs;
    const ge25519* V;
    const size_t* idx;
    size_t abl, Lr, n;
    size_t host_bytes(size_t, size_t c) const { return bp::ChunkLayout{c, abl, Lr}.bytes(); }
    size_t dev_bytes(size_t c0, size_t c) const { return host_bytes(c0, c); }
    size_t out_index(size_t k) const { return idx[k]; }
    int stage(size_t c0, size_t c, uint8_t* hc, uint8_t* dc, uint32_t*, hipStream_t s, hipbp_proof_batch* b) const {
        const bp::ChunkLayout lay{c, abl, Lr};
        for (size_t k = 0; k < c; k++) {
            const RangeProof& p = proofs[idx[c0 + k]];
            lay.pack(hc, k, p.ip_proof, &p, &V[idx[c0 + k]]);
        }
        hipError_t err = hipMemcpyAsync(dc, hc, lay.bytes(), hipMemcpyHostToDevice, s);
        if (err != hipSuccess) {
            g_err = std::string("chunk H2D: ") + hipGetErrorString(err);
            return HIPBP_ERR_DEVICE;
        }
        memset(b, 0, sizeof *b);
        b->n = n;
        lay.view(dc, b);
        return HIPBP_OK;
    }
};

inline size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }

// A host blob's proofs [lo, lo + B) (hipbp_batch_range_proof_verify_bytes_host; the blob parsed by the
// caller): a chunk uploads its kind bytes, its compact slots, its raw_index entries and raw records
// (raw_index is ascending: two binary searches bound them) and the caller's V rows, each part at a
// 16-byte boundary, and decodes them on the chunk's stream into a flat chunk behind the copy, with
// taux | mu after it when the blob has them.
struct BlobChunks {
    const uint8_t* blob;
    bp::CodecLayout l;   // the whole blob's
    size_t R, n, lo;
    const ge25519* V;    // the caller's, or null: each proof's own
    struct Parts { size_t j0, nr, o_cmp, o_idx, o_raw, o_v, slice, o_flat, o_tm, end; };
    Parts parts(size_t c0, size_t c) const {
        Parts p;
        const uint8_t* ri = blob + l.o_rawidx();
        p.j0 = bp::codec_raw_lower(ri, R, lo + c0);
        p.nr = bp::codec_raw_lower(ri, R, lo + c0 + c) - p.j0;
        p.o_cmp = pad16(c);
        p.o_idx = p.o_cmp + c * l.Sc();
        p.o_raw = p.o_idx + pad16(4 * p.nr);
        p.o_v = p.o_raw + pad16(p.nr * l.Sr());
        p.slice = p.o_v + (V ? c * bp::GE : 0);
        p.o_flat = (p.slice + 127) & ~(size_t)127;
        p.o_tm = p.o_flat + bp::ChunkLayout{c, l.abl, l.Lr}.bytes();
        p.end = p.o_tm + (l.f ? 2 * c * bp::FE : 0);
        return p;
    }
    size_t host_bytes(size_t c0, size_t c) const { return (parts(c0, c).slice + 127) & ~(size_t)127; }
    size_t dev_bytes(size_t c0, size_t c) const { return (parts(c0, c).end + 127) & ~(size_t)127; }
    size_t out_index(size_t k) const { return lo + k; }
    int stage(size_t c0, size_t c, uint8_t* hc, uint8_t* dc, uint32_t* word, hipStream_t s, hipbp_proof_batch* b) const {
        const Parts p = parts(c0, c);
        const size_t P0 = lo + c0;
        memcpy(hc, blob + l.o_kind() + P0, c);
        memcpy(hc + p.o_cmp, blob + l.o_compact() + P0 * l.Sc(), c * l.Sc());
        memcpy(hc + p.o_idx, blob + l.o_rawidx() + 4 * p.j0, 4 * p.nr);
        memcpy(hc + p.o_raw, blob + l.o_raw(R) + p.j0 * l.Sr(), p.nr * l.Sr());
        if (V) memcpy(hc + p.o_v, V + P0, c * bp::GE);
        hipError_t err = hipMemcpyAsync(dc, hc, p.slice, hipMemcpyHostToDevice, s);
        if (err != hipSuccess) {
            g_err = std::string("chunk H2D: ") + hipGetErrorString(err);
            return HIPBP_ERR_DEVICE;
        }
        memset(b, 0, sizeof *b);
        b->n = n;
        bp::ChunkLayout{c, l.abl, l.Lr}.view(dc + p.o_flat, b);
        bp::CodecArrays A;
        const ge25519* pts[5] = {b->V, b->A, b->S, b->T1, b->T2};
        for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
        A.t = (bp::fe*)b->t; A.c = (bp::fe*)b->c; A.x = (bp::fe*)b->x; A.a = (bp::fe*)b->a; A.b = (bp::fe*)b->b;
        A.L = (bp::ge*)b->L; A.R = (bp::ge*)b->R;
        A.taux = l.f ? (bp::fe*)(dc + p.o_tm) : nullptr;
        A.mu = l.f ? A.taux + c : nullptr;
        b->taux = (const fe25519*)A.taux; b->mu = (const fe25519*)A.mu;
        if (V) {   // the verify's V argument is the caller's; the proof's own V stays where it was decoded
            b->Vp = b->V;
            b->V = (const ge25519*)(dc + p.o_v);
        }
        bp::BlobView v;
        v.kind = dc; v.compact = dc + p.o_cmp; v.rawidx = dc + p.o_idx; v.raw = dc + p.o_raw;
        v.count = c; v.R = p.nr; v.base = P0;
        v.kind_n = v.compact_n = c; v.rawidx_n = v.raw_n = p.nr;
        bp::launch_codec_decode(v, A, l, word, s);
        if ((err = hipGetLastError()) != hipSuccess) {
            g_err = std::string("chunk decode: ") + hipGetErrorString(err);
            return HIPBP_ERR_DEVICE;
        }
        return HIPBP_OK;
    }
};

// one device's shard of a host verifier (its own host thread): B proofs from `src`.  The shard is cut
// into chunks of CHUNK proofs, each staged as its own little flat batch; each chunk is staged,
// copied and pushed as soon as it is staged (the GPU starts while the host stages the rest), and
// the chunks alternate over two pipelines on two streams, whose ticks fill each other's tails.
// mode 1: cuda_range_proof_verify semantics, with the cached host prefix tables; mode 2:
// range_proof_verify semantics (g read), without tables.
template <class Src>
int host_shard(int dev, const Src& src, size_t B, size_t n, const PointVector* G, const PointVector* H,
               const ge25519* g, const ge25519* h, int mode, uint8_t* ok) {
    BP_RET_ON(hipSetDevice(dev));
    BP_ENGINE_OR_RET(e);
    constexpr size_t CHUNK = 1024;
    const size_t GE = bp::GE;
    const size_t nch = (B + CHUNK - 1) / CHUNK;
    size_t hsum = 0, dsum = 0;
    for (size_t ch = 0; ch < nch; ch++) {
        const size_t c0 = ch * CHUNK, c = std::min(CHUNK, B - c0);
        hsum += src.host_bytes(c0, c);
        dsum += src.dev_bytes(c0, c);
    }
    // after the chunks: G | H | h | g, the verdicts, and the source's counter word
    const size_t tail = (2 * n + 2) * GE + pad16(B) + 16;
    const size_t gen_off_h = hsum, gen_off = dsum, ok_off_h = gen_off_h + (2 * n + 2) * GE, ok_off = gen_off + (2 * n + 2) * GE;
    const size_t bytes_h = hsum + tail, bytes = dsum + tail;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->stream2) BP_RET_ON(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
    hipStream_t st[2] = {e->stream, e->stream2};
    // need() frees a buffer that grows: nothing may still read either
    if ((bytes_h > e->host_pinned.cap && e->host_pinned.p) || bytes > e->host_dev.cap) {
        BP_RET_ON(hipStreamSynchronize(st[0]));
        BP_RET_ON(hipStreamSynchronize(st[1]));
    }
    BP_RET_ON(e->host_pinned.need(bytes_h));
    BP_RET_ON(e->host_dev.need(bytes));
    uint8_t* host = e->host_pinned.as<uint8_t>();
    uint8_t* dbuf = e->host_dev.as<uint8_t>();
    memcpy(host + gen_off_h, G->elements, n * GE);
    memcpy(host + gen_off_h + n * GE, H->elements, n * GE);
    memcpy(host + gen_off_h + 2 * n * GE, h, GE);
    if (mode == 2) memcpy(host + gen_off_h + (2 * n + 1) * GE, g, GE);
    BP_RET_ON(hipMemcpyAsync(dbuf + gen_off, host + gen_off_h, (2 * n + (mode == 2 ? 2 : 1)) * GE, hipMemcpyHostToDevice,
                             st[0]));
    uint32_t* word = (uint32_t*)(dbuf + ok_off + pad16(B));
    BP_RET_ON(hipMemsetAsync(word, 0, 16, st[0]));
    BP_RET_ON(e->ensure_two((int)n));   // engine stream: ordered before the pipeline's first tick
    const ge25519* dgen = (const ge25519*)(dbuf + gen_off);
    // the generators' prefix tables: reused when this call's generator bytes equal the cached set's
    // (then the pipelines read this call's copy and the tables built from identical bytes)
    int hb = 16;
    if (const char* pb = getenv("HIPBP_HOST_PREFIX_BITS")) hb = std::max(0, std::min(atoi(pb), bp::PREFIX_MAX_BITS));
    if (mode == 2) hb = 0;
    while (hb > 0 && ((2 * n + 2) << hb) * GE > (size_t(5) << 28)) hb--;   // at most 1.25 GB of tables (K = 12 at n = 1024)
    if (hb > 0) {
        const uint8_t* key = host + gen_off_h;
        const size_t kb = (2 * n + 1) * GE;
        if (e->host_tab_bits != hb || e->host_gens_key.size() != kb || memcmp(e->host_gens_key.data(), key, kb) != 0) {
            e->host_tab_bits = 0;
            e->host_gens_key.clear();
            BP_RET_ON(hipStreamSynchronize(st[0]));   // a previous call's tables are no longer read
            BP_RET_ON(hipStreamSynchronize(st[1]));
            if (e->host_gens.need((2 * n + 2) * GE) != hipSuccess || e->host_tab.need(((2 * n + 2) << hb) * GE) != hipSuccess) {
                (void)hipGetLastError();   // no room for the tables: verify without them
                hb = 0;
            }
        }
        if (hb > 0 && e->host_tab_bits == 0) {
            uint8_t* dg = e->host_gens.as<uint8_t>();
            BP_RET_ON(hipMemcpyAsync(dg, dbuf + gen_off, kb, hipMemcpyDeviceToDevice, st[0]));
            BP_RET_ON(hipMemcpyAsync(dg + kb, dbuf + gen_off + 2 * n * GE, GE, hipMemcpyDeviceToDevice, st[0]));
            const bp::ge* gg = e->host_gens.as<bp::ge>();
            bp::launch_prefix_tables(e->host_tab.as<bp::ge>(), gg, gg + n, gg + 2 * n, gg + 2 * n + 1, (int)n, hb,
                                     st[0]);
            BP_RET_ON(hipGetLastError());
            e->host_gens_key.assign(key, key + kb);
            e->host_tab_bits = hb;
        }
    }
    Pipeline* pl[2] = {nullptr, nullptr};
    int rc = HIPBP_OK;
    for (int k = 0; k < 2 && rc == HIPBP_OK; k++) {
        rc = pipeline_for(*e, st[k], std::min(B, CHUNK), (int)n, mode, &pl[k]);
        if (rc == HIPBP_OK) {
            pl[k]->set_gens(dgen, dgen + n, mode == 2 ? dgen + 2 * n + 1 : nullptr, dgen + 2 * n);
            // (the engine's one-shot pipelines are shared with the other entry points: the tables
            // are lent for this call only and taken back after the flush below)
            pl[k]->ext_tab = hb > 0 ? e->host_tab.as<bp::ge>() : nullptr;
            pl[k]->pbits = hb > 0 ? hb : 0;
        }
    }
    hipEvent_t gens_ready = nullptr;
    if (rc == HIPBP_OK) {   // the second stream waits for the generators' copy (and the zeroed word)
        BP_RET_ON(hipEventCreateWithFlags(&gens_ready, hipEventDisableTiming));
        BP_RET_ON(hipEventRecord(gens_ready, st[0]));
        BP_RET_ON(hipStreamWaitEvent(st[1], gens_ready, 0));
    }
    uint8_t* dok = dbuf + ok_off;
    size_t off_h = 0, off = 0;
    for (size_t ch = 0; ch < nch && rc == HIPBP_OK; ch++) {
        const size_t c0 = ch * CHUNK, c = std::min(CHUNK, B - c0);
        hipbp_proof_batch b;
        if ((rc = src.stage(c0, c, host + off_h, dbuf + off, word, st[ch & 1], &b)) != HIPBP_OK) break;
        rc = pl[ch & 1]->push(&b, nullptr, dok + c0, nullptr, nullptr);
        off_h += src.host_bytes(c0, c);
        off += src.dev_bytes(c0, c);
    }
    for (int k = 0; k < 2 && rc == HIPBP_OK; k++) rc = pl[k]->flush();
    for (int k = 0; k < 2; k++)
        if (pl[k]) {
            pl[k]->ext_tab = nullptr;
            pl[k]->pbits = 0;
        }
    hipError_t s1 = hipStreamSynchronize(st[1]);
    if (rc == HIPBP_OK && s1 == hipSuccess) {
        if ((err = hipMemcpyAsync(host + ok_off_h, dok, pad16(B) + 16, hipMemcpyDeviceToHost, st[0])) == hipSuccess)
            err = hipStreamSynchronize(st[0]);
        if (err != hipSuccess) { g_err = std::string("shard D2H: ") + hipGetErrorString(err); rc = HIPBP_ERR_DEVICE; }
        else if (*(const uint32_t*)(host + ok_off_h + pad16(B)) != 0) {   // (the blob was parsed: not reached)
            g_err = "blob decode skipped records of a parsed blob (internal)";
            rc = HIPBP_ERR_DEVICE;
        }
    } else {
        (void)hipStreamSynchronize(st[0]);   // nothing in flight reads the staging any more
        if (rc == HIPBP_OK) { g_err = std::string("stream2: ") + hipGetErrorString(s1); rc = HIPBP_ERR_DEVICE; }
    }
    if (gens_ready) (void)hipEventDestroy(gens_ready);
    if (rc == HIPBP_OK)
        for (size_t k = 0; k < B; k++) ok[src.out_index(k)] = host[ok_off_h + k] ? 1 : 0;
    return rc;
}

// the shape checks of the device batch (n a power of two, L_len <= log2 n) for a host batch
int host_verify_shape(size_t n, size_t abl, size_t Lr) {
    hipbp_proof_batch probe;
    memset(&probe, 0, sizeof probe);
    probe.count = 1; probe.n = n; probe.ab_len = abl; probe.L_len = Lr;
    const uint8_t dummy[1] = {0};
    probe.V = probe.A = probe.S = probe.T1 = probe.T2 = (const ge25519*)dummy;
    probe.t = probe.a = probe.b = probe.c = probe.x = (const fe25519*)dummy;
    probe.L = probe.R = (const ge25519*)dummy;
    return check_batch(&probe, 1);
}

}  // namespace

extern "C" {

int hipbp_batch_range_proof_verify_host(const RangeProof* proofs, const ge25519* V, size_t count, size_t n,
                                        const PointVector* G, const PointVector* H, const ge25519* g,
                                        const ge25519* h, int num_gpus, uint8_t* ok) {
    (void)g;   // g is not read by cuda_range_proof_verify (crv:82-127)
    if (count == 0) return HIPBP_OK;
    if (!proofs || !V || !G || !H || !h || !ok || !G->elements || !H->elements) {
        g_err = "null argument";
        return HIPBP_ERR_ARG;
    }
    HostFan fan;
    int rc = fan.open(count, num_gpus);
    if (rc != HIPBP_OK) return rc;
    // The flat batch needs one (a/b length, rounds) shape: the first proof that passes the checks
    // sets it (the reference prover's proofs all share it); proofs of another shape go one by one.
    size_t abl = 0, Lr = 0;
    std::vector<size_t> main, other;
    main.reserve(count);
    for (size_t i = 0; i < count; i++) {
        const InnerProductProof& ip = proofs[i].ip_proof;
        ok[i] = 0;
        if (G->length != ip.n || H->length != ip.n || n != ip.n) {   // crv:140-143, as the single call
            fprintf(stderr, "Error: Vector lengths must match for inner product verification\n");
            continue;
        }
        if (ip.b.length != ip.a.length || ip.a.length == 0 || ip.L.length < ip.L_len || ip.R.length < ip.L_len ||
            !ip.a.elements || !ip.b.elements || (ip.L_len && (!ip.L.elements || !ip.R.elements)))
            continue;   // stage_single's check: the single call returns false as well
        if (main.empty()) { abl = ip.a.length; Lr = ip.L_len; }
        (ip.a.length == abl && ip.L_len == Lr ? main : other).push_back(i);
    }
    if (!main.empty() && (rc = host_verify_shape(n, abl, Lr)) != HIPBP_OK) return rc;
    // (the shards: as many as `count` asks for, cut from the index list)
    rc = fan.run(main.size(), [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return host_shard(dev, StructChunks{proofs, V, main.data() + sh.lo, abl, Lr, n}, sh.hi - sh.lo, n, G, H, nullptr, h, 1, ok);
    });
    if (rc != HIPBP_OK) return rc;
    for (size_t i : other)
        ok[i] = verify_single(&proofs[i].ip_proof, &proofs[i], &V[i], nullptr, n, G, H, h) ? 1 : 0;
    return HIPBP_OK;
}

// ---- compact proof blobs (bp_codec.h, bp_codec.hip)
}  // extern "C"

namespace {

int codec_fail(const char* what, const char* why) {
    g_err = std::string(what) + ": " + why;
    return HIPBP_ERR_ARG;
}
// the arrays of one host struct as a one-proof batch (index 0): nothing is copied
bp::CodecArrays arrays_of_struct(const RangeProof& p) {
    RangeProof& q = const_cast<RangeProof&>(p);   // (the encoder only reads)
    bp::CodecArrays A;
    ge25519* pts[5] = {&q.V, &q.A, &q.S, &q.T1, &q.T2};
    for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
    A.t = (bp::fe*)&q.t; A.c = (bp::fe*)&q.ip_proof.c; A.x = (bp::fe*)&q.ip_proof.x;
    A.taux = (bp::fe*)&q.taux; A.mu = (bp::fe*)&q.mu;
    A.a = (bp::fe*)q.ip_proof.a.elements; A.b = (bp::fe*)q.ip_proof.b.elements;
    A.L = (bp::ge*)q.ip_proof.L.elements; A.R = (bp::ge*)q.ip_proof.R.elements;
    return A;
}
void free_proof_vectors(RangeProof& p) {
    free(p.ip_proof.a.elements); free(p.ip_proof.b.elements);
    free(p.ip_proof.L.elements); free(p.ip_proof.R.elements);
}

}  // namespace

extern "C" {

size_t hipbp_proof_blob_bound(size_t count, size_t ab_len, size_t L_len, unsigned flags) {
    return bp::CodecLayout{count, ab_len, L_len, (int)(flags & 1)}.bound();
}

int hipbp_proof_blob_header(const uint8_t* header32, size_t blob_bytes, hipbp_proof_blob_info* info) {
    if (!header32 || !info) return codec_fail("proof_blob_header", "null argument");
    if (const char* e = bp::codec_parse_header(header32, blob_bytes, info)) return codec_fail("proof_blob_header", e);
    return HIPBP_OK;
}

int hipbp_proof_blob_parse(const uint8_t* blob, size_t bytes, hipbp_proof_blob_info* info) {
    if (!info) return codec_fail("proof_blob_parse", "null argument");
    if (const char* e = bp::codec_parse(blob, bytes, info)) return codec_fail("proof_blob_parse", e);
    return HIPBP_OK;
}

int hipbp_batch_proof_encode(const hipbp_proof_batch* b, int with_blinding, uint8_t* blob_dev, size_t cap,
                             uint64_t* bytes_out_dev, void* stream) {
    if (!b || !blob_dev || !bytes_out_dev) return codec_fail("proof_encode", "null argument");
    if (const char* e = bp::codec_shape_error(b->count, b->n, b->ab_len, b->L_len, 0)) return codec_fail("proof_encode", e);
    if (b->count && !((b->Vp || b->V) && b->A && b->S && b->T1 && b->T2 && b->t && b->a && b->b && b->c && b->x &&
                      (!b->L_len || (b->L && b->R))))
        return codec_fail("proof_encode", "null batch field");
    if (with_blinding && b->count && (!b->taux || !b->mu)) return codec_fail("proof_encode", "with_blinding needs the batch's taux and mu");
    if ((uintptr_t)blob_dev % 8) return codec_fail("proof_encode", "blob_dev must be 8-byte aligned");
    const bp::CodecLayout l{b->count, b->ab_len, b->L_len, with_blinding ? 1 : 0};
    if (cap < l.bound()) return codec_fail("proof_encode", "cap below hipbp_proof_blob_bound");
    BP_ENGINE_OR_RET(e);
    bp::CodecArrays A;
    const ge25519* pts[5] = {b->Vp ? b->Vp : b->V, b->A, b->S, b->T1, b->T2};
    for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
    A.t = (bp::fe*)b->t; A.c = (bp::fe*)b->c; A.x = (bp::fe*)b->x; A.a = (bp::fe*)b->a; A.b = (bp::fe*)b->b;
    A.taux = with_blinding ? (bp::fe*)b->taux : nullptr; A.mu = with_blinding ? (bp::fe*)b->mu : nullptr;
    A.L = (bp::ge*)b->L; A.R = (bp::ge*)b->R;
    std::lock_guard<std::mutex> lk(e->mu);
    Buf(&cb)[bp::CDB_COUNT] = e->streams[pick(stream)].codec;
    size_t sz[bp::CDB_COUNT];
    {
        using namespace bp;
        const size_t count = b->count;
        BP_CODEC_BUFS(BP_BUF_SIZE)
    }
    // (a grown buffer frees the old one: the stream's earlier encode may still read it)
    if (sz[bp::CDB_BLK] > cb[bp::CDB_BLK].cap && cb[bp::CDB_BLK].p) BP_RET_ON(hipStreamSynchronize(pick(stream)));
    BP_RET_ON(need_all(cb, sz));
    bp::CodecWs w;
    {
        using namespace bp;
        Buf(&b)[CDB_COUNT] = cb;
        BP_CODEC_BUFS(BP_BUF_FIELD)
    }
    bp::launch_codec_encode(A, l, b->n, blob_dev, w, bytes_out_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_batch_proof_decode(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, hipbp_proof_out* o,
                             uint32_t* bad_dev, void* stream) {
    if (!blob_dev || !info || !o || !bad_dev) return codec_fail("proof_decode", "null argument");
    if (const char* e = bp::codec_shape_error(info->count, info->n, info->ab_len, info->L_len, info->flags))
        return codec_fail("proof_decode", e);
    const bp::CodecLayout l = bp::codec_layout(*info);
    if (info->raw_count > info->count || l.bytes(info->raw_count) != info->bytes || (l.Sc() == 0 && info->raw_count != info->count))
        return codec_fail("proof_decode", "info does not describe a blob (use hipbp_proof_blob_header)");
    if ((uintptr_t)blob_dev % 8) return codec_fail("proof_decode", "blob_dev must be 8-byte aligned");
    if (info->count && !(o->V && o->A && o->S && o->T1 && o->T2 && o->t && o->c && o->x && o->a && o->b &&
                         (!l.Lr || (o->L && o->R)) && (!l.f || (o->taux && o->mu))))
        return codec_fail("proof_decode", "null output array");
    BP_ENGINE_OR_RET(e);
    (void)e;
    bp::CodecArrays A;
    ge25519* pts[5] = {o->V, o->A, o->S, o->T1, o->T2};
    for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
    A.t = (bp::fe*)o->t; A.c = (bp::fe*)o->c; A.x = (bp::fe*)o->x; A.a = (bp::fe*)o->a; A.b = (bp::fe*)o->b;
    A.taux = l.f ? (bp::fe*)o->taux : nullptr; A.mu = l.f ? (bp::fe*)o->mu : nullptr;
    A.L = (bp::ge*)o->L; A.R = (bp::ge*)o->R;
    BP_RET_ON(hipMemsetAsync(bad_dev, 0, sizeof(uint32_t), pick(stream)));
    bp::launch_codec_decode(bp::codec_view(blob_dev, info->bytes, l, info->raw_count), A, l, bad_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_proofs_encode_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* blob,
                             size_t cap, size_t* bytes) {
    if (!blob || !bytes || (count && !proofs)) return codec_fail("proofs_encode_host", "null argument");
    const size_t abl = count ? proofs[0].ip_proof.a.length : 1, Lr = count ? proofs[0].ip_proof.L_len : 0;
    for (size_t i = 0; i < count; i++) {
        const InnerProductProof& ip = proofs[i].ip_proof;
        if (ip.a.length != abl || ip.b.length != abl || ip.L_len != Lr || ip.L.length < Lr || ip.R.length < Lr ||
            !ip.a.elements || !ip.b.elements || (Lr && (!ip.L.elements || !ip.R.elements)))
            return codec_fail("proofs_encode_host", ("proof " + std::to_string(i) +
                                                     ": another shape than the first proof's, or inconsistent vector lengths").c_str());
    }
    if (const char* e = bp::codec_shape_error(count, n, abl, Lr, 0)) return codec_fail("proofs_encode_host", e);
    const bp::CodecLayout l{count, abl, Lr, with_blinding ? 1 : 0};
    if (cap < l.bound()) return codec_fail("proofs_encode_host", "cap below hipbp_proof_blob_bound");
    // the device encoder's three steps, one proof at a time through the same bodies
    uint8_t* kind = blob + l.o_kind();
    memset(kind, 0, bp::pad8(count));
    size_t R = 0;
    for (size_t i = 0; i < count; i++) R += kind[i] = bp::codec_classify(arrays_of_struct(proofs[i]), l, 0);
    uint8_t* ridx = blob + l.o_rawidx();
    memset(ridx, 0, bp::pad8(4 * R));
    size_t j = 0;
    for (size_t i = 0; i < count; i++) {
        const bp::CodecArrays A = arrays_of_struct(proofs[i]);
        bp::codec_write_compact(blob + l.o_compact() + i * l.Sc(), A, l, 0, kind[i]);
        if (!kind[i]) continue;
        bp::put_le(ridx + 4 * j, i, 4);
        bp::codec_write_raw(blob + l.o_raw(R) + j * l.Sr(), A, l, 0);
        j++;
    }
    bp::codec_write_header(blob, l, n, R);
    *bytes = l.bytes(R);
    return HIPBP_OK;
}

int hipbp_proofs_decode_host(const uint8_t* blob, size_t bytes, RangeProof* proofs) {
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail("proofs_decode_host", e);
    if (info.count == 0) return HIPBP_OK;
    if (!proofs) return codec_fail("proofs_decode_host", "null proofs");
    const bp::CodecLayout l = bp::codec_layout(info);
    const size_t R = info.raw_count;
    memset(proofs, 0, info.count * sizeof(RangeProof));
    size_t j = 0, bad = 0, i = 0;
    bool oom = false;
    for (; i < info.count && !bad && !oom; i++) {
        RangeProof& p = proofs[i];
        if (!bp::proof_vectors_alloc(p.ip_proof, info.n, l.Lr, malloc, l.abl)) { oom = true; i++; break; }
        const uint8_t k = blob[l.o_kind() + i];
        bp::BlobView v;
        v.kind = blob + l.o_kind() + i; v.compact = blob + l.o_compact() + i * l.Sc();
        v.rawidx = blob + l.o_rawidx() + 4 * j; v.raw = blob + l.o_raw(R) + j * l.Sr();
        v.count = 1; v.R = k; v.base = i;
        v.kind_n = v.compact_n = 1; v.rawidx_n = v.raw_n = k;
        bp::CodecArrays A = arrays_of_struct(p);
        if (!l.f) A.taux = A.mu = nullptr;
        bad += bp::codec_decode_cpu(v, A, l);
        j += k;
    }
    if (bad || oom) {   // nothing stays allocated, every struct zero
        for (size_t k = 0; k < i; k++) free_proof_vectors(proofs[k]);
        memset(proofs, 0, info.count * sizeof(RangeProof));
        if (oom) { g_err = "proofs_decode_host: out of memory"; return HIPBP_ERR_DEVICE; }
        return codec_fail("proofs_decode_host", "a record failed its checks");
    }
    return HIPBP_OK;
}

int hipbp_batch_range_proof_verify_bytes_host(const uint8_t* blob, size_t bytes, const ge25519* V, size_t n,
                                              const PointVector* G, const PointVector* H, const ge25519* g,
                                              const ge25519* h, int check, int num_gpus, uint8_t* ok) {
    const char* me = "range_proof_verify_bytes_host";
    if (check != 1 && check != 2) return codec_fail(me, "check must be 1 or 2");
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail(me, e);   // before anything is uploaded
    if (info.n != n) return codec_fail(me, "n differs from the blob header's");
    if (!G || !H || !h || !G->elements || !H->elements || (info.count && !ok)) return codec_fail(me, "null argument");
    if (G->length != n || H->length != n) return codec_fail(me, "G and H must have n generators");
    if (check == 2 && !(info.flags & 1)) return codec_fail(me, "check 2 needs a blob with taux and mu");
    if (check == 2 && !g) return codec_fail(me, "check 2 needs g");
    if (info.count == 0) return HIPBP_OK;
    int rc = host_verify_shape(n, info.ab_len, info.L_len);
    if (rc != HIPBP_OK) return rc;
    HostFan fan;
    if ((rc = fan.open(info.count, num_gpus)) != HIPBP_OK) return rc;
    const bp::CodecLayout l = bp::codec_layout(info);
    return fan.run(info.count, [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return host_shard(dev, BlobChunks{blob, l, info.raw_count, n, sh.lo, V}, sh.hi - sh.lo, n, G, H, g, h, check, ok);
    });
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

// ---- proof ids and the batch Merkle root (bp_ids.h, bp_ids.hip)
namespace {

// the stream's ids workspace grown for a root over `leaves` ids / a blob of `count` proofs
int ids_workspace(Engine* e, hipStream_t s, size_t leaves, size_t count, bp::IdsWs& w) {
    Buf(&ib)[bp::IDB_COUNT] = e->streams[s].ids;
    size_t sz[bp::IDB_COUNT];
    bp::ids_sizes(leaves, count, sz);
    // (a grown buffer frees the old one: the stream's earlier call may still use it)
    bool grow = false;
    for (int k = 0; k < bp::IDB_COUNT; k++) grow = grow || (sz[k] > ib[k].cap && ib[k].p);
    if (grow) BP_RET_ON(hipStreamSynchronize(s));
    BP_RET_ON(need_all(ib, sz));
    {
        using namespace bp;
        Buf(&b)[IDB_COUNT] = ib;
        BP_IDS_BUFS(BP_BUF_FIELD)
    }
    return HIPBP_OK;
}

// fn(lo, hi) over [0, count) in contiguous parts on HIPBP_HOST_THREADS threads (unset: the machine's,
// 16 at most; at least 256 items a thread, so a small batch stays on the caller's thread)
template <class F>
void host_parts(size_t count, F fn) {
    const char* env = getenv("HIPBP_HOST_THREADS");
    size_t nt = env && atoi(env) > 0 ? (size_t)atoi(env) : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, (count + 255) / 256);
    if (nt <= 1) {
        fn((size_t)0, count);
        return;
    }
    std::vector<std::thread> workers;
    for (size_t k = 0; k < nt; k++) workers.emplace_back(fn, count * k / nt, count * (k + 1) / nt);
    for (auto& w : workers) w.join();
}

}  // namespace

extern "C" {

int hipbp_batch_proof_ids(const hipbp_proof_batch* b, int with_blinding, uint8_t* ids_dev, uint8_t* kind_dev,
                          void* stream) {
    if (!b || (b->count && !ids_dev)) return codec_fail("proof_ids", "null argument");
    if (const char* e = bp::codec_shape_error(b->count, b->n, b->ab_len, b->L_len, 0)) return codec_fail("proof_ids", e);
    if (b->count && !((b->Vp || b->V) && b->A && b->S && b->T1 && b->T2 && b->t && b->a && b->b && b->c && b->x &&
                      (!b->L_len || (b->L && b->R))))
        return codec_fail("proof_ids", "null batch field");
    if (with_blinding && b->count && (!b->taux || !b->mu)) return codec_fail("proof_ids", "with_blinding needs the batch's taux and mu");
    if ((uintptr_t)ids_dev % 4) return codec_fail("proof_ids", "ids_dev must be 4-byte aligned");
    if (b->count == 0) return HIPBP_OK;
    const bp::CodecLayout l{b->count, b->ab_len, b->L_len, with_blinding ? 1 : 0};
    BP_ENGINE_OR_RET(e);
    (void)e;
    bp::CodecArrays A;
    const ge25519* pts[5] = {b->Vp ? b->Vp : b->V, b->A, b->S, b->T1, b->T2};
    for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
    A.t = (bp::fe*)b->t; A.c = (bp::fe*)b->c; A.x = (bp::fe*)b->x; A.a = (bp::fe*)b->a; A.b = (bp::fe*)b->b;
    A.taux = with_blinding ? (bp::fe*)b->taux : nullptr; A.mu = with_blinding ? (bp::fe*)b->mu : nullptr;
    A.L = (bp::ge*)b->L; A.R = (bp::ge*)b->R;
    bp::launch_proof_ids(A, l, b->n, ids_dev, kind_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_blob_proof_ids(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, uint8_t* ids_dev, uint32_t* bad_dev,
                         void* stream) {
    if (!blob_dev || !info || !bad_dev || (info->count && !ids_dev)) return codec_fail("blob_proof_ids", "null argument");
    if (const char* e = bp::codec_shape_error(info->count, info->n, info->ab_len, info->L_len, info->flags))
        return codec_fail("blob_proof_ids", e);
    const bp::CodecLayout l = bp::codec_layout(*info);
    if (info->raw_count > info->count || l.bytes(info->raw_count) != info->bytes || (l.Sc() == 0 && info->raw_count != info->count))
        return codec_fail("blob_proof_ids", "info does not describe a blob (use hipbp_proof_blob_header)");
    if ((uintptr_t)blob_dev % 8) return codec_fail("blob_proof_ids", "blob_dev must be 8-byte aligned");
    if ((uintptr_t)ids_dev % 4 || (uintptr_t)bad_dev % 4) return codec_fail("blob_proof_ids", "ids_dev and bad_dev must be 4-byte aligned");
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    bp::IdsWs w;
    if (int rc = ids_workspace(e, pick(stream), 0, info->count, w)) return rc;
    bp::launch_blob_ids(bp::codec_view(blob_dev, info->bytes, l, info->raw_count), l, info->n, ids_dev, w, bad_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_merkle_root(const uint8_t* ids_dev, size_t count, uint8_t* root_dev, void* stream) {
    if (!root_dev || (count && !ids_dev)) return codec_fail("merkle_root", "null argument");
    if (count > bp::MERKLE_MAX_COUNT) return codec_fail("merkle_root", "count above 2^24");
    if ((uintptr_t)ids_dev % 4 || (uintptr_t)root_dev % 4) return codec_fail("merkle_root", "ids_dev and root_dev must be 4-byte aligned");
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    bp::IdsWs w;
    if (int rc = ids_workspace(e, pick(stream), count, 0, w)) return rc;
    bp::launch_merkle_root(ids_dev, count, root_dev, w, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_proof_ids_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* ids) {
    if (count && (!proofs || !ids)) return codec_fail("proof_ids_host", "null argument");
    const size_t abl = count ? proofs[0].ip_proof.a.length : 1, Lr = count ? proofs[0].ip_proof.L_len : 0;
    for (size_t i = 0; i < count; i++) {
        const InnerProductProof& ip = proofs[i].ip_proof;
        if (ip.a.length != abl || ip.b.length != abl || ip.L_len != Lr || ip.L.length < Lr || ip.R.length < Lr ||
            !ip.a.elements || !ip.b.elements || (Lr && (!ip.L.elements || !ip.R.elements)))
            return codec_fail("proof_ids_host", ("proof " + std::to_string(i) +
                                                 ": another shape than the first proof's, or inconsistent vector lengths").c_str());
    }
    if (const char* e = bp::codec_shape_error(count, n, abl, Lr, 0)) return codec_fail("proof_ids_host", e);
    const bp::CodecLayout l{count, abl, Lr, with_blinding ? 1 : 0};
    host_parts(count, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) bp::ids_flat_proof(arrays_of_struct(proofs[i]), l, n, 0, ids + bp::ID_BYTES * i);
    });
    return HIPBP_OK;
}

int hipbp_blob_proof_ids_host(const uint8_t* blob, size_t bytes, uint8_t* ids) {
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail("blob_proof_ids_host", e);
    if (info.count && !ids) return codec_fail("blob_proof_ids_host", "null ids");
    const bp::CodecLayout l = bp::codec_layout(info);
    const bp::BlobView v = bp::codec_view(blob, bytes, l, info.raw_count);
    std::atomic<size_t> bad{0};
    host_parts(info.count, [&](size_t lo, size_t hi) {
        size_t b = 0;
        for (size_t i = lo; i < hi; i++) b += bp::ids_blob_proof(v, l, info.n, i, ids + bp::ID_BYTES * i);
        bad += b;
    });
    if (bad) {   // (not after a full parse)
        memset(ids, 0, info.count * bp::ID_BYTES);
        return codec_fail("blob_proof_ids_host", "a record failed its checks");
    }
    return HIPBP_OK;
}

int hipbp_merkle_root_host(const uint8_t* ids, size_t count, uint8_t root[32]) {
    if (!root || (count && !ids)) return codec_fail("merkle_root_host", "null argument");
    if (count > bp::MERKLE_MAX_COUNT) return codec_fail("merkle_root_host", "count above 2^24");
    if (count == 0) {
        uint32_t d[8];
        bp::merkle_empty(d);
        bp::ids_store(root, d);
        return HIPBP_OK;
    }
    std::vector<std::vector<uint8_t>> lv;
    bp::merkle_levels_cpu(ids, count, lv);
    memcpy(root, lv.back().data(), bp::ID_BYTES);
    return HIPBP_OK;
}

int hipbp_merkle_path_host(const uint8_t* ids, size_t count, size_t index, uint8_t* path, size_t* path_len) {
    if (!ids || !path || !path_len) return codec_fail("merkle_path_host", "null argument");
    if (count > bp::CODEC_MAX_COUNT) return codec_fail("merkle_path_host", "count above 2^22");
    if (index >= count) return codec_fail("merkle_path_host", "index not below count");
    std::vector<std::vector<uint8_t>> lv;
    bp::merkle_levels_cpu(ids, count, lv);
    *path_len = bp::merkle_path_cpu(lv, count, index, path);
    return HIPBP_OK;
}

int hipbp_merkle_verify_host(const uint8_t id[32], size_t index, size_t count, const uint8_t* path, size_t path_len,
                             const uint8_t root[32]) {
    if (!id || !root || (path_len && !path)) return 0;
    return bp::merkle_verify_cpu(id, index, count, path, path_len, root) ? 1 : 0;
}

}  // extern "C"

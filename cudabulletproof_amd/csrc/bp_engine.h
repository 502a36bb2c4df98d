// bp_engine.h — what the C ABI's translation units share (internal; the ABI: include/cudabulletproof_hip.h):
//   bp_api_engine.hip  the engine, the device-data verifiers, pipelines, generator sets, MSMs, probes
//   bp_api_prove.hip   the device-data provers and Pedersen commitments
//   bp_api_host.hip    the host-data provers, commitments and verifiers, sharded over devices
//   bp_api_blob.hip    proof blobs, proof ids and Merkle roots
//   bp_api_ref.hip     the reference's cuda_* surface (Part 1)
// All of it lies in a namespace of hidden visibility (the library exports the C ABI alone); what must
// exist once (engines, g_err, g_accept_stats, the tick-size bounds) is defined in bp_api_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cudabulletproof_hip.h"
#include "bp_tick_plan.h"
#include "bp_buf.h"
#include "bp_host_prove.h"
#include "ge25519_dev.h"

static_assert(sizeof(fe25519) == 32, "fe25519 layout");
static_assert(sizeof(ge25519) == 128, "ge25519 layout");
static_assert(sizeof(bp::fe) == 32 && sizeof(bp::ge) == 128, "device layout");
static_assert(sizeof(InnerProductProof) == 144, "InnerProductProof layout (SURVEY 8b)");
static_assert(sizeof(RangeProof) == 880, "RangeProof layout (SURVEY 8b)");

namespace bpe __attribute__((visibility("hidden"))) {

using bp::Buf;
using bp::GenView;
using bp::PinnedBuf;
using bp::need_all;

extern thread_local std::string g_err;   // hipbp_last_error's message

// Part 1's convention on a device error (CUDA_CHECK, cuda_bulletproof_kernels.cu:13-21) ...
#define BP_EXIT_ON(call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "HIP error at %s:%d - %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(EXIT_FAILURE);                                                               \
        }                                                                                     \
    } while (0)

// ... and Part 2's
#define BP_RET_ON(call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return HIPBP_ERR_DEVICE;                                                          \
        }                                                                                     \
    } while (0)

// HIP-event timing of the verify pipeline's kernels (bench.py's live roofline numbers).
struct EventTimer {
    struct Rec { int kind; hipEvent_t a, b; };
    bool on = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<Rec> pending;
    hipEvent_t open[bp::KT_COUNT] = {};
    double total_ms[bp::KT_COUNT] = {};
    uint64_t count[bp::KT_COUNT] = {};

    void mark(int kind, bool end, hipStream_t s) {
        if (used == pool.size()) {
            hipEvent_t fresh;
            if (hipEventCreate(&fresh) != hipSuccess) return;
            pool.push_back(fresh);
        }
        hipEvent_t e = pool[used++];
        (void)hipEventRecord(e, s);
        if (!end)
            open[kind] = e;
        else
            pending.push_back(Rec{kind, open[kind], e});
    }
    hipError_t collect();
    void reset();
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

    hipError_t init();
    hipError_t upload(void* dst, const void* src, size_t bytes);
    std::vector<bp::fe> two_host;
    std::vector<bp::fe*> two_retired;
    hipError_t ensure_two(int n);
};

extern Engine* engines[64];
extern std::mutex engines_mu;
Engine* engine_or_null(hipError_t* err);
Engine& engine_or_exit();

// How an entry point begins: the current device's engine as `e` (and `err`, for its own HIP calls),
// or HIPBP_ERR_DEVICE with the runtime's message.
#define BP_ENGINE_OR_RET(e)           \
    hipError_t err;                   \
    Engine* e = engine_or_null(&err); \
    BP_RET_ON(err)

// Part-2 entry points run on the caller's stream; NULL is the default (null) stream, as for a
// kernel launch — the stream torch reports as 0 — so work stays ordered with the caller's.
inline hipStream_t pick(void* s) { return (hipStream_t)s; }

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

constexpr size_t MAX_N = size_t(1) << 16;   // generators per proof (range bits / IPA length)

inline int log2i(size_t n) {
    int k = 0;
    while ((size_t(1) << k) < n) k++;
    return k;
}

// a blob or id entry point's "<entry point>: <reason>" argument error
inline int codec_fail(const char* what, const char* why) {
    g_err = std::string(what) + ": " + why;
    return HIPBP_ERR_ARG;
}

int check_batch(const hipbp_proof_batch* b, int range_mode);
bp::BatchView view_of(const hipbp_proof_batch* b);

// A generator set (hipbp_gens_create): a device snapshot of its generators in GenView's packed order
// and, optionally, their fixed-base prefix tables (bp::launch_prefix_tables, same base order).
struct Gens {
    int device = -1;
    size_t n = 0;
    Buf gen, tab;
    int bits = 0;
    GenView view() const { return GenView::at(gen.p, n).with_tables(tab.p, bits); }
    void release() { (void)gen.release(); (void)tab.release(); }
};

// What every _gens entry point checks of its generator set: that it is there, that it holds the
// call's n (`what` is the entry point's own message; null: the call brings no n) and that it was
// created on the current device.
int gens_check(const void* gens, size_t n, const char* what);

// Drain-tick thresholds (bp::plan_tick): ticks with at most this many scalar-multiplication items
// run them on lane quads, up to PAIR_MAX_ITEMS on lane pairs.  The cost model (tools/ubench_issue.hip
// with -DLAT: one wave alone issues one instruction per ~9 cycles, the SIMD one per ~4.4): a tick
// lasts about (instructions per wave) x max(9, 4.4 w) cycles for w waves per SIMD, counting the other
// pipeline's concurrent tick (they drain side by side).  Quads cut the instructions per wave of a
// point operation from ~1700 to ~750 for 4x the lanes, pairs to ~1140 for 2x: with both pipelines'
// drains together, a 65,536-item tick is fastest on lanes, 32,768 on pairs, 16,384 on quads
// (configs[4] shard: 173.8 K verifies/s vs 172.1 K with the round-3 bounds 49,152 / 98,304).
// 16-lane rows (sm_row) up to ROW_MAX_ITEMS items: a one-proof call's ticks (r04b, one MI355X, warm
// cuda_range_proof_verify: n = 16 4.9 -> 4.0 ms, n = 64 6.7 -> 5.5 ms)
extern const unsigned long long ROW_MAX_ITEMS, QUAD_MAX_ITEMS, PAIR_MAX_ITEMS;

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
    // generator set's, lend_tables: ext_tab, borrowed); pbits = 0: none
    Buf ptab;
    const bp::ge* ext_tab = nullptr;
    int pbits = 0;
    const bp::ge* tables() const { return ext_tab ? ext_tab : ptab.as<bp::ge>(); }
    void set_gens(const GenView& gv) { G = gv.G; H = gv.H; g = gv.g; h = gv.h; }   // (its tables: lend_tables)
    // borrowed tables (null, 0: none) in the place of any the pipeline had; a pipeline that owns
    // tables (ptab) takes none: the caller releases those first
    void lend_tables(const bp::ge* tab, int bits) {
        assert(!ptab.p);
        ext_tab = tab;
        pbits = bits;
    }
    bool busy() const {
        for (int k = 0; k < D; k++) if (ring[k].active) return true;
        return false;
    }
    hipError_t init(Engine* eng, hipStream_t st, int nn, int range);
    void release();
    // The batch's lane-order buffers and sort plan (its per-lane item sets: bp::lane_sort_sets).
    hipError_t plan_sort(Slot& sl, int idx);
    hipError_t carve(Slot& sl, size_t B, size_t Lb);
    // One tick; `b` may be null (drain).  Outputs of `b` are written when it completes.
    int push(const hipbp_proof_batch* b, const ge25519* P_in, uint8_t* ok, ge25519* P_out, ge25519* chk,
             uint8_t* flags_out = nullptr, ge25519* poly_out = nullptr);
    int flush();
};

// The engine's cached one-shot pipeline for (stream, n, mode); created on first use.  Cached only
// once fully initialised (a failed init is released, never reused).
int pipeline_for(Engine& e, hipStream_t s, size_t max_batch, int n, int range_mode, Pipeline** out);

// A call's generators and prefix tables on the engine's cached one-shot pipelines, for that call
// only: the pipelines are shared with the calls that bring no tables, and the ticks' slot records
// take the table pointer at push.  Made under e->mu once the call has its pipelines; going out of
// scope (still under e->mu, after the call's flush) it takes the tables back on every return path.
struct TableLoan {
    Pipeline* pl[2];
    TableLoan(const GenView& gv, Pipeline* a, Pipeline* b = nullptr) : pl{a, b} {
        for (Pipeline* p : pl)
            if (p) { p->set_gens(gv); p->lend_tables(gv.tab, gv.bits); }   // (cached pipelines own no tables)
    }
    ~TableLoan() {
        for (Pipeline* p : pl)
            if (p) p->lend_tables(nullptr, 0);
    }
    TableLoan(const TableLoan&) = delete;
};

// One-shot verify of a whole batch on `s` (push + drain of a cached pipeline); e.mu held.
int run_verify(Engine& e, const hipbp_proof_batch* batch, const ge25519* P_in, const GenView& gv, uint8_t* ok,
               ge25519* P_out, ge25519* chk_out, int range_mode, hipStream_t s, uint8_t* flags_out = nullptr,
               ge25519* poly_out = nullptr);

// `count` canonical-tree MSMs of n points each on stream s, in s's own workspace; e.mu held.
hipError_t msm_run(Engine& e, bp::ge* results, const bp::fe* scalars, const bp::ge* points, size_t n, size_t count,
                   hipStream_t s, const bp::ge* ptab = nullptr, int K = 0);

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

// ---- one surface's functions that another calls
// bp_api_prove.hip.  The seeded and the accepted prover on device data (the host provers' shards run
// them chunk by chunk), their shared shape check, the accepted prover's record of what the last call
// on this thread did (tools/bench_prove_accepted.py: the proofs proved per round and, with
// HIPBP_ACCEPT_TIMING=1, the loop's own kernels' times), and Pedersen commitments over one device array.
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
// (constant-initialised, and declared so: otherwise every other translation unit calls the object's
// thread-local init function before it touches it, a weak hidden symbol that nothing defines)
[[clang::require_constant_initialization]] extern thread_local AcceptStats g_accept_stats;
int seed_check(const uint8_t* seed32, const fe25519* v, const fe25519* gamma, size_t count, size_t n);
int prove_seeded(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, const GenView& gv,
                 hipbp_proof_out* out, void* stream);
int prove_accepted(const hipbp_prove_input* in, const uint8_t* seed32, uint64_t index_base, int max_attempts, int check,
                   const GenView& gv, hipbp_proof_out* out, uint8_t* attempts, void* stream);
size_t env_commit_chunk(size_t count);   // HIPBP_COMMIT_CHUNK for a call of `count` (bp::commit_chunk's rule)
int commit_run(Engine& e, ge25519* out, uint8_t* ok, const ge25519* V, const fe25519* v, const fe25519* gamma,
               size_t count, const GenView& gv, hipStream_t s);
// ... the stand-alone IPA prover's enqueue (Q = gv.h); e.mu held
int ipa_enqueue(Engine& e, const hipbp_ipa_prove_input* in, const GenView& gv, const hipbp_ipa_proof_out* out,
                hipStream_t s);
// bp_api_ref.hip.  One proof of the reference's host structs through the one-shot verify, synchronously
// (rp null: the inner-product verify of P), with Part 1's conventions.
bool verify_single(const InnerProductProof* ip, const RangeProof* rp, const ge25519* V, const ge25519* P, size_t n,
                   const PointVector* G, const PointVector* H, const ge25519* h);

}  // namespace bpe

// bp_tick_plan.h — the verify pipeline's tick planner (internal to the library).  Host-only and
// pure: no HIP runtime calls, so tests/tick_plan_check.hip runs every plan on a CPU.
#pragma once
#include "bp_kernels.h"

namespace bp {

// The pipeline's layout knobs (Pipeline::init reads them once) and one ring slot's planning state.
struct PlanConfig {
    int n = 0;
    int range_mode = 1;       // 0 inner product only, 1 cuda_range_proof_verify, 2 range_proof_verify
    bool lane_tree = false;   // MSM trees as RK_LTREE lanes (n <= HIPBP_LANE_TREE_MAX), else RK_TREE blocks
    int quad_force = -1;      // lanes per scalar multiplication forced on every tick (-1: by size)
    unsigned long long row_max = 0, quad_max = 0, pair_max = 0;   // size bounds of the tick forms
    int lane_sort_mask = 7;   // bit 0 stage 0, bit 1 rounds, bit 2 final terms, bit 3 shortest first
};
struct PlanSlot {
    bool active = false;
    int stage = 0;
    unsigned long long B = 0;
    int L = 0;       // the batch's fold rounds (L_len)
    int defer = 0;   // its stage 0 is split (SlotDev::defer)
};

// ------------------------------------------------------------------ the stage table
// Every tick is ONE k_terms launch over all in-flight batches, each at its own stage; within a batch
// the reference's order is kept exactly, across batches nothing depends on anything.  A round-r
// item forms its own input point G'/H' from two round r-1 terms (each folded point has exactly one
// consumer), so the fold combinations need no launch of their own.  batch_schedule() below is the
// one statement of which stage of a batch with L fold rounds runs which region:
//   0: RK_PREP (challenges, MSM scalars, round challenges)
//   1: RK_STAGE0 (both MSMs' point terms, fold round 0, t*h, c*Q [, the 7 polynomial terms])
//   2: RK_TREE (MSM trees of n > LANE_TREE_MAX points) [, RK_POLY]   r+1 (1 <= r < L): RK_ROUND r
//   FT = L+1 (1 when L = 0): RK_FINAL_TERMS           mode 2, max(3, FT): RK_M3
//   min(3, FIN - 1): RK_LTREE (the trees of n <= LANE_TREE_MAX MSMs, one lane per proof: they need
//     only stage 0's terms, so a drain's last tick is the short P / check-point assembly alone)
//   FIN = 1 + the last of those: RK_FINAL (P, check point, accept)
// A split batch (defer; hipbp_pipeline_defer_msm / HIPBP_DEFER_MSM=1) runs only fold round 0 (+ the
// polynomial terms) in its stage-0 tick (S0_CRIT).  Its MSM terms, t*h and c*Q (S0_DEFER, read only by
// the lane trees and the final assembly) run as L - 1 equal wave-aligned RK_MSMT chunks in its
// fold-round ticks, stages 2 .. L, whose items shrink round by round (r04k: better than a shorter
// or a weighted span), and its lane trees move to stage L + 1.  For a finite batch (configs[4]'s shards)
// the rounds that would run half empty before the latency-bound last ticks carry the MSM work.
// The lane trees must land at least one tick before the final assembly, and always do:
// FIN >= FT + 1 = L + 2 > L + 1.
enum RegionGroup { RG_TREE = 0, RG_SM = 1, RG_CHAIN = 2 };   // a tick's order: block trees, scalar mults, chains
struct SchedEntry {
    int stage, kind, r, group;
    unsigned align;
    unsigned long long items;
};
constexpr int MAX_ROUNDS = 16;                 // log2(MAX_N)
constexpr int MAX_SCHED = 2 * MAX_ROUNDS + 8;
constexpr int MAX_DEPTH = MAX_ROUNDS + 3;      // pipeline_depth(n = 65536)
struct Schedule {
    int fin = 0;   // the batch's last stage: it retires after fin + 1 ticks
    int count = 0;
    SchedEntry e[MAX_SCHED];
};
// lanes [lo, hi) of chunk k of m of a split stage 0's deferred part (total lanes)
inline void msm_chunk(unsigned long long total, int m, int k, unsigned long long& lo, unsigned long long& hi) {
    auto cut = [&](int j) { return j >= m ? total : total / 64 * (unsigned long long)j / (unsigned long long)m * 64; };
    lo = cut(k);
    hi = cut(k + 1);
}
// Entries of one group that share a stage are listed in the order the tick lays them out.
inline Schedule batch_schedule(const PlanConfig& c, unsigned long long B, int L, int defer) {
    Schedule s{};
    const int n = c.n, mode = c.range_mode;
    const int ft = L > 0 ? L + 1 : 1, m3 = ft > 3 ? ft : 3;
    int last = ft;
    if (mode && last < 2) last = 2;   // the MSM trees
    if (mode == 2 && m3 > last) last = m3;
    s.fin = last + 1;
    auto add = [&s](int stage, int kind, int r, unsigned long long items, int group, unsigned align = 64) {
        if (items) s.e[s.count++] = SchedEntry{stage, kind, r, group, align, items};
    };
    if (mode && !c.lane_tree) add(2, RK_TREE, 0, B * 2 * n, RG_TREE, 256);
    add(1, RK_STAGE0, 0, stage0_lanes(B, n, L, mode, defer ? S0_CRIT : S0_ALL).total, RG_SM);
    for (int st = 2; st <= L; st++) add(st, RK_ROUND, st - 1, B * 4 * (unsigned long long)(n >> st), RG_SM);
    const unsigned long long deferred = defer ? stage0_lanes(B, n, L, mode, S0_DEFER).total : 0;
    for (int st = 2; defer && st <= L; st++) {
        unsigned long long lo, hi;
        msm_chunk(deferred, L - 1, st - 2, lo, hi);
        add(st, RK_MSMT, (int)lo, hi - lo, RG_SM);
    }
    add(ft, RK_FINAL_TERMS, 0, B * 2, RG_SM);
    if (mode == 2) add(m3, RK_M3, 0, B * 2, RG_SM);
    add(s.fin, RK_FINAL, 0, B, RG_CHAIN);
    if (mode && c.lane_tree) add(defer ? L + 1 : (s.fin - 1 < 3 ? s.fin - 1 : 3), RK_LTREE, 0, B, RG_CHAIN);
    if (mode == 2) add(2, RK_POLY, 0, B, RG_CHAIN);
    add(0, RK_PREP, 0, mode ? 2 * B : B, RG_CHAIN);
    return s;
}
// ring slots: a full-L batch's slot is free again when the ring comes round (fewer rounds finish earlier)
inline int pipeline_depth(const PlanConfig& c) { return batch_schedule(c, 1, log2n(c.n), 0).fin + 1; }
// A split batch adds one RK_MSMT region to each of its stages 2 .. L: in steady state a tick then
// holds up to 2 L + 5 regions (RK_STAGE0, L - 1 RK_ROUND + L - 1 RK_MSMT, RK_FINAL_TERMS, RK_M3,
// RK_FINAL, RK_LTREE, RK_POLY, RK_PREP), which must fit the kernel's region list (n <= 512 when
// HIPBP_LANE_TREE_MAX raises the lane-tree limit; the default limit is n <= 64, 17 regions).
inline bool defer_ok(const PlanConfig& c) {
    return c.range_mode != 0 && c.lane_tree && log2n(c.n) >= 2 && 2 * log2n(c.n) + 5 <= MAX_REGIONS;
}
inline bool batch_defers(const PlanConfig& c, int L) { return defer_ok(c) && L >= 2; }

// ------------------------------------------------------------------ one tick
enum PlanError { PLAN_OK = 0, PLAN_OVERFLOW /* region list */, PLAN_TOO_LARGE /* >= 2^32 lanes */ };
struct TickPlan {
    RegionList rl;
    int ql;   // lanes per scalar-multiplication item: k_terms<ql>
};
// The tick over the ring's active slots, newest first from `head` within each group: the
// (block-aligned) tree regions, which must start the list; the scalar multiplications; the
// per-proof chains (final assembly, lane trees, polynomial sides, challenges) last (measured faster
// than at the grid's start: 138.7 K vs 130.6 K verifies/s).  k_terms' find_region relies on this order.
inline PlanError plan_tick(const PlanConfig& c, const PlanSlot* slots, int D, int head, TickPlan& out) {
    RegionList& tr = out.rl;
    tr = RegionList{};
    Schedule sch[MAX_DEPTH];
    for (int k = 0; k < D; k++)
        if (slots[k].active) sch[k] = batch_schedule(c, slots[k].B, slots[k].L, slots[k].defer);
    for (int group = RG_TREE; group <= RG_CHAIN; group++)
        for (int k = 0; k < D; k++) {
            const int idx = (head - k + D) % D;
            const PlanSlot& sl = slots[idx];
            if (!sl.active) continue;
            const Schedule& s = sch[idx];
            for (int i = 0; i < s.count; i++) {
                const SchedEntry& e = s.e[i];
                if (e.stage != sl.stage || e.group != group) continue;
                if (tr.count == MAX_REGIONS) return PLAN_OVERFLOW;
                tr.reg[tr.count++] = Region{e.kind, idx, e.r, 0, tr.total, e.items};
                tr.total += (e.items + e.align - 1) & ~(unsigned long long)(e.align - 1);   // wave / block aligned
            }
        }
    // Tick form: a tick whose scalar multiplications cannot fill the SIMDs (the last fold rounds and
    // final terms of the last batches, a one-proof verify) lasts one scalar-multiplication chain's
    // latency; its items then take a 16-lane row, a lane quad (3 product latencies per point op instead
    // of 9) or a lane pair each, by their number against row_max, quad_max and pair_max.
    unsigned long long sm_items = 0, all_items = 0;
    for (int k = 0; k < tr.count; k++) {
        all_items += tr.reg[k].items;
        if (region_is_sm(tr.reg[k].kind)) sm_items += tr.reg[k].items;
    }
    out.ql = sm_items <= c.row_max ? 16 : sm_items <= c.quad_max ? 4 : sm_items <= c.pair_max ? 2 : 1;
    // a tick of chains alone: the chains on quads, in the row-form kernel when the tick is small (a
    // one-proof call's ticks then load one tick code object, not two)
    if (!sm_items) out.ql = all_items <= c.row_max ? 16 : 4;
    if (c.quad_force >= 0) out.ql = c.quad_force;
    if (out.ql > 1) {   // re-lay the regions: scalar-multiplication items ql lanes each
        tr.total = 0;
        for (int k = 0; k < tr.count; k++) {
            Region& g = tr.reg[k];
            g.items *= region_lanes(g.kind, out.ql);
            g.begin = tr.total;
            const unsigned long long al = g.kind == RK_TREE ? 256 : 64;
            tr.total += (g.items + al - 1) & ~(al - 1);
        }
    }
    return tr.total >= (1ull << 32) ? PLAN_TOO_LARGE : PLAN_OK;
}
// After a tick: every batch moves on one stage or retires, and the ring turns.
inline void advance_ring(const PlanConfig& c, PlanSlot* slots, int D, int& head) {
    for (int k = 0; k < D; k++) {
        PlanSlot& sl = slots[k];
        if (!sl.active) continue;
        if (sl.stage == batch_schedule(c, sl.B, sl.L, sl.defer).fin) sl.active = false;
        else sl.stage++;
    }
    head = (head + 1) % D;
}

// ------------------------------------------------------------------ admission
// May a batch (B, L, defer) be staged in slot `head`?  PLAN_OK: yes, and then every tick the ring
// still needs plans, whatever is admitted after it (each later batch passes this test itself).
// Otherwise the error the ring would run into with the batch in it; the caller stages nothing.
// Batches of different round counts can reach their two-region stages in one tick (round counts
// descending by one per push all run RK_FINAL_TERMS together), which the region list cannot always
// hold, so the ring is played forward on a copy, the candidate included, until it is idle: the
// ticks of a drain, and further pushes are tested against what is then in flight.  An idle ring
// admits every batch that plans at all, so a refused batch is admitted after at most D drain ticks.
// A ring whose batches all share the candidate's (L, defer) has at most one batch per stage: L + 6
// regions, 2 L + 5 when split (defer_ok), both within MAX_REGIONS; and a batch's items of all its
// stages together are below B (8 n + 24) (RK_TREE 2 n B, stage 0 (4 n + 9) B, the rounds 2 n B, the
// one-per-proof regions 9 B), 16 lanes each at the most, with the regions' alignment far below 2^20
// lanes: such a ring needs no replay (the steady state's push scans its D slots and no more).
inline PlanError push_admits(const PlanConfig& c, const PlanSlot* slots, int D, int head, unsigned long long B,
                             int L, int defer) {
    bool uniform = true;
    unsigned long long sumB = B;
    for (int k = 0; k < D; k++)
        if (slots[k].active) {
            uniform &= slots[k].L == L && slots[k].defer == defer;
            sumB += slots[k].B;
        }
    if (uniform && sumB < ((1ull << 32) - (1ull << 20)) / (16ull * (8ull * c.n + 24))) return PLAN_OK;
    PlanSlot sim[MAX_DEPTH];
    for (int k = 0; k < D; k++) sim[k] = slots[k];
    sim[head] = PlanSlot{true, 0, B, L, defer};
    for (bool busy = true; busy;) {
        TickPlan t;
        const PlanError pe = plan_tick(c, sim, D, head, t);
        if (pe != PLAN_OK) return pe;
        advance_ring(c, sim, D, head);
        busy = false;
        for (int k = 0; k < D; k++) busy |= sim[k].active;
    }
    return PLAN_OK;
}

// ------------------------------------------------------------------ the lane sort's sets
// A batch's per-lane item sets in perm order (stage 0's per-lane classes, the rounds whose scalar
// runs are shorter than a wave, the final terms), for batches of at least LANE_SORT_MIN proofs
// (HIPBP_LANE_SORT=0 turns the sort off, for A/B runs); count = 0: no sort.
constexpr unsigned long long LANE_SORT_MIN = 64;
struct SortSets {
    int count = 0;
    unsigned blocks = 0;
    unsigned long long total = 0;   // items of all sets = the perm buffer's length
    struct Set {
        int kind, r;
        unsigned long long items;
        unsigned block0;
    } set[LANE_SORT_SETS];
};
inline SortSets lane_sort_sets(const PlanConfig& c, unsigned long long B, int L) {
    SortSets s{}, none{};
    if (B < LANE_SORT_MIN) return none;
    auto add = [&s](int kind, int r, unsigned long long items) {
        s.set[s.count++] = {kind, r, items, s.blocks};
        s.blocks += (unsigned)((items + LANE_SORT_BLOCK - 1) / LANE_SORT_BLOCK);
        s.total += items;
    };
    const Stage0Lanes z = stage0_lanes(B, c.n, L, c.range_mode);
    for (int k = 0; k < 4; k++)   // one set per class, contiguous in perm0 (stage0_item)
        if (z.size[k] && (c.lane_sort_mask & 1)) add(SS_STAGE0, k, z.size[k]);
    for (int r = 1; r < L; r++)
        if (round_per_lane(c.n, r) && (c.lane_sort_mask & 2)) add(SS_ROUND, r, B * 4 * (unsigned long long)(c.n >> (r + 1)));
    if (c.lane_sort_mask & 4) add(SS_FT, 0, B * 2);
    return s.total > 0xFFFFFFFFull ? none : s;
}
}  // namespace bp

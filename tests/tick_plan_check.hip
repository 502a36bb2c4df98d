// tick_plan_check.hip — TEST INFRASTRUCTURE (tests/test_tick_plan.py).
//
// Runs the verify pipeline's tick planner (cudabulletproof_amd/csrc/bp_tick_plan.h, host-only) on
// the CPU, driving the ring exactly as Pipeline::push does (stage a batch in slot `head`, plan the
// tick, advance the ring).
//   replay: reads "cfg n mode lane_tree quad_force row_max quad_max pair_max sort_mask", then
//           "push B L defer" / "tick" (a drain tick) / "flush" lines from stdin and prints "depth D",
//           then for every accepted push a "sort blocks count (kind r items block0)*" line, for every
//           refused push (push_admits) "refused E" and nothing else, and for every tick a
//           "tick ql count total (kind slot r begin items)*" line: the rows of tests/golden/tick_plans.json.
//   sweep:  the planner's invariants over the whole parameter space, then free-form rings (every
//           push with its own B, L and defer, drain ticks mixed in) under the admission contract;
//           prints "<cases> <failures>", exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_tick_plan.h"

using namespace bp;
typedef unsigned long long u64;

struct Ring {
    PlanConfig c;
    int D, head = 0;
    PlanSlot slot[MAX_DEPTH];
    explicit Ring(const PlanConfig& cfg) : c(cfg), D(pipeline_depth(cfg)) {}
    bool busy() const {
        for (int k = 0; k < D; k++) if (slot[k].active) return true;
        return false;
    }
    bool stage(u64 B, int L, bool want_defer) {   // false: the slot is still busy
        if (slot[head].active) return false;
        slot[head] = PlanSlot{true, 0, B, L, (want_defer && batch_defers(c, L)) ? 1 : 0};
        return true;
    }
};

static void print_tick(const TickPlan& t) {
    std::printf("tick %d %d %llu", t.ql, t.rl.count, t.rl.total);
    for (int k = 0; k < t.rl.count; k++) {
        const Region& g = t.rl.reg[k];
        std::printf(" %d %d %d %llu %llu", g.kind, g.slot, g.r, g.begin, g.items);
    }
    std::printf("\n");
}

static int replay() {
    PlanConfig c;
    int lt = 0;
    if (std::scanf(" cfg %d %d %d %d %llu %llu %llu %d", &c.n, &c.range_mode, &lt, &c.quad_force, &c.row_max,
                   &c.quad_max, &c.pair_max, &c.lane_sort_mask) != 8) return 2;
    c.lane_tree = lt != 0;
    Ring R(c);
    std::printf("depth %d\n", R.D);
    char op[16];
    auto tick = [&R]() {
        TickPlan t;
        const PlanError pe = plan_tick(R.c, R.slot, R.D, R.head, t);
        if (pe != PLAN_OK) { std::printf("error %d\n", (int)pe); return false; }
        print_tick(t);
        advance_ring(R.c, R.slot, R.D, R.head);
        return true;
    };
    while (std::scanf(" %15s", op) == 1) {
        if (!std::strcmp(op, "flush")) {
            while (R.busy()) if (!tick()) return 1;
            continue;
        }
        if (!std::strcmp(op, "tick")) {   // a drain tick: push(NULL)
            if (!tick()) return 1;
            continue;
        }
        u64 B;
        int L, defer;
        if (std::strcmp(op, "push") || std::scanf(" %llu %d %d", &B, &L, &defer) != 3) return 2;
        if (R.slot[R.head].active) { std::printf("error busy\n"); return 1; }
        const PlanError adm = push_admits(c, R.slot, R.D, R.head, B, L, (defer && batch_defers(c, L)) ? 1 : 0);
        if (adm != PLAN_OK) { std::printf("refused %d\n", (int)adm); continue; }   // nothing staged, no tick
        R.stage(B, L, defer != 0);
        const SortSets ss = lane_sort_sets(c, B, L);
        std::printf("sort %u %d", ss.blocks, ss.count);
        for (int k = 0; k < ss.count; k++)
            std::printf(" %d %d %llu %u", ss.set[k].kind, ss.set[k].r, ss.set[k].items, ss.set[k].block0);
        std::printf("\n");
        if (!tick()) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------- sweep
static int g_cases = 0, g_fails = 0;
static const char* g_what = "";
static void fail(const PlanConfig& c, u64 B, int L, int defer, const char* msg) {
    g_fails++;
    if (g_fails <= 20)
        std::printf("FAIL %s: %s (n %d mode %d lane_tree %d B %llu L %d defer %d)\n", g_what, msg, c.n, c.range_mode,
                    (int)c.lane_tree, B, L, defer);
}
#define CHECK(cond, msg) do { if (!(cond)) fail(c, B, L, defer, msg); } while (0)

// properties of one batch's schedule
static void check_schedule(const PlanConfig& c, u64 B, int L, int defer) {
    const Schedule s = batch_schedule(c, B, L, defer);
    CHECK(s.count <= MAX_SCHED, "schedule too long");
    int st_final = -1, st_ltree = -1;
    u64 next = 0;
    bool chunks_ok = true;
    for (int i = 0; i < s.count; i++) {
        const SchedEntry& e = s.e[i];
        CHECK(e.stage >= 0 && e.stage <= s.fin, "stage outside 0 .. fin");
        CHECK(e.align == (e.kind == RK_TREE ? 256u : 64u), "alignment");
        CHECK(e.group == (e.kind == RK_TREE ? RG_TREE : region_is_sm(e.kind) ? RG_SM : RG_CHAIN), "group");
        if (e.kind == RK_FINAL) st_final = e.stage;
        if (e.kind == RK_LTREE) st_ltree = e.stage;
        if (e.kind == RK_MSMT) {   // the chunks come in stage order
            chunks_ok &= (u64)e.r == next && e.r % 64 == 0;
            next = (u64)e.r + e.items;
        }
    }
    CHECK(st_final == s.fin, "RK_FINAL is the last stage");
    if (c.range_mode && c.lane_tree) CHECK(st_ltree >= 0 && st_ltree < st_final, "lane trees before RK_FINAL");
    if (defer) {
        CHECK(st_ltree == L + 1 && st_ltree + 1 <= st_final, "a split batch's lane trees a tick before RK_FINAL");
        CHECK(chunks_ok && next == stage0_lanes(B, c.n, L, c.range_mode, S0_DEFER).total, "chunks partition S0_DEFER");
    } else {
        CHECK(next == 0, "RK_MSMT without defer");
    }
    const SortSets ss = lane_sort_sets(c, B, L);
    unsigned blk = 0;
    u64 tot = 0;
    CHECK(ss.count <= LANE_SORT_SETS && (B >= LANE_SORT_MIN || !ss.count), "sort sets");
    for (int k = 0; k < ss.count; k++) {
        CHECK(ss.set[k].block0 == blk && ss.set[k].items > 0, "sort set blocks");
        blk += (unsigned)((ss.set[k].items + LANE_SORT_BLOCK - 1) / LANE_SORT_BLOCK);
        tot += ss.set[k].items;
    }
    CHECK(ss.blocks == blk && ss.total == tot, "sort totals");
}

// A ring with every per-tick invariant checked: aligned disjoint regions, each schedule entry of each
// batch exactly once and in stage order, count <= MAX_REGIONS, total below 2^32.
struct Live { bool on = false; int ticks = 0; Schedule s; int seen[MAX_SCHED]; };
struct Checked {
    const PlanConfig& c;
    Ring R;
    std::vector<Live> live;
    u64 B = 0;             // the last batch pushed, for the failure messages
    int L = 0, defer = 0;
    int max_count = 0;     // the largest region list of any tick
    explicit Checked(const PlanConfig& cfg) : c(cfg), R(cfg), live(MAX_DEPTH) {}
    bool push(u64 Bn, int Ln, int dn) {   // stage a batch in slot head; false: the slot is busy
        B = Bn; L = Ln; defer = dn;
        if (!R.stage(B, L, defer != 0)) { CHECK(false, "slot busy when the ring comes round"); return false; }
        CHECK((R.slot[R.head].defer != 0) == (defer && L >= 2 && defer_ok(c)), "defer applies for L >= 2");
        Live& nw = live[R.head];
        nw.on = true;
        nw.ticks = 0;
        nw.s = batch_schedule(c, B, L, R.slot[R.head].defer);
        std::memset(nw.seen, 0, sizeof(nw.seen));
        return true;
    }
    PlanError tick() {   // plans, checks and advances (a tick that overflows the region list is not run)
        TickPlan tp;
        const PlanError pe = plan_tick(c, R.slot, R.D, R.head, tp);
        const RegionList& rl = tp.rl;
        CHECK(pe != PLAN_OVERFLOW && rl.count <= MAX_REGIONS, "region list overflow");
        if (pe == PLAN_OVERFLOW) return pe;
        if (rl.count > max_count) max_count = rl.count;
        CHECK((pe == PLAN_TOO_LARGE) == (rl.total >= (1ull << 32)), "2^32-lane error");
        CHECK(tp.ql == 1 || tp.ql == 2 || tp.ql == 4 || tp.ql == 16, "tick form");
        CHECK(rl.count > 0, "empty tick with batches in flight");
        u64 end = 0;
        for (int k = 0; k < rl.count; k++) {
            const Region& g = rl.reg[k];
            const u64 al = g.kind == RK_TREE ? 256 : 64;
            CHECK(g.begin == end && g.begin % al == 0 && g.items > 0, "regions ascending, aligned, disjoint");
            CHECK(g.kind != RK_TREE || k == 0, "RK_TREE only first");
            end = (g.begin + g.items + al - 1) & ~(al - 1);
            CHECK(g.slot >= 0 && g.slot < R.D && R.slot[g.slot].active, "region of an idle slot");
            if (g.slot < 0 || g.slot >= R.D || !live[g.slot].on) continue;
            const PlanSlot& sl = R.slot[g.slot];   // match the region to its batch's schedule entry
            const Schedule& s = live[g.slot].s;
            int hit = -1;
            for (int i = 0; i < s.count; i++)
                if (s.e[i].stage == sl.stage && s.e[i].kind == g.kind && s.e[i].r == g.r &&
                    s.e[i].items * (u64)region_lanes(g.kind, tp.ql) == g.items) hit = i;
            CHECK(hit >= 0, "region not in its batch's schedule at this stage");
            if (hit >= 0) live[g.slot].seen[hit]++;
        }
        CHECK(rl.total == end, "total = the last region's aligned end");
        bool was[MAX_DEPTH];
        for (int k = 0; k < R.D; k++) {
            was[k] = R.slot[k].active;
            if (was[k]) live[k].ticks++;
        }
        advance_ring(c, R.slot, R.D, R.head);
        for (int k = 0; k < R.D; k++) {
            if (!was[k] || R.slot[k].active) continue;   // retired with this tick
            const Schedule& s = live[k].s;
            CHECK(live[k].ticks == s.fin + 1, "retires after fin + 1 ticks");
            for (int i = 0; i < s.count; i++) CHECK(live[k].seen[i] == 1, "each region exactly once");
            live[k].on = false;
        }
        return pe;
    }
};

// one pipeline run: `pushes` batches (every other one with the pipeline's full L when `mixed`), then a drain
static void run_ring(const PlanConfig& c, u64 B, int L, int defer, int pushes, bool mixed) {
    Checked K(c);
    const int Lr = log2n(c.n);
    for (int t = 0; t < pushes || K.R.busy(); t++) {
        if (t < pushes && !K.push(B, (mixed && (t & 1)) ? Lr : L, defer)) return;
        K.B = B; K.L = L;
        if (K.tick() == PLAN_OVERFLOW) return;
        if (t > pushes + 4 * MAX_DEPTH) { CHECK(false, "drain does not end"); return; }
    }
}

// ---------------------------------------------------------------- free-form rings
// Every push has its own B, L and defer; B = 0 is a drain tick.  Pipeline::push's contract:
//   an accepted push is followed only by ticks that plan, whatever is accepted after it;
//   a refused push leaves the ring byte-identical and is accepted after at most D drain ticks;
//   push_admits refuses exactly the batches with which the ring, drained, would meet a tick that does
//   not plan (would_fail: this file's own statement of that), and never a uniform ring.
struct Op { u64 B; int L, defer; };
struct FreeStats { int refused = 0, max_count = 0; };
static bool would_fail(const Ring& R0, u64 B, int L, int split) {
    Ring R = R0;
    R.slot[R.head] = PlanSlot{true, 0, B, L, split};
    while (R.busy()) {
        TickPlan t;
        if (plan_tick(R.c, R.slot, R.D, R.head, t) != PLAN_OK) return true;
        advance_ring(R.c, R.slot, R.D, R.head);
    }
    return false;
}
static FreeStats run_free(const PlanConfig& c, const std::vector<Op>& ops) {
    Checked K(c);
    FreeStats st;
    g_cases++;
    for (const Op& op : ops) {
        const u64 B = op.B;
        const int L = op.L, defer = op.defer;
        if (B) {
            const int split = (defer && batch_defers(c, L)) ? 1 : 0;
            for (int waited = 0;; waited++) {
                CHECK(!K.R.slot[K.R.head].active, "slot busy when the ring comes round");
                if (K.R.slot[K.R.head].active) return st;
                bool uniform = true;
                for (int k = 0; k < K.R.D; k++)
                    uniform &= !K.R.slot[k].active || (K.R.slot[k].L == L && K.R.slot[k].defer == split);
                Ring before = K.R;
                const PlanError adm = push_admits(c, K.R.slot, K.R.D, K.R.head, B, L, split);
                CHECK(!std::memcmp(before.slot, K.R.slot, sizeof(before.slot)) && before.head == K.R.head,
                      "admission leaves the ring byte-identical");
                CHECK((adm != PLAN_OK) == would_fail(K.R, B, L, split), "refused exactly when a later tick would not plan");
                if (adm == PLAN_OK) break;
                if (!waited) st.refused++;
                CHECK(!uniform, "a uniform ring is never refused");
                CHECK(waited < K.R.D, "a refused push is accepted after at most D drain ticks");
                if (waited >= K.R.D) return st;
                CHECK(K.tick() == PLAN_OK, "a drain tick after a refusal plans");
            }
            if (!K.push(B, L, defer)) return st;
        }
        K.B = B; K.L = L; K.defer = defer;
        if (K.R.busy()) CHECK(K.tick() == PLAN_OK, "an accepted push is followed only by ticks that plan");
    }
    for (int t = 0; K.R.busy(); t++) {
        const u64 B = K.B;
        const int L = K.L, defer = K.defer;
        CHECK(K.tick() == PLAN_OK, "the drain plans");
        if (t > 2 * MAX_DEPTH) { CHECK(false, "drain does not end"); break; }
    }
    st.max_count = K.max_count;
    return st;
}

// the round counts log2 n, log2 n - 1, .. 2, one per push (every batch's final-terms stage in one
// tick), then three full-L batches
static FreeStats descending(int n, int mode, bool raised, int defer) {
    PlanConfig c;
    c.n = n; c.range_mode = mode; c.lane_tree = raised || n <= LANE_TREE_MAX;
    c.row_max = 2048; c.quad_max = 16384; c.pair_max = 32768;
    std::vector<Op> ops;
    for (int L = log2n(n); L >= 2; L--) ops.push_back(Op{2, L, defer});
    for (int k = 0; k < 3; k++) ops.push_back(Op{2, log2n(n), defer});
    return run_free(c, ops);
}
static void check_refusal_table() {
    struct Row { int n, mode; bool raised; int defer; bool refused; };
    static const Row rows[] = {
        // the default configuration
        {1024, 2, false, 0, false}, {2048, 2, false, 0, true}, {4096, 2, false, 0, true},
        {65536, 2, false, 0, true},  {65536, 0, false, 0, false}, {65536, 1, false, 0, false},
        // the lane-tree limit raised (HIPBP_LANE_TREE_MAX), split stage 0
        {64, 1, true, 1, false},  {64, 2, true, 1, false}, {128, 2, true, 1, false},
        {256, 1, true, 1, false}, {256, 2, true, 1, true},  {512, 1, true, 1, false},
        {512, 2, true, 1, true},
    };
    g_what = "refusal table";
    for (const Row& w : rows) {
        const FreeStats st = descending(w.n, w.mode, w.raised, w.defer);
        PlanConfig c;
        c.n = w.n; c.range_mode = w.mode; c.lane_tree = w.raised;
        const u64 B = 2;
        const int L = 0, defer = w.defer;
        CHECK((st.refused > 0) == w.refused, "descending round counts: refused where the region list would overflow");
        CHECK(st.max_count <= MAX_REGIONS, "descending round counts: the largest tick");
        std::printf("descending n %d mode %d raised %d defer %d: refused %d max %d\n", w.n, w.mode, (int)w.raised,
                    w.defer, st.refused, st.max_count);
    }
}

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned m) {   // xorshift64*, seeded per configuration
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (unsigned)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % m;
}
static void free_form(int random_per_cfg) {
    static const u64 Bs[] = {1, 3, 63, 64, 65, 1000};
    for (int n : {4, 16, 64, 256, 512, 2048, 65536})
        for (int mode = 0; mode <= 2; mode++)
            for (int lane_tree = 0; lane_tree <= 1; lane_tree++) {
                PlanConfig c;
                c.n = n; c.range_mode = mode; c.lane_tree = lane_tree != 0;
                c.row_max = 2048; c.quad_max = 16384; c.pair_max = 32768;
                const int ln = log2n(n), D = pipeline_depth(c);
                g_what = "structured";
                for (int dsel = 0; dsel < 3; dsel++)       // split stage 0: never, always, every other push
                    for (u64 B : Bs) {
                        auto df = [dsel](int k) { return dsel == 2 ? (k & 1) : dsel; };
                        std::vector<Op> desc, asc, saw, con;
                        for (int k = 0; k < 2 * D + 3; k++) {
                            desc.push_back(Op{B, ln - k % (ln + 1), df(k)});
                            asc.push_back(Op{B, k % (ln + 1), df(k)});
                            saw.push_back(Op{B, (k & 1) ? ln : k / 2 % (ln + 1), df(k)});
                        }
                        run_free(c, desc);
                        run_free(c, asc);
                        run_free(c, saw);
                        for (int L = 0; L <= ln; L++) {   // constant L (a uniform ring unless dsel = 2), drain ticks mixed in
                            con.clear();
                            for (int k = 0; k < 2 * D + 3; k++) con.push_back(Op{k % 5 == 3 ? 0 : B + (u64)k, L, df(k)});
                            const FreeStats st = run_free(c, con);
                            const int defer = dsel;
                            if (dsel < 2) CHECK(st.refused == 0, "a uniform ring is never refused");
                        }
                    }
                g_what = "random";
                g_rng = 0x9E3779B97F4A7C15ull ^ ((u64)n << 20) ^ (u64)(mode * 2 + lane_tree);
                for (int it = 0; it < random_per_cfg; it++) {
                    std::vector<Op> ops;
                    const int len = D + 4 + (int)rnd(D + 4);
                    const int style = (int)rnd(3);   // any L; mostly two neighbouring values; a downward drift
                    int Lw = (int)rnd(ln + 1);
                    for (int k = 0; k < len; k++) {
                        if (rnd(6) == 0) { ops.push_back(Op{0, 0, 0}); continue; }
                        int L = (int)rnd(ln + 1);
                        if (style == 1) L = Lw - (int)rnd(2);
                        if (style == 2) { L = Lw; Lw = Lw > 0 && rnd(4) ? Lw - 1 : (int)rnd(ln + 1); }
                        if (L < 0) L = 0;
                        ops.push_back(Op{Bs[rnd(6)], L, (int)rnd(2)});
                    }
                    run_free(c, ops);
                }
            }
    // a uniform ring at every n and mode, both tree forms, drain ticks mixed in
    g_what = "uniform";
    for (int ln = 0; ln <= 16; ln++)
        for (int mode = 0; mode <= 2; mode++)
            for (int lane_tree = 0; lane_tree <= 1; lane_tree++) {
                PlanConfig c;
                c.n = 1 << ln; c.range_mode = mode; c.lane_tree = lane_tree != 0;
                c.row_max = 2048; c.quad_max = 16384; c.pair_max = 32768;
                const int D = pipeline_depth(c);
                for (int L = 0; L <= ln; L++)
                    for (int defer = 0; defer <= 1; defer++) {
                        std::vector<Op> ops;
                        for (int k = 0; k < 2 * D + 3; k++) ops.push_back(Op{k % 7 == 5 ? 0 : Bs[k % 6], L, defer});
                        const u64 B = 0;
                        CHECK(run_free(c, ops).refused == 0, "a uniform ring is never refused");
                    }
            }
}

static void check_depth(const PlanConfig& c) {
    const u64 B = 1000;
    const int L = log2n(c.n), defer = 0;
    const int D = pipeline_depth(c);
    CHECK(D == batch_schedule(c, B, L, 0).fin + 1 && D <= MAX_DEPTH, "D = fin + 1 of the full-L batch");
    if (defer_ok(c)) CHECK(D == batch_schedule(c, B, L, 1).fin + 1, "D = fin + 1 of the split full-L batch");
}

static int sweep(int random_per_cfg) {
    for (int ln = 0; ln <= 16; ln++)
        for (int mode = 0; mode <= 2; mode++)
            for (int lane_tree = 0; lane_tree <= 1; lane_tree++) {
                PlanConfig c;
                c.n = 1 << ln; c.range_mode = mode; c.lane_tree = lane_tree != 0;
                c.row_max = 2048; c.quad_max = 16384; c.pair_max = 32768;
                g_what = "depth";
                check_depth(c);
                const int D = pipeline_depth(c);
                for (int L = 0; L <= ln; L++)
                    for (int defer = 0; defer <= (defer_ok(c) ? 1 : 0); defer++)
                        for (u64 B : {1ull, 63ull, 64ull, 1000ull}) {
                            g_cases++;
                            g_what = "schedule";
                            const int split = defer && batch_defers(c, L);
                            check_schedule(c, B, L, split);
                            CHECK(batch_schedule(c, B, L, split).fin < D, "a batch retires before the ring comes round");
                            g_what = "full ring";
                            run_ring(c, B, L, defer, 2 * D + 3, false);
                            g_what = "mixed ring";
                            run_ring(c, B, L, defer, 2 * D + 3, true);
                            g_what = "drain";
                            run_ring(c, B, L, defer, 1, false);
                        }
            }
    const int fixed = g_cases;
    check_refusal_table();
    free_form(random_per_cfg);
    std::printf("free-form rings %d\n", g_cases - fixed);
    std::printf("%d %d\n", g_cases, g_fails);
    return g_fails ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "replay")) return replay();
    if (argc >= 2 && !std::strcmp(argv[1], "sweep")) return sweep(argc > 2 ? std::atoi(argv[2]) : 2000);
    std::fprintf(stderr, "usage: %s replay < ops | sweep [random sequences per configuration]\n", argv[0]);
    return 2;
}

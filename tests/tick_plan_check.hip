// tick_plan_check.hip — TEST INFRASTRUCTURE (tests/test_tick_plan.py).
//
// Runs the verify pipeline's tick planner (cudabulletproof_amd/csrc/bp_tick_plan.h, host-only) on
// the CPU, driving the ring exactly as Pipeline::push does (stage a batch in slot `head`, plan the
// tick, advance the ring).
//   replay: reads "cfg n mode lane_tree quad_force row_max quad_max pair_max sort_mask", then
//           "push B L defer" / "flush" lines from stdin and prints "depth D", then for every push a
//           "sort blocks count (kind r items block0)*" line and for every tick a
//           "tick ql count total (kind slot r begin items)*" line: the rows of tests/golden/tick_plans.json.
//   sweep:  the planner's invariants over the whole parameter space; prints "<cases> <failures>",
//           exit status 1 on any failure.
#include <cstdio>
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
        u64 B;
        int L, defer;
        if (std::strcmp(op, "push") || std::scanf(" %llu %d %d", &B, &L, &defer) != 3) return 2;
        if (!R.stage(B, L, defer != 0)) { std::printf("error busy\n"); return 1; }
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

// one pipeline run: `pushes` batches (every other one with the pipeline's full L when `mixed`), then a drain
static void run_ring(const PlanConfig& c, u64 B, int L, int defer, int pushes, bool mixed) {
    Ring R(c);
    const int Lr = log2n(c.n);
    struct Live { bool on = false; int ticks = 0; Schedule s; int seen[MAX_SCHED]; };
    std::vector<Live> live(MAX_DEPTH);
    for (int t = 0; t < pushes || R.busy(); t++) {
        if (t < pushes) {
            const int Lb = (mixed && (t & 1)) ? Lr : L;
            if (!R.stage(B, Lb, defer != 0)) { CHECK(false, "slot busy when the ring comes round"); return; }
            CHECK((R.slot[R.head].defer != 0) == (defer && Lb >= 2), "defer applies for L >= 2");
            Live& nw = live[R.head];
            nw.on = true;
            nw.ticks = 0;
            nw.s = batch_schedule(c, B, Lb, R.slot[R.head].defer);
            std::memset(nw.seen, 0, sizeof(nw.seen));
        }
        TickPlan tp;
        const PlanError pe = plan_tick(c, R.slot, R.D, R.head, tp);
        const RegionList& rl = tp.rl;
        CHECK(pe != PLAN_OVERFLOW && rl.count <= MAX_REGIONS, "region list overflow");
        if (pe == PLAN_OVERFLOW) return;
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
        if (t > pushes + 4 * MAX_DEPTH) { CHECK(false, "drain does not end"); return; }
    }
}

static void check_depth(const PlanConfig& c) {
    const u64 B = 1000;
    const int L = log2n(c.n), defer = 0;
    const int D = pipeline_depth(c);
    CHECK(D == batch_schedule(c, B, L, 0).fin + 1 && D <= MAX_DEPTH, "D = fin + 1 of the full-L batch");
    if (defer_ok(c)) CHECK(D == batch_schedule(c, B, L, 1).fin + 1, "D = fin + 1 of the split full-L batch");
}

static int sweep() {
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
    std::printf("%d %d\n", g_cases, g_fails);
    return g_fails ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "replay")) return replay();
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    std::fprintf(stderr, "usage: %s replay < ops | sweep\n", argv[0]);
    return 2;
}

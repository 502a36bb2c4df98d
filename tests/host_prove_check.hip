// host_prove_check.hip — TEST INFRASTRUCTURE (tests/test_host_prove_plan.py).
//
// Runs the host provers' plan and result owner (cudabulletproof_amd/csrc/bp_host_prove.h, host-only)
// on the CPU.
//   plan:   over count x ng x chunk x index_base the shards are contiguous, disjoint, cover [0, count),
//           differ in size by at most one, none empty when ng <= count; every shard's chunks cover it
//           in order and carry index_base + c0 mod 2^64 (restated here with 128-bit arithmetic); the
//           wrap past 2^64 is reached
//   count:  the shard count over num_gpus x ndev x HIPBP_HOST_SHARDS's value x count against its rule
//           restated here: the two errors with their codes and messages, the override only at
//           num_gpus <= 0, capped at 64 and at one shard per proof
//   fanout: host lambdas as shards: every callback once and returned before the fan-out returns, the
//           caller's thread only for a single shard with d = 0; shard k failing is the one reported,
//           with its own message; of two own failures among shards stopped for the flag, the first
//           in shard order, whichever came first in time
//   owner:  9 proofs (L_len 0 and 4, one refused value, with and without attempts) filled from three
//           threads through a counting allocator, then rolled back: no vector left, every output byte
//           zero; the same with the k-th allocation failing, for every k up to the total
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_host_prove.h"

typedef unsigned long long u64;
static std::atomic<u64> checks(0), fails(0);
#define CHECK(cond, ...)                                    \
    do {                                                    \
        checks++;                                           \
        if (!(cond)) {                                      \
            if (fails++ < 20) {                             \
                std::printf("FAIL line %d: ", __LINE__);    \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

static bool all_zero(const void* p, size_t len) {
    for (size_t i = 0; i < len; i++) if (((const uint8_t*)p)[i]) return false;
    return true;
}

// ------------------------------------------------------------------ plan
static void plan() {
    const size_t counts[] = {1, 2, 3, 9, 70, 65537}, chunks[] = {1, 4, 16384};
    const int ngs[] = {1, 2, 3, 8, 64};
    const uint64_t bases[] = {0, (uint64_t(1) << 32) - 3, ~uint64_t(0) - 1};   // 0, 2^32 - 3, 2^64 - 2
    u64 wraps = 0, multi_chunk = 0, short_last = 0;
    for (size_t count : counts)
        for (int ng : ngs)
            for (size_t chunk : chunks)
                for (uint64_t base : bases) {
                    const std::vector<bp::HostShard> sh = bp::plan_host_shards(count, ng);
                    CHECK(!sh.empty() && sh.front().lo == 0 && sh.back().hi == count, "cover count=%zu ng=%d", count, ng);
                    CHECK(sh.size() == std::min<size_t>(count, (size_t)ng), "shards %zu count=%zu ng=%d", sh.size(), count, ng);
                    size_t smin = count, smax = 0;
                    for (size_t k = 0; k < sh.size(); k++) {
                        const size_t sz = sh[k].hi - sh[k].lo;
                        CHECK(sh[k].hi > sh[k].lo, "empty shard listed");
                        CHECK(sh[k].d >= 0 && sh[k].d < ng && (k == 0 || sh[k].d > sh[k - 1].d), "shard ids");
                        CHECK(k == 0 || sh[k].lo == sh[k - 1].hi, "shards not contiguous");
                        CHECK(sh[k].lo == count * (size_t)sh[k].d / ng && sh[k].hi == count * (size_t)(sh[k].d + 1) / ng,
                              "block bounds");
                        smin = std::min(smin, sz);
                        smax = std::max(smax, sz);
                        // the shard's chunks, cut as the library cuts them
                        const size_t ch = std::min(chunk, sz);
                        const std::vector<bp::HostChunk> cs = bp::plan_host_chunks(sh[k], ch, base);
                        CHECK(cs.size() == (sz + ch - 1) / ch, "chunk count");
                        size_t at = sh[k].lo;
                        for (size_t q = 0; q < cs.size(); q++) {
                            CHECK(cs[q].c0 == at, "chunk %zu starts at %zu, want %zu", q, cs[q].c0, at);
                            CHECK(cs[q].c >= 1 && cs[q].c <= ch && (cs[q].c == ch || q + 1 == cs.size()), "chunk size");
                            const uint64_t want = (uint64_t)((unsigned __int128)base + (unsigned __int128)cs[q].c0);
                            CHECK(cs[q].index_base == want, "chunk base");
                            if (cs[q].index_base < base) wraps++;
                            if (cs[q].c < ch) short_last++;
                            at += cs[q].c;
                        }
                        CHECK(at == sh[k].hi, "chunks end at %zu, want %zu", at, sh[k].hi);
                        if (cs.size() > 1) multi_chunk++;
                    }
                    CHECK(smax - smin <= 1, "sizes differ by %zu", smax - smin);
                    if ((size_t)ng <= count) CHECK(sh.size() == (size_t)ng && smin >= 1, "an empty shard at ng <= count");
                }
    CHECK(wraps > 0, "the wrap past 2^64 was never reached");
    CHECK(multi_chunk > 0 && short_last > 0, "the grid has no shard of several chunks / no short last chunk");
}

// ------------------------------------------------------------------ shard count
static void shard_count() {
    const char* envs[] = {nullptr, "0", "-3", "1", "3", "64", "65", "abc"};
    const long env_val[] = {0, 0, -3, 1, 3, 64, 65, 0};   // what each asks for (0: nothing)
    const int ndevs[] = {0, 1, 2, 8};
    const size_t counts[] = {1, 2, 70};
    u64 overrides = 0, ignored = 0;
    for (int ndev : ndevs)
        for (int num_gpus : {-1, 0, 1, 2, ndev, ndev + 1})
            for (size_t e = 0; e < 8; e++)
                for (size_t count : counts) {
                    int ng = -7;
                    std::string err = "untouched";
                    const int rc = bp::resolve_host_shards(num_gpus, ndev, envs[e], count, &ng, &err);
                    if (ndev == 0) {
                        CHECK(rc == 2 && err == "no HIP device" && ng == -7, "ndev = 0: rc %d '%s'", rc, err.c_str());
                        continue;
                    }
                    if (num_gpus > ndev) {
                        char want[96];
                        std::snprintf(want, sizeof want, "num_gpus = %d but %d HIP device(s) visible", num_gpus, ndev);
                        CHECK(rc == 1 && err == want && ng == -7, "num_gpus %d ndev %d: rc %d '%s'", num_gpus, ndev, rc, err.c_str());
                        continue;
                    }
                    long want = num_gpus >= 1 ? num_gpus : ndev;
                    if (num_gpus < 1 && env_val[e] >= 1) {
                        want = env_val[e] > 64 ? 64 : env_val[e];
                        if ((size_t)want > count) want = (long)count;
                        overrides++;
                    }
                    if (num_gpus >= 1 && env_val[e] >= 1 && env_val[e] != num_gpus) ignored++;
                    CHECK(rc == 0 && ng == want, "num_gpus %d ndev %d env %s count %zu: rc %d ng %d, want %ld", num_gpus, ndev,
                          envs[e] ? envs[e] : "(null)", count, rc, ng, want);
                    CHECK(err == "untouched", "a message without an error");
                }
    CHECK(overrides > 0 && ignored > 0, "the grid never reached the override / never had one to ignore");
}

// ------------------------------------------------------------------ fan-out
static std::vector<bp::HostShard> unit_shards(int ns) { return bp::plan_host_shards((size_t)ns, ns); }   // d = 0 .. ns - 1

// a shard's wait for the flag (bounded: a flag that is never raised fails the check, it does not hang it)
static bool wait_raised(const bp::HostStop& stop) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(60);
    while (!stop.raised() && std::chrono::steady_clock::now() < until) std::this_thread::yield();
    return stop.raised();
}

static void fanout() {
    const std::thread::id me = std::this_thread::get_id();
    // every shard succeeds: each callback once, on the caller's thread only for one shard with d = 0
    std::vector<std::vector<bp::HostShard>> plans;
    for (int ns : {1, 2, 3, 8}) plans.push_back(unit_shards(ns));
    plans.push_back({bp::HostShard{2, 0, 5}});   // one shard, not the caller's device
    for (const auto& shards : plans) {
        const size_t ns = shards.size();
        std::vector<std::atomic<int>> ran(64);
        std::vector<std::thread::id> tid(64);
        std::atomic<size_t> exits(0);
        const bp::HostFanFailure f = bp::host_fanout(shards, [&](const bp::HostShard& sh, const bp::HostStop& stop, std::string&) {
            ran[sh.d]++;
            tid[sh.d] = std::this_thread::get_id();
            const int rc = stop.raised() ? 9 : 0;
            exits++;
            return rc;
        });
        CHECK(f.k == ns && f.rc == 0 && f.err.empty(), "success reported as a failure of shard %zu", f.k);
        CHECK(exits == ns, "%zu of %zu callbacks had returned", (size_t)exits, ns);
        const bool inline_run = ns == 1 && shards[0].d == 0;
        for (const bp::HostShard& sh : shards) {
            CHECK(ran[sh.d] == 1, "shard %d ran %d times", sh.d, (int)ran[sh.d]);
            CHECK((tid[sh.d] == me) == inline_run, "shard %d of %zu on the wrong thread", sh.d, ns);
        }
    }
    // shard k fails, the others succeed
    for (int ns : {1, 2, 3, 8})
        for (int k = 0; k < ns; k++) {
            std::atomic<int> exits(0);
            const bp::HostFanFailure f =
                bp::host_fanout(unit_shards(ns), [&](const bp::HostShard& sh, const bp::HostStop&, std::string& err) {
                    err = "shard " + std::to_string(sh.d) + (sh.d == k ? " failed" : " left a stale message");
                    exits++;
                    return sh.d == k ? 40 + k : 0;
                });
            CHECK(f.k == (size_t)k && f.rc == 40 + k && f.err == "shard " + std::to_string(k) + " failed",
                  "ns %d, shard %d failing: reported %zu rc %d '%s'", ns, k, f.k, f.rc, f.err.c_str());
            CHECK(exits == ns, "%d of %d callbacks had returned", (int)exits, ns);
        }
    // shards 1 and 3 of 5 fail on their own, one at once and the other only after the flag is up; 2 and
    // 4 (and 0, or not) stop for the flag: shard 1 is reported, whichever failed first
    for (int first : {1, 3})
        for (bool zero_stops : {false, true}) {
            std::atomic<int> exits(0), stopped(0);
            const bp::HostFanFailure f =
                bp::host_fanout(unit_shards(5), [&](const bp::HostShard& sh, const bp::HostStop& stop, std::string& err) {
                    int rc = 0;
                    if (sh.d == 1 || sh.d == 3) {
                        rc = sh.d != first && !wait_raised(stop) ? 99 : 50 + sh.d;
                        err = "own " + std::to_string(sh.d);
                    } else if (sh.d != 0 || zero_stops) {
                        rc = wait_raised(stop) ? bp::HOST_SHARD_STOPPED : 99;
                        err = "stopped";
                        stopped++;
                    }
                    exits++;
                    return rc;
                });
            CHECK(f.k == 1 && f.rc == 51 && f.err == "own 1", "first %d, shard 0 %s: reported %zu rc %d '%s'", first,
                  zero_stops ? "stops" : "succeeds", f.k, f.rc, f.err.c_str());
            CHECK(exits == 5 && stopped == (zero_stops ? 3 : 2), "%d callbacks had returned, %d stopped", (int)exits, (int)stopped);
        }
}

// ------------------------------------------------------------------ owner
// the allocator handed to the owner: counts, fails the fail_at-th call, tracks what is live
static std::mutex g_mu;
static std::set<void*> g_live;
static std::atomic<long> g_calls(0);
static long g_fail_at = 0;   // 0: never
static void* t_alloc(size_t bytes) {
    const long k = ++g_calls;
    if (k == g_fail_at) return nullptr;
    void* p = malloc(bytes);
    std::lock_guard<std::mutex> lk(g_mu);
    g_live.insert(p);
    return p;
}
static void t_release(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        CHECK(g_live.erase(p) == 1, "released a pointer the allocator did not hand out (or twice)");
    }
    free(p);
}

static void pattern(void* p, size_t len, u64 seed) {
    uint8_t* q = (uint8_t*)p;
    for (size_t i = 0; i < len; i++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        q[i] = (uint8_t)(seed >> 56) | 1;   // never zero
    }
}

// B proofs of Lr rounds, proof `refused` refused, as the host copy of a chunk's output; filled by
// three threads (blocks of the plan), with the fail_at-th allocation failing (0: none)
static void owner_case(size_t Lr, bool with_attempts, long fail_at) {
    const size_t B = 9, refused = 5, n = size_t(1) << Lr;
    const bp::OutLayout lay{B, B, Lr, 64};
    std::vector<uint8_t> host(lay.slot_bytes());
    pattern(host.data(), host.size(), 77 + Lr);
    hipbp_proof_out o;
    lay.view(host.data(), &o);
    for (size_t k = 0; k < B; k++) o.valid[k] = k != refused;
    std::vector<RangeProof> proofs(B);
    std::vector<uint8_t> valid(B), attempts(B);
    pattern(proofs.data(), B * sizeof(RangeProof), 5);   // the owner zeroes what it is given
    pattern(valid.data(), B, 6);
    pattern(attempts.data(), B, 7);
    g_calls = 0;
    g_fail_at = fail_at;
    bp::ProofOwner own(proofs.data(), valid.data(), with_attempts ? attempts.data() : nullptr, B,
                       bp::HostAlloc{t_alloc, t_release});
    CHECK(all_zero(proofs.data(), B * sizeof(RangeProof)) && all_zero(valid.data(), B), "outputs not zeroed at the start");
    CHECK(!with_attempts || all_zero(attempts.data(), B), "attempts not zeroed at the start");
    std::atomic<int> failed(0);
    std::vector<std::thread> th;
    for (const bp::HostShard& sh : bp::plan_host_shards(B, 3))
        th.emplace_back([&, sh]() {
            for (size_t i = sh.lo; i < sh.hi; i++)
                if (!own.fill(i, lay, host.data(), i, n, (uint8_t)(i == refused ? 0 : i % 3 + 1))) {   // a shard stops at its first failure
                    failed++;
                    return;
                }
        });
    for (auto& t : th) t.join();
    const long total = 4 * (long)(B - 1);
    if (fail_at == 0 || fail_at > total) {
        CHECK(failed == 0 && g_calls == total, "allocations %ld, want %ld", (long)g_calls, total);
        CHECK(g_live.size() == (size_t)total, "live vectors %zu", g_live.size());
        for (size_t i = 0; i < B; i++) {
            const RangeProof& p = proofs[i];
            const InnerProductProof& ip = p.ip_proof;
            CHECK(!memcmp(&p.V, &o.V[i], 128) && !memcmp(&p.T2, &o.T2[i], 128) && !memcmp(&p.mu, &o.mu[i], 32), "head %zu", i);
            CHECK(valid[i] == (i != refused), "valid %zu", i);
            if (with_attempts) CHECK(attempts[i] == (i == refused ? 0 : i % 3 + 1), "attempts %zu", i);
            if (i == refused) {
                CHECK(all_zero(&ip, sizeof ip), "refused proof's ip_proof not zero");
                continue;
            }
            CHECK(ip.n == n && ip.L_len == Lr && ip.a.length == 1 && ip.b.length == 1 && ip.L.length == Lr && ip.R.length == Lr,
                  "lengths %zu", i);
            CHECK(!memcmp(ip.a.elements, &o.a[i], 32) && !memcmp(ip.b.elements, &o.b[i], 32) && !memcmp(&ip.x, &o.x[i], 32),
                  "a, b, x %zu", i);
            if (Lr) CHECK(!memcmp(ip.L.elements, o.L + i * Lr, Lr * 128) && !memcmp(ip.R.elements, o.R + i * Lr, Lr * 128), "L, R %zu", i);
        }
    } else {
        CHECK(failed >= 1, "allocation %ld failed but no fill reported it", fail_at);
    }
    own.rollback();
    CHECK(g_live.empty(), "%zu vectors left after the rollback", g_live.size());
    CHECK(all_zero(proofs.data(), B * sizeof(RangeProof)), "a struct byte is not zero after the rollback");
    CHECK(all_zero(valid.data(), B), "a valid byte is not zero after the rollback");
    if (with_attempts) CHECK(all_zero(attempts.data(), B), "an attempts byte is not zero after the rollback");
    else {   // the seeded prover has no attempts: the owner never touches a buffer it was not given
        std::vector<uint8_t> want(B);
        pattern(want.data(), B, 7);
        CHECK(attempts == want, "attempts written without being given");
    }
    own.rollback();   // a second rollback finds nothing to free
    CHECK(g_live.empty(), "second rollback");
}

int main() {
    plan();
    shard_count();
    fanout();
    for (size_t Lr : {size_t(0), size_t(4)})
        for (bool att : {false, true})
            for (long k = 0; k <= 4 * 8 + 1; k++) owner_case(Lr, att, k);
    std::printf("%llu %llu\n", (u64)checks, (u64)fails);
    return fails ? 1 : 0;
}

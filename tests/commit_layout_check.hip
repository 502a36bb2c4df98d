// commit_layout_check.hip — TEST INFRASTRUCTURE (tests/test_commit_cpu.py).
//
// Runs the host-only parts of the batched Pedersen commitments on the CPU: the commit workspace's
// table and chunking rule (cudabulletproof_amd/csrc/bp_layout.h) and k_commit_terms' lane layout
// (bp_kernels.h).  The expectations are restated here as plain formulas (128-byte points).
//   table:  the terms buffer holds two points per commitment of a chunk
//   sort:   HIPBP_COMMIT_SORT's rule
//   chunk:  HIPBP_COMMIT_CHUNK's default, clamp and "never more than count"; the chunks of a call
//           cover [0, count) in order, each at most the workspace's size
//   lanes:  over a sweep of counts every commitment has exactly one blinding lane and one value lane,
//           no aligned 64 lanes mix the classes, the blinding class comes first, padding lanes map to
//           no item, and the launch's 256-lane blocks cover both classes
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_layout.h"

typedef unsigned long long u64;
static u64 checks = 0, fails = 0;
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

int main() {
    using namespace bp;
    // table
    for (size_t c : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)130, (size_t)1 << 20, (size_t)1 << 24}) {
        size_t sz[CB_COUNT];
        commit_sizes(c, false, sz);
        CHECK(CB_COUNT == 3 && sz[CB_TERMS] == c * 256, "terms of %zu: %zu bytes", c, sz[CB_TERMS]);
        CHECK(sz[CB_ORDER] == 0 && sz[CB_BINS] == 0, "unsorted call of %zu: sort buffers", c);
        commit_sizes(c, true, sz);
        CHECK(sz[CB_TERMS] == c * 256 && sz[CB_ORDER] == c * 8 && sz[CB_BINS] == 2 * 513 * 4,
              "sorted call of %zu: %zu %zu %zu", c, sz[CB_TERMS], sz[CB_ORDER], sz[CB_BINS]);
    }
    {
        size_t sz[CB_COUNT];
        commit_sizes((size_t)1 << 20, false, sz);
        CHECK(sz[CB_TERMS] == (size_t)256 << 20, "default chunk: 256 MB of terms, got %zu", sz[CB_TERMS]);
    }
    // chunk
    CHECK(commit_chunk(5, 0) == 5 && commit_chunk(5, -3) == 5, "unset: count below the default");
    CHECK(commit_chunk((size_t)3 << 20, 0) == (size_t)1 << 20, "unset: the default");
    CHECK(commit_chunk(130, 64) == 64 && commit_chunk(64, 64) == 64 && commit_chunk(63, 64) == 63, "env 64");
    CHECK(commit_chunk((size_t)1 << 30, 1ll << 40) == (size_t)1 << 24, "clamp");
    for (size_t count : {(size_t)1, (size_t)64, (size_t)130, (size_t)1000, ((size_t)5 << 20) + 7})
        for (long long env : {0ll, 1ll, 64ll, 100ll, 1ll << 21}) {
            const size_t ch = commit_chunk(count, env);
            size_t next = 0, n = 0;
            for (size_t c0 = 0; c0 < count && n < 200; c0 += ch, n++) {   // commit_run's loop (bp_api_prove.hip)
                const size_t c = count - c0 < ch ? count - c0 : ch;
                CHECK(c0 == next && c >= 1 && c <= ch, "chunk at %zu of %zu", c0, count);
                next = c0 + c;
            }
            CHECK(n == 200 || next == count, "chunks of %zu end at %zu", count, next);
        }
    // the sort's rule
    CHECK(!commit_sorted(4095, nullptr) && commit_sorted(4096, nullptr), "unset: from 4096 on");
    CHECK(commit_sorted(1, "1") && !commit_sorted((size_t)1 << 20, "0"), "switch");
    // lanes
    for (size_t count : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)127, (size_t)128,
                         (size_t)130, (size_t)255, (size_t)256, (size_t)257, (size_t)1000}) {
        const size_t P = commit_class_lanes(count);
        CHECK(P % 64 == 0 && P >= count && P < count + 64, "class lanes of %zu: %zu", count, P);
        const size_t blocks = (2 * P + 255) / 256, lanes = blocks * 256;
        std::vector<int> seen[2] = {std::vector<int>(count, 0), std::vector<int>(count, 0)};
        for (size_t w = 0; w < lanes / 64; w++) {
            bool wave_val = false;
            for (size_t l = 0; l < 64; l++) {
                bool val;
                const size_t lane = w * 64 + l, j = commit_lane_item(count, lane, val);
                if (l == 0) wave_val = val;
                CHECK(val == wave_val, "count %zu wave %zu mixes the classes", count, w);
                CHECK(val == (lane >= P), "count %zu lane %zu: class", count, lane);
                if (j == SIZE_MAX) {
                    CHECK((val ? lane - P : lane) >= count, "count %zu lane %zu: live lane unmapped", count, lane);
                    continue;
                }
                CHECK(j < count && j == (val ? lane - P : lane), "count %zu lane %zu -> %zu", count, lane, j);
                if (j < count) seen[val ? 1 : 0][j]++;
            }
        }
        for (size_t j = 0; j < count; j++)
            CHECK(seen[0][j] == 1 && seen[1][j] == 1, "count %zu item %zu: %d blinding, %d value lanes", count, j,
                  seen[0][j], seen[1][j]);
    }
    std::printf("%llu %llu\n", checks, fails);
    return fails ? 1 : 0;
}

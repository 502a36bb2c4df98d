// gens_derive_check.hip — TEST INFRASTRUCTURE (tests/test_gens_derive_cpu.py).
//
// Runs the two lane bodies of cudabulletproof_amd/csrc/bp_gens_derive.h (what the kernels of
// bp_gens_derive.hip and the _host entry points call) in CPU loops against a byte-at-a-time SHA-256
// written here and the header's host fe_mul.  Built --cuda-host-only, once plain and once under
// ASan + UBSan; a stand-alone program.
//   vector:  seeds all-zero, all-0xFF, 01 00.., and random ones, each read from an allocation of exactly
//            32 bytes; indices 0..70, around every byte carry of the big-endian index (255|256,
//            65535|65536, 2^24-1|2^24), the last five below 2^32: X, Y bytes, Z = 1, T = X * Y
//   single:  the same seeds: X bytes, Y = Z = 1, T = X * 1; T != X for 01 00.. (bit 255 of X is set)
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_gens_derive.h"

typedef unsigned long long u64;
typedef std::vector<uint8_t> Bytes;
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

static u64 g_state = 0x243F6A8885A308D3ull;
static u64 rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    u64 x = g_state;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 29;
    return x;
}

// ------------------------------------------------------------------ SHA-256, a byte at a time (FIPS 180-4)
struct RefSha {
    uint32_t h[8];
    uint8_t buf[64];
    size_t fill = 0;
    u64 total = 0;
    RefSha() {
        const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        memcpy(h, iv, sizeof(h));
    }
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block() {
        static const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
            0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
            0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
            0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
            0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
            0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
            0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
            0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)buf[4 * i] << 24 | (uint32_t)buf[4 * i + 1] << 16 | (uint32_t)buf[4 * i + 2] << 8 | buf[4 * i + 3];
        for (int i = 16; i < 64; i++)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
                   (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void byte(uint8_t v) {
        buf[fill++] = v;
        total++;
        if (fill == 64) { block(); fill = 0; }
    }
    Bytes done() {
        const u64 bits = total * 8;
        byte(0x80);
        while (fill != 56) byte(0);
        for (int k = 7; k >= 0; k--) byte((uint8_t)(bits >> (8 * k)));
        Bytes out(32);
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
        return out;
    }
};
static Bytes ref_sha(const Bytes& b) {
    RefSha s;
    for (uint8_t v : b) s.byte(v);
    return s.done();
}

// ------------------------------------------------------------------ the lane bodies
static bp::fe fe_of_bytes(const Bytes& b) {   // a plain little-endian load
    bp::fe r;
    for (int k = 0; k < 4; k++) {
        r.v[k] = 0;
        for (int j = 0; j < 8; j++) r.v[k] |= (u64)b[8 * k + j] << (8 * j);
    }
    return r;
}
static bool same(const bp::fe& a, const bp::fe& b) { return memcmp(&a, &b, sizeof a) == 0; }
static const bp::fe ONE = {{1, 0, 0, 0}};

static void check_seed(const Bytes& seed_in, bool expect_bit255) {
    uint8_t* heap = (uint8_t*)malloc(32);   // exactly the 32 bytes the loader may read
    memcpy(heap, seed_in.data(), 32);
    const bp::GenSeed seed = bp::gens_seed_words(heap);
    free(heap);

    std::vector<u64> idx;
    for (u64 i = 0; i <= 70; i++) idx.push_back(i);
    for (u64 c : {256ull, 65536ull, 1ull << 24})
        for (u64 i = c - 3; i < c + 3; i++) idx.push_back(i);
    for (u64 i = (1ull << 32) - 5; i < (1ull << 32); i++) idx.push_back(i);
    for (int k = 0; k < 8; k++) idx.push_back(rnd() & 0xFFFFFFFFull);
    for (u64 i : idx) {
        Bytes msg(seed_in);
        for (int k = 3; k >= 0; k--) msg.push_back((uint8_t)(i >> (8 * k)));
        const Bytes x = ref_sha(msg), y = ref_sha(x);
        const bp::ge p = bp::derive_base_point(seed, (uint32_t)i);
        CHECK(same(p.X, fe_of_bytes(x)), "vector X, index %llu", i);
        CHECK(same(p.Y, fe_of_bytes(y)), "vector Y, index %llu", i);
        CHECK(same(p.Z, ONE), "vector Z, index %llu", i);
        CHECK(same(p.T, bp::fe_mul(fe_of_bytes(x), fe_of_bytes(y))), "vector T, index %llu", i);
    }

    const Bytes x = ref_sha(seed_in);
    const bp::ge p = bp::derive_single_point(seed);
    CHECK(same(p.X, fe_of_bytes(x)), "single X");
    CHECK(same(p.Y, ONE) && same(p.Z, ONE), "single Y, Z");
    CHECK(same(p.T, bp::fe_mul(fe_of_bytes(x), ONE)), "single T");
    if (expect_bit255) {
        CHECK((x[31] & 0x80) != 0, "the seed's digest has bit 255 set");
        CHECK(!same(p.T, p.X), "single T is a product, not a copy of X");
    }
}

int main() {
    {
        const char* abc = "abc";
        const Bytes d = ref_sha(Bytes(abc, abc + 3));
        CHECK(d[0] == 0xba && d[1] == 0x78 && d[31] == 0xad, "the byte-at-a-time hash on \"abc\"");
    }
    check_seed(Bytes(32, 0x00), false);
    check_seed(Bytes(32, 0xFF), false);
    Bytes one(32, 0);
    one[0] = 1;
    check_seed(one, true);
    for (int t = 0; t < 12; t++) {
        Bytes s(32);
        for (auto& b : s) b = (uint8_t)rnd();
        check_seed(s, false);
    }
    std::printf("%llu %llu\n", checks, fails);
    return fails ? 1 : 0;
}

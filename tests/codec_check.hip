// codec_check.hip — TEST INFRASTRUCTURE (tests/test_codec_cpu.py).
//
// Runs the compact proof blob's layout, header and lane bodies (cudabulletproof_amd/csrc/bp_codec.h, the
// functions the kernels of bp_codec.hip call) in CPU loops.  Built --cuda-host-only, once plain and
// once under ASan + UBSan; a stand-alone program.
//   layout:     offsets and sizes against the format's formulas restated here
//   roundtrip:  random limbs with forced edge proofs, whole blobs and 256-proof slices
//   malformed:  every malformed blob is rejected by the parser, and the decode bodies run on the same
//               bytes with the parser bypassed, each blob in an allocation of exactly its size: they
//               stay in range (the sanitizer's check) and count what they skip
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_codec.h"

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

static u64 g_state = 0x243F6A8885A308D3ull;
static u64 rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    u64 x = g_state;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 29;
    return x;
}
static bp::fe rnd_fe() { return bp::fe{{rnd(), rnd(), rnd(), rnd()}}; }
static const bp::fe ONE = {{1, 0, 0, 0}};
static const bp::fe P = {{0xFFFFFFFFFFFFFFEDull, ~0ull, ~0ull, 0x7FFFFFFFFFFFFFFFull}};

// ------------------------------------------------------------------ a batch in flat arrays
struct Batch {
    size_t count, abl, Lr;
    std::vector<bp::ge> pt[5], L, R;
    std::vector<bp::fe> t, c, x, taux, mu, a, b;
    Batch(size_t count_, size_t abl_, size_t Lr_) : count(count_), abl(abl_), Lr(Lr_) {
        for (auto& v : pt) v.resize(count + 1);   // (+1: never an empty vector's null data())
        L.resize(count * Lr + 1); R.resize(count * Lr + 1);
        for (auto* v : {&t, &c, &x, &taux, &mu}) v->resize(count + 1);
        a.resize(count * abl + 1); b.resize(count * abl + 1);
    }
    bp::CodecArrays arrays(bool f) {
        bp::CodecArrays A;
        for (int k = 0; k < 5; k++) A.pt[k] = pt[k].data();
        A.t = t.data(); A.c = c.data(); A.x = x.data(); A.a = a.data(); A.b = b.data();
        A.taux = f ? taux.data() : nullptr; A.mu = f ? mu.data() : nullptr;
        A.L = L.data(); A.R = R.data();
        return A;
    }
    bp::ge* point(size_t i, size_t q) { return q < 5 ? &pt[q][i] : q < 5 + Lr ? &L[i * Lr + q - 5] : &R[i * Lr + q - 5 - Lr]; }
    void fill_random() {   // nothing compact about it
        for (size_t i = 0; i < count; i++) {
            for (size_t q = 0; q < 5 + 2 * Lr; q++) *point(i, q) = bp::ge{rnd_fe(), rnd_fe(), rnd_fe(), rnd_fe()};
            t[i] = rnd_fe(); c[i] = rnd_fe(); x[i] = rnd_fe(); taux[i] = rnd_fe(); mu[i] = rnd_fe();
            for (size_t k = 0; k < abl; k++) { a[i * abl + k] = rnd_fe(); b[i * abl + k] = rnd_fe(); }
        }
    }
    void make_compact(size_t i) {   // as the reference's prover leaves a proof (any limbs in X, Y: some >= p)
        for (size_t q = 0; q < 5 + 2 * Lr; q++) {
            bp::ge* g = point(i, q);
            if (q % 3 == 0) g->X.v[3] |= 1ull << 63;   // a coordinate >= p
            if (q % 5 == 1) g->Y = P;
            g->Z = ONE;
            g->T = bp::fe_mul(g->X, g->Y);
        }
        a[i * abl] = t[i]; c[i] = t[i]; b[i * abl] = ONE;
    }
    bool equal(const Batch& o, bool f) const {
        bool e = true;
        for (int k = 0; k < 5; k++) e = e && memcmp(pt[k].data(), o.pt[k].data(), count * 128) == 0;
        e = e && memcmp(L.data(), o.L.data(), count * Lr * 128) == 0 && memcmp(R.data(), o.R.data(), count * Lr * 128) == 0;
        e = e && memcmp(t.data(), o.t.data(), count * 32) == 0 && memcmp(c.data(), o.c.data(), count * 32) == 0 &&
            memcmp(x.data(), o.x.data(), count * 32) == 0;
        if (f) e = e && memcmp(taux.data(), o.taux.data(), count * 32) == 0 && memcmp(mu.data(), o.mu.data(), count * 32) == 0;
        return e && memcmp(a.data(), o.a.data(), count * abl * 32) == 0 && memcmp(b.data(), o.b.data(), count * abl * 32) == 0;
    }
};

// a blob in an allocation of exactly `bytes` bytes (one byte for none), so that a read past it is caught
struct Exact {
    uint8_t* p;
    size_t bytes;
    Exact(const uint8_t* src, size_t n) : p((uint8_t*)malloc(n ? n : 1)), bytes(n) { if (n) memcpy(p, src, n); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};

// ------------------------------------------------------------------ layout
static void layout() {
    const size_t Lrs[] = {0, 4, 6}, abls[] = {1, 2}, counts[] = {0, 1, 255, 256, 257};
    for (size_t Lr : Lrs)
        for (size_t abl : abls)
            for (int f = 0; f < 2; f++)
                for (size_t count : counts) {
                    const bp::CodecLayout l{count, abl, Lr, f};
                    const size_t Sc = abl == 1 ? 64 * (5 + 2 * Lr) + 64 + 64 * f : 0;
                    const size_t Sr = 128 * (5 + 2 * Lr) + 96 + 64 * f + 64 * abl;
                    const size_t kp = (count + 7) / 8 * 8;
                    CHECK(l.Sc() == Sc && l.Sr() == Sr, "S_c / S_r Lr=%zu abl=%zu f=%d", Lr, abl, f);
                    CHECK(l.o_kind() == 32 && l.o_compact() == 32 + kp && l.o_rawidx() == 32 + kp + count * Sc, "offsets");
                    for (size_t R : {(size_t)0, (size_t)1, count / 2, count}) {
                        if (R > count) continue;
                        const size_t ip = (4 * R + 7) / 8 * 8;
                        CHECK(l.o_raw(R) == l.o_rawidx() + ip, "o_raw R=%zu", R);
                        CHECK(l.bytes(R) == 32 + kp + count * Sc + ip + R * Sr, "bytes R=%zu", R);
                        CHECK(l.o_compact() % 8 == 0 && l.o_rawidx() % 8 == 0 && l.o_raw(R) % 8 == 0, "8-byte sections");
                    }
                    CHECK(l.bound() == l.bytes(count), "bound");
                }
    const bp::CodecLayout l64{1, 1, 6, 1};
    CHECK(l64.Sc() == 1216 && l64.Sr() == 2400, "the n = 64 sizes");
    size_t sz[bp::CDB_COUNT];
    bp::codec_sizes(257, sz);
    CHECK(sz[bp::CDB_BLK] == 3 * 4, "block counts of 257 proofs");
    bp::codec_sizes(bp::CODEC_MAX_COUNT, sz);
    CHECK(sz[bp::CDB_BLK] == (bp::CODEC_MAX_BLOCKS + 1) * 4, "block counts at the limit");
}

// ------------------------------------------------------------------ round trips
// the edge proofs forced into a compact batch: index -> what is broken; all must come out raw
enum Edge { Z_P1, T_LIMB3, A_NE_T, B_1P, C_NE_T, ZEROED, EDGES };
static void force_edge(Batch& b, size_t i, int e) {
    switch (e) {
    case Z_P1: b.point(i, 2)->Z = bp::fe{{P.v[0] + 1, P.v[1], P.v[2], P.v[3]}}; break;   // p + 1
    case T_LIMB3: b.point(i, 5 + 2 * b.Lr - 1)->T.v[3] ^= 1; break;
    case A_NE_T: b.a[i * b.abl].v[0] ^= 2; break;
    case B_1P: b.b[i * b.abl] = bp::fe{{P.v[0] + 1, P.v[1], P.v[2], P.v[3]}}; break;     // 1 + p
    case C_NE_T: b.c[i].v[2] += 1; break;
    case ZEROED:   // the prover's valid = 0 proof: b = 0
        for (size_t q = 0; q < 5 + 2 * b.Lr; q++) *b.point(i, q) = q < 5 ? bp::ge_zero() : bp::ge{};
        b.t[i] = b.c[i] = b.x[i] = b.taux[i] = b.mu[i] = bp::fe{};
        b.a[i * b.abl] = b.b[i * b.abl] = bp::fe{};
        break;
    }
}

static std::vector<uint8_t> encode(Batch& b, int f, size_t n, size_t* R) {
    const bp::CodecLayout l{b.count, b.abl, b.Lr, f};
    std::vector<uint8_t> blob(l.bound() + 1, 0xAB);   // (stale bytes: the encoder must write all it owns)
    const size_t bytes = bp::codec_encode_cpu(blob.data(), b.arrays(f), l, n);
    CHECK(bytes <= l.bound() && blob[l.bound()] == 0xAB, "encoder stays inside the bound");
    blob.resize(bytes);
    *R = (size_t)bp::get_le(blob.data() + 20, 4);
    return blob;
}

static void roundtrip_one(size_t count, size_t abl, size_t Lr, int f, const std::vector<size_t>& raw_at) {
    const size_t n = (size_t)1 << Lr;
    Batch b(count, abl, Lr);
    b.fill_random();
    if (abl == 1)
        for (size_t i = 0; i < count; i++) b.make_compact(i);
    std::vector<uint8_t> want_kind(count, abl == 1 ? 0 : 1);
    for (size_t k = 0; k < raw_at.size(); k++)
        if (raw_at[k] < count) { force_edge(b, raw_at[k], (int)(k % EDGES)); want_kind[raw_at[k]] = 1; }
    size_t R = 0;
    const std::vector<uint8_t> blob = encode(b, f, n, &R);
    const bp::CodecLayout l{count, abl, Lr, f};
    size_t wantR = 0;
    for (size_t i = 0; i < count; i++) {
        CHECK(blob[32 + i] == want_kind[i], "kind[%zu] = %d, want %d (count %zu)", i, blob[32 + i], want_kind[i], count);
        wantR += want_kind[i];
    }
    CHECK(R == wantR && blob.size() == l.bytes(wantR), "R and size");
    hipbp_proof_blob_info info;
    const Exact ex(blob.data(), blob.size());
    const char* e = bp::codec_parse(ex.p, ex.bytes, &info);
    CHECK(e == nullptr, "parse: %s", e ? e : "");
    CHECK(info.count == count && info.n == n && info.ab_len == abl && info.L_len == Lr && info.flags == (unsigned)f &&
              info.raw_count == wantR && info.bytes == blob.size(), "info");
    // determinism: the same proofs encode to the same bytes whatever the buffer held
    {
        std::vector<uint8_t> again(l.bound(), 0x11);
        bp::codec_encode_cpu(again.data(), b.arrays(f), l, n);
        CHECK(memcmp(again.data(), blob.data(), blob.size()) == 0, "deterministic bytes");
    }
    // whole-blob decode
    Batch d(count, abl, Lr);
    d.fill_random();
    size_t bad = bp::codec_decode_cpu(bp::codec_view(ex.p, ex.bytes, l, info.raw_count), d.arrays(f), l);
    CHECK(bad == 0, "bad = %zu on a well-formed blob", bad);
    CHECK(d.equal(b, f), "round trip count=%zu abl=%zu Lr=%zu f=%d", count, abl, Lr, f);
    // 256-proof slices, as the host verifier cuts them: copied out, each part in an exact allocation
    for (size_t c0 = 0; c0 < count; c0 += 256) {
        const size_t c = count - c0 < 256 ? count - c0 : 256;
        const uint8_t* ri = ex.p + l.o_rawidx();
        const size_t j0 = bp::codec_raw_lower(ri, info.raw_count, c0), nr = bp::codec_raw_lower(ri, info.raw_count, c0 + c) - j0;
        const Exact kind(ex.p + l.o_kind() + c0, c), cmp(ex.p + l.o_compact() + c0 * l.Sc(), c * l.Sc()),
            idx(ri + 4 * j0, 4 * nr), raw(ex.p + l.o_raw(info.raw_count) + j0 * l.Sr(), nr * l.Sr());
        bp::BlobView v;
        v.kind = kind.p; v.compact = cmp.p; v.rawidx = idx.p; v.raw = raw.p;
        v.count = c; v.R = nr; v.base = c0;
        v.kind_n = v.compact_n = c; v.rawidx_n = v.raw_n = nr;
        Batch s(c, abl, Lr);
        s.fill_random();
        bad = bp::codec_decode_cpu(v, s.arrays(f), l);
        CHECK(bad == 0, "slice bad = %zu", bad);
        bool same = true;
        for (size_t i = 0; i < c && same; i++) {
            for (size_t q = 0; q < 5 + 2 * Lr; q++) same = same && memcmp(s.point(i, q), b.point(c0 + i, q), 128) == 0;
            same = same && memcmp(&s.t[i], &b.t[c0 + i], 32) == 0 && memcmp(&s.c[i], &b.c[c0 + i], 32) == 0 &&
                   memcmp(&s.x[i], &b.x[c0 + i], 32) == 0 && memcmp(&s.a[i * abl], &b.a[(c0 + i) * abl], abl * 32) == 0 &&
                   memcmp(&s.b[i * abl], &b.b[(c0 + i) * abl], abl * 32) == 0;
            if (f) same = same && memcmp(&s.taux[i], &b.taux[c0 + i], 32) == 0 && memcmp(&s.mu[i], &b.mu[c0 + i], 32) == 0;
        }
        CHECK(same, "slice at %zu", c0);
    }
}

static void roundtrips() {
    for (size_t Lr : {(size_t)0, (size_t)4, (size_t)6})
        for (int f = 0; f < 2; f++) {
            roundtrip_one(0, 1, Lr, f, {});
            roundtrip_one(1, 1, Lr, f, {});
            roundtrip_one(1, 1, Lr, f, {0});
            roundtrip_one(13, 1, Lr, f, {1, 2, 3, 4, 5, 6});                 // one of every edge
            roundtrip_one(600, 1, Lr, f, {0, 255, 256, 257, 599, 300, 301});   // both sides of a block boundary, both ends
            roundtrip_one(257, 1, Lr, f, {});                                 // R = 0
            roundtrip_one(7, 2, Lr, f, {});                                   // ab_len 2: no compact slots
        }
    // each edge alone makes its proof raw; coordinates >= p alone do not
    for (int e = 0; e < EDGES; e++) {
        Batch b(3, 1, 4);
        b.fill_random();
        for (size_t i = 0; i < 3; i++) b.make_compact(i);
        const bp::CodecLayout l{3, 1, 4, 1};
        CHECK(bp::codec_classify(b.arrays(true), l, 1) == 0, "compact before the edge");
        force_edge(b, 1, e);
        CHECK(bp::codec_classify(b.arrays(true), l, 1) == 1, "edge %d makes the proof raw", e);
        CHECK(bp::codec_classify(b.arrays(true), l, 0) == 0 && bp::codec_classify(b.arrays(true), l, 2) == 0, "neighbours stay compact");
    }
}

// ------------------------------------------------------------------ malformed blobs
// parse must refuse; then the decode bodies on the same bytes, the parser bypassed (the header's
// fields taken as they are, the view cut to the bytes held)
static void expect_bad(const std::vector<uint8_t>& blob, size_t bytes, const char* what, bool must_count, size_t count,
                       size_t abl, size_t Lr) {
    const Exact ex(blob.data(), bytes);
    hipbp_proof_blob_info info;
    CHECK(bp::codec_parse(ex.p, ex.bytes, &info) != nullptr, "parse accepted: %s", what);
    if (bytes < 32) return;
    const int f = (int)(bp::get_le(ex.p + 6, 2) & 1);
    const size_t R = (size_t)bp::get_le(ex.p + 20, 4);
    const bp::CodecLayout l{count, abl, Lr, f};   // (count, ab_len, L_len: never altered below)
    Batch d(count, abl, Lr);
    const size_t bad = bp::codec_decode_cpu(bp::codec_view(ex.p, ex.bytes, l, R), d.arrays(f), l);
    if (must_count) CHECK(bad > 0, "decode counted nothing: %s", what);
    CHECK(bad <= count + R, "bad count in range: %s", what);
}

static void malformed() {
    for (int f = 0; f < 2; f++) {
        const size_t count = 21, Lr = 4, n = 16;
        Batch b(count, 1, Lr);
        b.fill_random();
        for (size_t i = 0; i < count; i++) b.make_compact(i);
        for (size_t i : {(size_t)2, (size_t)9, (size_t)20}) force_edge(b, i, T_LIMB3);   // R = 3 (odd: raw_index is padded)
        size_t R = 0;
        const std::vector<uint8_t> good = encode(b, f, n, &R);
        const bp::CodecLayout l{count, 1, Lr, f};
        CHECK(R == 3 && l.o_compact() - l.o_kind() > count && l.o_raw(R) - l.o_rawidx() > 4 * R, "the blob has both paddings");
        hipbp_proof_blob_info info;
        CHECK(bp::codec_parse(good.data(), good.size(), &info) == nullptr, "the unaltered blob parses");
        auto alter = [&](size_t off, uint8_t v, const char* what, bool must_count) {
            std::vector<uint8_t> m = good;
            m[off] = v;
            expect_bad(m, m.size(), what, must_count, count, 1, Lr);
        };
        alter(0, 'X', "magic", false);
        alter(4, 2, "version", false);
        alter(6, (uint8_t)(f | 2), "flag bits", false);
        alter(7, 1, "flag bits (high byte)", false);
        // truncation by one byte at every section boundary, and below the header
        for (size_t cut : {l.o_compact(), l.o_rawidx(), l.o_raw(R), good.size()}) expect_bad(good, cut - 1, "truncated", true, count, 1, Lr);
        expect_bad(good, 31, "shorter than the header", false, count, 1, Lr);
        expect_bad(good, good.size() - l.Sr(), "a record short", true, count, 1, Lr);
        {   // one byte too long
            std::vector<uint8_t> m = good;
            m.push_back(0);
            expect_bad(m, m.size(), "one byte long", false, count, 1, Lr);
        }
        alter(l.o_kind() + 5, 2, "kind of 2", true);
        alter(l.o_kind() + 5, 1, "a raw kind raw_index does not name", true);
        alter(l.o_kind() + 9, 0, "a compact kind raw_index names", true);
        alter(20, (uint8_t)(R + 1), "R one too many", true);
        alter(20, (uint8_t)(R - 1), "R one too few", true);
        auto idx = [&](size_t j, uint32_t v, const char* what) {
            std::vector<uint8_t> m = good;
            bp::put_le(m.data() + l.o_rawidx() + 4 * j, v, 4);
            expect_bad(m, m.size(), what, true, count, 1, Lr);
        };
        {   // unsorted: the first two swapped
            std::vector<uint8_t> m = good;
            bp::put_le(m.data() + l.o_rawidx(), 9, 4);
            bp::put_le(m.data() + l.o_rawidx() + 4, 2, 4);
            expect_bad(m, m.size(), "raw_index unsorted", true, count, 1, Lr);
        }
        idx(1, 2, "raw_index duplicated");
        idx(2, (uint32_t)count, "raw_index = count");
        idx(2, 0xFFFFFFFFu, "raw_index far above count");
        idx(1, 10, "raw_index names a compact proof");
        alter(l.o_kind() + count, 1, "padding after kind", false);
        alter(l.o_rawidx() + 4 * R + 1, 7, "padding after raw_index", false);
        alter(l.o_compact() + 2 * l.Sc() + 17, 1, "a raw proof's slot not zero", false);
    }
}

int main() {
    layout();
    roundtrips();
    malformed();
    std::printf("%llu %llu\n", checks, fails);
    return fails ? 1 : 0;
}

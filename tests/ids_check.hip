// ids_check.hip — TEST INFRASTRUCTURE (tests/test_proof_ids_cpu.py).
//
// Runs the proof ids' and the Merkle tree's lane bodies (cudabulletproof_amd/csrc/bp_ids.h, the functions
// the kernels of bp_ids.hip call) in CPU loops against a byte-at-a-time SHA-256 written here.  Built
// --cuda-host-only, once plain and once under ASan + UBSan; a stand-alone program.
//   sha:        the piece-wise hash on messages of 1 .. 12 pieces: both tail shapes, and the empty message
//   ids:        flat and blob ids of batches with forced raw proofs, L_len 0 / 4 / 6, ab_len 1 / 2, f 0 / 1,
//               against SHA-256(hdr | the record's bytes as the encoder wrote them)
//   merkle:     leaf, node, every level, the root against the recursive RFC 6962 form, paths and their check
//   malformed:  the blob body on truncated blobs, out-of-range and unsorted raw_index entries and bad kinds,
//               each blob in an allocation of exactly its size: it stays in range (the sanitizer's
//               check), counts what fails and gives those the all-zero id
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_ids.h"

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

static u64 g_state = 0x13198A2E03707344ull;
static u64 rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    u64 x = g_state;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 29;
    return x;
}
static bp::fe rnd_fe() { return bp::fe{{rnd(), rnd(), rnd(), rnd()}}; }
static const bp::fe ONE = {{1, 0, 0, 0}};

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
static Bytes ref_sha(const uint8_t* p, size_t n) {
    RefSha s;
    for (size_t i = 0; i < n; i++) s.byte(p[i]);
    return s.done();
}
static Bytes ref_sha(const Bytes& b) { return ref_sha(b.data(), b.size()); }
static std::string hex(const Bytes& b) {
    std::string s;
    char t[3];
    for (uint8_t v : b) { std::snprintf(t, 3, "%02x", v); s += t; }
    return s;
}

// ------------------------------------------------------------------ sha: the piece-wise hash
static Bytes header(uint8_t kind, int f, size_t n, size_t abl, size_t Lr) {
    Bytes h(32, 0);
    memcpy(h.data(), "hipbpProofIdV1", 14);
    h[14] = kind; h[15] = (uint8_t)f;
    bp::put_le(h.data() + 16, n, 4); bp::put_le(h.data() + 20, abl, 4); bp::put_le(h.data() + 24, Lr, 4);
    return h;
}
static void sha_shapes() {
    CHECK(hex(ref_sha(nullptr, 0)) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855", "the reference on the empty message");
    const uint8_t abc[3] = {'a', 'b', 'c'};
    CHECK(hex(ref_sha(abc, 3)) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad", "the reference on abc");
    uint32_t d[8];
    uint8_t out[32];
    bp::merkle_empty(d);
    bp::ids_store(out, d);
    CHECK(hex(Bytes(out, out + 32)) == hex(ref_sha(nullptr, 0)), "merkle_empty");
    // hdr | P random pieces: P even ends half a block (a compact record), P odd a whole one (a raw record)
    for (size_t P = 1; P <= 12; P++) {
        Bytes rec(32 * P);
        for (auto& v : rec) v = (uint8_t)rnd();
        const bp::CodecLayout l{1, 3, 5, (int)(P & 1)};
        Bytes msg = header((uint8_t)(P % 2), l.f, 1u << 20, 3, 5);
        msg.insert(msg.end(), rec.begin(), rec.end());
        bp::ids_hash_record((uint8_t)(P % 2), l, (size_t)1 << 20, P, [&](size_t r, bp::u128& a, bp::u128& b) {
            memcpy(&a, rec.data() + 32 * r, 16); memcpy(&b, rec.data() + 32 * r + 16, 16); }, d);
        bp::ids_store(out, d);
        CHECK(msg.size() % 64 == (P % 2 ? 0u : 32u), "tail shape");
        CHECK(memcmp(out, ref_sha(msg).data(), 32) == 0, "pieces = %zu", P);
        uint32_t back[8];
        bp::ids_load(out, back);
        CHECK(memcmp(back, d, 32) == 0, "ids_load(ids_store)");
    }
}

// ------------------------------------------------------------------ a batch in flat arrays
struct Batch {
    size_t count, abl, Lr;
    std::vector<bp::ge> pt[5], L, R;
    std::vector<bp::fe> t, c, x, taux, mu, a, b;
    Batch(size_t count_, size_t abl_, size_t Lr_) : count(count_), abl(abl_), Lr(Lr_) {
        for (auto& v : pt) v.resize(count + 1);
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
    void fill(bool compact) {
        for (size_t i = 0; i < count; i++) {
            for (size_t q = 0; q < 5 + 2 * Lr; q++) {
                bp::ge* g = point(i, q);
                *g = bp::ge{rnd_fe(), rnd_fe(), rnd_fe(), rnd_fe()};
                if (compact) { g->Z = ONE; g->T = bp::fe_mul(g->X, g->Y); }
            }
            t[i] = rnd_fe(); c[i] = rnd_fe(); x[i] = rnd_fe(); taux[i] = rnd_fe(); mu[i] = rnd_fe();
            for (size_t k = 0; k < abl; k++) { a[i * abl + k] = rnd_fe(); b[i * abl + k] = rnd_fe(); }
            if (compact) { a[i * abl] = t[i]; c[i] = t[i]; b[i * abl] = ONE; }
        }
    }
};

struct Exact {   // a blob in an allocation of exactly `bytes` bytes
    uint8_t* p;
    size_t bytes;
    Exact(const uint8_t* src, size_t n) : p((uint8_t*)malloc(n ? n : 1)), bytes(n) { if (n) memcpy(p, src, n); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};

static Bytes encode(Batch& b, int f, size_t n) {
    const bp::CodecLayout l{b.count, b.abl, b.Lr, f};
    Bytes blob(l.bound());
    blob.resize(bp::codec_encode_cpu(blob.data(), b.arrays(f), l, n));
    return blob;
}

// the id of proof i from the blob's own bytes: the record found by a linear walk, hashed a byte at a time
static Bytes ref_id(const Bytes& blob, const bp::CodecLayout& l, size_t n, size_t i) {
    const size_t R = (size_t)bp::get_le(blob.data() + 20, 4);
    const uint8_t kind = blob[l.o_kind() + i];
    size_t j = 0;
    for (size_t k = 0; k < i; k++) j += blob[l.o_kind() + k];
    const uint8_t* rec = kind ? blob.data() + l.o_raw(R) + j * l.Sr() : blob.data() + l.o_compact() + i * l.Sc();
    Bytes msg = header(kind, l.f, n, l.abl, l.Lr);
    msg.insert(msg.end(), rec, rec + (kind ? l.Sr() : l.Sc()));
    return ref_sha(msg);
}

static void ids_one(size_t count, size_t abl, size_t Lr, int f, const std::vector<size_t>& raw_at) {
    const size_t n = (size_t)1 << Lr;
    Batch b(count, abl, Lr);
    b.fill(abl == 1);
    for (size_t k = 0; k < raw_at.size(); k++)
        if (raw_at[k] < count) {
            if (k % 2) b.point(raw_at[k], k % (5 + 2 * Lr))->T.v[3] ^= 1;
            else b.b[raw_at[k] * abl].v[3] |= 1ull << 62;
        }
    const bp::CodecLayout l{count, abl, Lr, f};
    const Bytes blob = encode(b, f, n);
    const Exact ex(blob.data(), blob.size());
    hipbp_proof_blob_info info;
    CHECK(bp::codec_parse(ex.p, ex.bytes, &info) == nullptr, "the blob parses");
    const bp::BlobView v = bp::codec_view(ex.p, ex.bytes, l, info.raw_count);
    size_t raws = 0;
    for (size_t i = 0; i < count; i++) {
        const Bytes want = ref_id(blob, l, n, i);
        uint8_t got[32], got2[32];
        const uint8_t kind = bp::ids_flat_proof(b.arrays(f), l, n, i, got);
        CHECK(kind == blob[l.o_kind() + i], "kind of proof %zu", i);
        CHECK(memcmp(got, want.data(), 32) == 0, "flat id %zu (count %zu abl %zu Lr %zu f %d kind %d)", i, count, abl, Lr, f, kind);
        CHECK(bp::ids_blob_proof(v, l, n, i, got2) == 0, "blob id %zu counted as bad", i);
        CHECK(memcmp(got2, want.data(), 32) == 0, "blob id %zu", i);
        raws += kind;
        // f and kind are hashed: the other f gives another id
        if (i == 0) {
            const bp::CodecLayout lo{count, abl, Lr, 1 - f};
            uint8_t other[32];
            bp::ids_flat_proof(b.arrays(true), lo, n, i, other);
            CHECK(memcmp(other, got, 32) != 0, "f is part of the id");
        }
    }
    CHECK(raws == info.raw_count, "raw proofs");
}

static void ids() {
    for (size_t Lr : {(size_t)0, (size_t)4, (size_t)6})
        for (int f = 0; f < 2; f++) {
            ids_one(1, 1, Lr, f, {});
            ids_one(1, 1, Lr, f, {0});
            ids_one(13, 1, Lr, f, {1, 2, 3, 7, 12});
            ids_one(7, 2, Lr, f, {});   // ab_len 2: every proof raw
            ids_one(0, 1, Lr, f, {});
        }
    ids_one(300, 1, 4, 1, {0, 255, 256, 257, 299});
}

// ------------------------------------------------------------------ merkle
static Bytes cat(uint8_t tag, const Bytes& a, const Bytes& b = Bytes()) {
    Bytes m(1, tag);
    m.insert(m.end(), a.begin(), a.end());
    m.insert(m.end(), b.begin(), b.end());
    return m;
}
static size_t split(size_t n) {
    size_t k = 1;
    while (2 * k < n) k *= 2;
    return k;
}
static Bytes mth(const std::vector<Bytes>& d, size_t lo, size_t hi) {   // RFC 6962 §2.1
    if (hi == lo) return ref_sha(nullptr, 0);
    if (hi - lo == 1) return ref_sha(cat(0, d[lo]));
    const size_t k = split(hi - lo);
    return ref_sha(cat(1, mth(d, lo, lo + k), mth(d, lo + k, hi)));
}
static void path_ref(const std::vector<Bytes>& d, size_t lo, size_t hi, size_t m, std::vector<Bytes>& out) {   // §2.1.1
    if (hi - lo == 1) return;
    const size_t k = split(hi - lo);
    if (m < k) { path_ref(d, lo, lo + k, m, out); out.push_back(mth(d, lo + k, hi)); }
    else { path_ref(d, lo + k, hi, m - k, out); out.push_back(mth(d, lo, lo + k)); }
}

static void merkle() {
    for (size_t count = 0; count <= 40; count++) {
        std::vector<Bytes> d(count);
        Bytes flat;
        for (auto& id : d) {
            id.resize(32);
            for (auto& v : id) v = (uint8_t)rnd();
            flat.insert(flat.end(), id.begin(), id.end());
        }
        const Bytes want = mth(d, 0, count);
        if (count == 0) continue;   // (merkle_empty: sha_shapes)
        const Exact ids(flat.data(), flat.size());
        std::vector<Bytes> lv;
        bp::merkle_levels_cpu(ids.p, count, lv);
        CHECK(lv.back().size() == 32 && lv.back() == want, "root of %zu", count);
        CHECK(lv[0].size() == 32 * count && Bytes(lv[0].begin(), lv[0].begin() + 32) == ref_sha(cat(0, d[0])), "leaf");
        // level 0 fused with the leaf hash gives level 1
        if (count > 1) {
            Bytes l1(32 * bp::merkle_up(count));
            for (size_t k = 0; k < bp::merkle_up(count); k++) bp::merkle_level_node<true>(ids.p, count, k, l1.data());
            CHECK(l1 == lv[1], "fused level 1 of %zu", count);
        }
        for (size_t i = 0; i < count; i++) {
            std::vector<Bytes> pw;
            path_ref(d, 0, count, i, pw);
            uint8_t path[32 * (bp::MERKLE_MAX_PATH + 1)];
            const size_t len = bp::merkle_path_cpu(lv, count, i, path);
            bool same = len == pw.size();
            for (size_t k = 0; same && k < len; k++) same = memcmp(path + 32 * k, pw[k].data(), 32) == 0;
            CHECK(same, "path of %zu in %zu", i, count);
            CHECK(bp::merkle_verify_cpu(d[i].data(), i, count, path, len, want.data()), "verify %zu in %zu", i, count);
            CHECK(!bp::merkle_verify_cpu(d[i].data(), (i + 1) % count, count, path, len, want.data()) || count == 1, "wrong index");
            CHECK(!bp::merkle_verify_cpu(d[i].data(), count, count, path, len, want.data()), "index = count");
            if (len) CHECK(!bp::merkle_verify_cpu(d[i].data(), i, count, path, len - 1, want.data()), "a path one short");
            memcpy(path + 32 * len, path, 32);
            CHECK(!bp::merkle_verify_cpu(d[i].data(), i, count, path, len + 1, want.data()), "a path one long");
            if (len) {
                path[32 * (len - 1) + 5] ^= 0x10;
                CHECK(!bp::merkle_verify_cpu(d[i].data(), i, count, path, len, want.data()), "a flipped bit");
            }
        }
    }
    // node against the reference
    Bytes a(32), b(32);
    for (auto& v : a) v = (uint8_t)rnd();
    for (auto& v : b) v = (uint8_t)rnd();
    uint32_t wa[8], wb[8], d[8];
    uint8_t out[32];
    bp::ids_load(a.data(), wa); bp::ids_load(b.data(), wb);
    bp::merkle_node(wa, wb, d);
    bp::ids_store(out, d);
    CHECK(Bytes(out, out + 32) == ref_sha(cat(1, a, b)), "node");
}

// ------------------------------------------------------------------ malformed blobs
// the body over every proof of the bytes held, the parser bypassed (the header's R taken as it is, the
// view cut to the bytes): in range, the failed ones counted and zero
static void run_bad(const Bytes& blob, size_t bytes, const char* what, bool must_count, size_t count, size_t Lr) {
    const Exact ex(blob.data(), bytes);
    const int f = (int)(bp::get_le(ex.p + 6, 2) & 1);
    const size_t R = (size_t)bp::get_le(ex.p + 20, 4);
    const bp::CodecLayout l{count, 1, Lr, f};
    const bp::BlobView v = bp::codec_view(ex.p, ex.bytes, l, R);
    size_t bad = 0;
    const uint8_t zero[32] = {0};
    for (size_t i = 0; i < count; i++) {
        uint8_t id[32];
        memset(id, 0xEE, 32);
        const unsigned r = bp::ids_blob_proof(v, l, (size_t)1 << Lr, i, id);
        CHECK(r <= 1 && (r == 1) == (memcmp(id, zero, 32) == 0), "a failed record has the zero id, no other: %s", what);
        bad += r;
    }
    if (must_count) CHECK(bad > 0, "counted nothing: %s", what);
    CHECK(bad <= count, "bad count in range: %s", what);
}

static void malformed() {
    for (int f = 0; f < 2; f++) {
        const size_t count = 21, Lr = 4, n = 16;
        Batch b(count, 1, Lr);
        b.fill(true);
        for (size_t i : {(size_t)2, (size_t)9, (size_t)20}) b.point(i, 3)->T.v[3] ^= 1;   // R = 3
        const Bytes good = encode(b, f, n);
        const bp::CodecLayout l{count, 1, Lr, f};
        const size_t R = (size_t)bp::get_le(good.data() + 20, 4);
        CHECK(R == 3, "three raw proofs");
        run_bad(good, good.size(), "the unaltered blob", false, count, Lr);
        {   // ... on which nothing is counted
            const bp::BlobView v = bp::codec_view(good.data(), good.size(), l, R);
            uint8_t id[32];
            size_t bad = 0;
            for (size_t i = 0; i < count; i++) bad += bp::ids_blob_proof(v, l, n, i, id);
            CHECK(bad == 0, "bad = %zu on a well-formed blob", bad);
        }
        for (size_t cut : {l.o_compact(), l.o_rawidx(), l.o_raw(R), good.size()}) run_bad(good, cut - 1, "truncated", true, count, Lr);
        run_bad(good, good.size() - l.Sr(), "a record short", true, count, Lr);
        run_bad(good, 32, "the header alone", true, count, Lr);
        auto alter = [&](size_t off, uint8_t v, const char* what, bool must_count) {
            Bytes m = good;
            m[off] = v;
            run_bad(m, m.size(), what, must_count, count, Lr);
        };
        alter(l.o_kind() + 5, 2, "kind of 2", true);
        alter(l.o_kind() + 5, 1, "a raw kind raw_index does not name", true);
        alter(20, (uint8_t)(R + 1), "R one too many", false);
        alter(20, (uint8_t)(R - 1), "R one too few", true);
        alter(20, 0, "R of zero", true);
        auto idx = [&](size_t j, uint32_t v, const char* what) {
            Bytes m = good;
            bp::put_le(m.data() + l.o_rawidx() + 4 * j, v, 4);
            run_bad(m, m.size(), what, true, count, Lr);
        };
        {   // unsorted: the first two swapped
            Bytes m = good;
            bp::put_le(m.data() + l.o_rawidx(), 9, 4);
            bp::put_le(m.data() + l.o_rawidx() + 4, 2, 4);
            run_bad(m, m.size(), "raw_index unsorted", true, count, Lr);
        }
        idx(1, 2, "raw_index duplicated");
        idx(2, (uint32_t)count, "raw_index = count");
        idx(2, 0xFFFFFFFFu, "raw_index far above count");
        idx(0, 0xFFFFFFF0u, "raw_index[0] far above count");
        idx(1, 10, "raw_index names a compact proof");
    }
    // ab_len = 2 has no compact slots: a kind of 0 there fails
    Batch b(3, 2, 4);
    b.fill(false);
    Bytes m = encode(b, 1, 16);
    const bp::CodecLayout l{3, 2, 4, 1};
    m[l.o_kind() + 1] = 0;
    const bp::BlobView v = bp::codec_view(m.data(), m.size(), l, 3);
    uint8_t id[32];
    CHECK(bp::ids_blob_proof(v, l, 16, 1, id) == 1, "a compact kind without compact slots");
    CHECK(bp::ids_blob_proof(v, l, 16, 0, id) == 0 && bp::ids_blob_proof(v, l, 16, 2, id) == 0, "its neighbours");
}

int main() {
    sha_shapes();
    ids();
    merkle();
    malformed();
    std::printf("%llu %llu\n", checks, fails);
    return fails ? 1 : 0;
}

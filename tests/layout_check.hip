// layout_check.hip — TEST INFRASTRUCTURE (tests/test_layout.py).
//
// Runs the flat batch layouts and workspace tables of cudabulletproof_amd/csrc/bp_layout.h (host-only)
// on the CPU.  The expected offsets and sizes are restated here as plain formulas (32-byte field
// elements, 128-byte points), independent of the header's own constants and helpers.
//   offsets:   the verify chunk and the proof output over a sweep of shapes: every region where the
//              formulas put it, in order, disjoint, 32-byte aligned relative to the base
//   pack:      proofs with distinct bytes in every field, packed and read back through the batch view
//   unpack:    a pattern written through the hipbp_proof_out view, unpacked into RangeProof structs
//   tables:    every workspace buffer's bytes
//   pippenger: the Pippenger part's shape and buffer bytes over a grid of shapes
//   gen_view:  the generator view: pack_gens / GenView::at round trips, the packed order, the table rule
// Prints "<checks> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// deterministic distinct bytes
static u64 g_state = 0x1234567;
static void fill(void* p, size_t len) {
    uint8_t* q = (uint8_t*)p;
    for (size_t i = 0; i < len; i++) {
        g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
        q[i] = (uint8_t)(g_state >> 56) | 1;   // never zero: a zeroed region is told apart
    }
}
template <class T>
static bool same(const T& a, const T& b) { return memcmp(&a, &b, sizeof(T)) == 0; }
static bool all_zero(const void* p, size_t len) {
    for (size_t i = 0; i < len; i++) if (((const uint8_t*)p)[i]) return false;
    return true;
}

struct Region { const void* p; size_t len; };
// the regions start at base + off0, follow each other in order without overlap, each 32-byte aligned
// relative to the base; returns the end offset of the last
static size_t check_regions(const uint8_t* base, const std::vector<Region>& rg, const std::vector<size_t>& want) {
    size_t end = 0;
    for (size_t i = 0; i < rg.size(); i++) {
        const size_t off = (size_t)((const uint8_t*)rg[i].p - base);
        CHECK(off == want[i], "region %zu at %zu, want %zu", i, off, want[i]);
        CHECK(off % 32 == 0, "region %zu not 32-byte aligned", i);
        CHECK(off >= end, "region %zu overlaps its predecessor", i);
        end = off + rg[i].len;
    }
    return end;
}

static void offsets() {
    const size_t cs[] = {1, 2, 3, 1024}, abls[] = {1, 2, 3}, Lrs[] = {0, 1, 6, 16};
    for (size_t c : cs)
        for (size_t Lr : Lrs) {
            for (size_t abl : abls) {
                const bp::ChunkLayout l{c, abl, Lr};
                const size_t bytes = c * (5 * 128 + 3 * 32 + 2 * abl * 32 + 2 * Lr * 128);
                CHECK(l.bytes() == bytes, "chunk bytes c=%zu abl=%zu Lr=%zu", c, abl, Lr);
                uint8_t* base = (uint8_t*)malloc(bytes);
                hipbp_proof_batch b;
                memset(&b, 0xEE, sizeof b);
                l.view(base, &b);
                CHECK(b.count == c && b.ab_len == abl && b.L_len == Lr, "chunk view header");
                std::vector<Region> rg = {{b.V, c * 128}, {b.A, c * 128}, {b.S, c * 128}, {b.T1, c * 128}, {b.T2, c * 128},
                                          {b.t, c * 32}, {b.c, c * 32}, {b.x, c * 32}, {b.a, c * abl * 32},
                                          {b.b, c * abl * 32}};
                std::vector<size_t> want;
                for (size_t i = 0; i < 5; i++) want.push_back(i * c * 128);
                for (size_t i = 0; i < 3; i++) want.push_back(5 * c * 128 + i * c * 32);
                for (size_t i = 0; i < 2; i++) want.push_back(5 * c * 128 + 3 * c * 32 + i * c * abl * 32);
                if (Lr) {
                    rg.push_back({b.L, c * Lr * 128});
                    rg.push_back({b.R, c * Lr * 128});
                    for (size_t i = 0; i < 2; i++)
                        want.push_back(5 * c * 128 + 3 * c * 32 + 2 * c * abl * 32 + i * c * Lr * 128);
                } else {
                    CHECK(!b.L && !b.R, "L, R must be null at Lr = 0");
                }
                CHECK(check_regions(base, rg, want) == bytes, "chunk regions do not fill the chunk");
                free(base);
            }
            const size_t caps[] = {c, c + 1, 16384};
            for (size_t CH : caps)
                for (int with_lead = 0; with_lead < 2; with_lead++) {
                    // the prove-host slot's formulas (lead = its v | gamma region; 0: outputs alone)
                    const size_t o_pts = with_lead ? 2 * CH * 32 : 0, o_fe = o_pts + 5 * CH * 128;
                    const size_t o_lr = o_fe + 7 * CH * 32, o_valid = o_lr + 2 * CH * Lr * 128;
                    const size_t slot_bytes = (o_valid + CH + 127) & ~(size_t)127;
                    const bp::OutLayout l{CH, c, Lr, o_pts};
                    CHECK(l.o_pts() == o_pts && l.o_fe() == o_fe && l.o_lr() == o_lr && l.o_valid() == o_valid,
                          "output offsets cap=%zu c=%zu Lr=%zu", CH, c, Lr);
                    CHECK(l.slot_bytes() == slot_bytes && l.end() == o_valid + CH, "output bytes cap=%zu Lr=%zu", CH, Lr);
                    CHECK(l.used() == o_valid + c - o_pts, "output D2H bytes");
                    uint8_t* base = (uint8_t*)malloc(slot_bytes);
                    hipbp_proof_out o;
                    l.view(base, &o);
                    std::vector<Region> rg = {{o.V, c * 128}, {o.A, c * 128}, {o.S, c * 128}, {o.T1, c * 128},
                                              {o.T2, c * 128}, {o.taux, c * 32}, {o.mu, c * 32}, {o.t, c * 32},
                                              {o.c, c * 32}, {o.x, c * 32}, {o.a, c * 32}, {o.b, c * 32}};
                    std::vector<size_t> want;
                    for (size_t i = 0; i < 5; i++) want.push_back(o_pts + i * c * 128);
                    for (size_t i = 0; i < 7; i++) want.push_back(o_fe + i * c * 32);
                    if (Lr) {
                        rg.push_back({o.L, c * Lr * 128});
                        rg.push_back({o.R, c * Lr * 128});
                        want.push_back(o_lr);
                        want.push_back(o_lr + c * Lr * 128);
                    } else {
                        CHECK(!o.L && !o.R, "L, R must be null at Lr = 0");
                    }
                    rg.push_back({o.valid, c});
                    want.push_back(o_valid);
                    CHECK(check_regions(base, rg, want) <= slot_bytes, "output regions leave the slot");
                    // the packed arrays stay inside their cap-sized regions
                    CHECK(5 * c * 128 <= o_fe - o_pts && 7 * c * 32 <= o_lr - o_fe && 2 * c * Lr * 128 <= o_valid - o_lr,
                          "packed arrays leave their regions");
                    free(base);
                }
        }
}

// c proofs of one shape, every field and vector filled with distinct bytes
struct Proofs {
    std::vector<RangeProof> rp;
    std::vector<ge25519> V;
    std::vector<std::vector<fe25519>> a, b;
    std::vector<std::vector<ge25519>> L, R;
    Proofs(size_t c, size_t abl, size_t Lr, size_t n) : rp(c), V(c), a(c), b(c), L(c), R(c) {
        for (size_t k = 0; k < c; k++) {
            fill(&rp[k], sizeof(RangeProof));
            fill(&V[k], sizeof(ge25519));
            a[k].resize(abl); b[k].resize(abl); L[k].resize(Lr); R[k].resize(Lr);
            fill(a[k].data(), abl * 32); fill(b[k].data(), abl * 32);
            fill(L[k].data(), Lr * 128); fill(R[k].data(), Lr * 128);
            InnerProductProof& ip = rp[k].ip_proof;
            ip.n = n;
            ip.a = FieldVector{a[k].data(), abl};
            ip.b = FieldVector{b[k].data(), abl};
            ip.L = PointVector{Lr ? L[k].data() : nullptr, Lr};
            ip.R = PointVector{Lr ? R[k].data() : nullptr, Lr};
            ip.L_len = Lr;
        }
    }
};

static void pack_view() {
    const size_t cs[] = {1, 2, 3, 5}, abls[] = {1, 2, 3}, Lrs[] = {0, 1, 6};
    for (size_t c : cs)
        for (size_t abl : abls)
            for (size_t Lr : Lrs)
                for (int range = 1; range >= 0; range--) {   // 0: the inner-product-only staging (no RangeProof, no V)
                    const Proofs P(c, abl, Lr, (size_t)1 << Lr);
                    const bp::ChunkLayout l{c, abl, Lr};
                    std::vector<uint8_t> buf(l.bytes(), 0xAA);   // exactly the chunk: an overrun is the sanitizer's
                    for (size_t k = 0; k < c; k++)
                        l.pack(buf.data(), k, P.rp[k].ip_proof, range ? &P.rp[k] : nullptr, range ? &P.V[k] : nullptr);
                    hipbp_proof_batch b;
                    l.view(buf.data(), &b);
                    for (size_t k = 0; k < c; k++) {
                        const RangeProof& p = P.rp[k];
                        if (range) {
                            CHECK(same(b.V[k], P.V[k]) && same(b.A[k], p.A) && same(b.S[k], p.S) && same(b.T1[k], p.T1) &&
                                  same(b.T2[k], p.T2) && same(b.t[k], p.t), "range fields of proof %zu", k);
                        } else {
                            CHECK(all_zero(&b.V[k], 128) && all_zero(&b.A[k], 128) && all_zero(&b.S[k], 128) &&
                                  all_zero(&b.T1[k], 128) && all_zero(&b.T2[k], 128) && all_zero(&b.t[k], 32),
                                  "absent range fields of proof %zu must be zero", k);
                        }
                        CHECK(same(b.c[k], p.ip_proof.c) && same(b.x[k], p.ip_proof.x), "c, x of proof %zu", k);
                        for (size_t j = 0; j < abl; j++)
                            CHECK(same(b.a[k * abl + j], P.a[k][j]) && same(b.b[k * abl + j], P.b[k][j]), "a, b of proof %zu", k);
                        for (size_t j = 0; j < Lr; j++)
                            CHECK(same(b.L[k * Lr + j], P.L[k][j]) && same(b.R[k * Lr + j], P.R[k][j]), "L, R of proof %zu", k);
                    }
                }
}

static void unpack() {
    const size_t shapes[][3] = {{4, 4, 3}, {5, 3, 3}, {3, 3, 0}, {4, 2, 0}, {2, 1, 6}, {16, 7, 1}};   // cap, c, Lr
    for (auto& sh : shapes)
        for (int with_lead = 0; with_lead < 2; with_lead++) {
            const size_t cap = sh[0], c = sh[1], Lr = sh[2], n = (size_t)1 << Lr;
            const bp::OutLayout l{cap, c, Lr, with_lead ? 2 * cap * 32 : 0};
            std::vector<uint8_t> buf(l.slot_bytes(), 0xAA);
            hipbp_proof_out o;
            l.view(buf.data(), &o);
            // the source pattern, proof by proof, written through the view
            const Proofs P(c, 1, Lr, n);
            std::vector<fe25519> a(c), b(c);
            for (size_t k = 0; k < c; k++) {
                const RangeProof& p = P.rp[k];
                o.V[k] = p.V; o.A[k] = p.A; o.S[k] = p.S; o.T1[k] = p.T1; o.T2[k] = p.T2;
                o.taux[k] = p.taux; o.mu[k] = p.mu; o.t[k] = p.t; o.c[k] = p.ip_proof.c; o.x[k] = p.ip_proof.x;
                o.a[k] = P.a[k][0]; o.b[k] = P.b[k][0];
                for (size_t j = 0; j < Lr; j++) { o.L[k * Lr + j] = P.L[k][j]; o.R[k * Lr + j] = P.R[k][j]; }
                o.valid[k] = k % 3 != 1;   // proofs 1, 4, .. are refused
            }
            for (size_t k = 0; k < c; k++) {
                const RangeProof& p = P.rp[k];
                RangeProof got;
                memset(&got, 0xFF, sizeof got);
                const int v = l.unpack(buf.data(), k, n, got);
                CHECK(v == (k % 3 != 1 ? 1 : 0), "unpack verdict of proof %zu: %d", k, v);
                CHECK(same(got.V, p.V) && same(got.A, p.A) && same(got.S, p.S) && same(got.T1, p.T1) && same(got.T2, p.T2) &&
                      same(got.taux, p.taux) && same(got.mu, p.mu) && same(got.t, p.t), "head of proof %zu", k);
                const InnerProductProof& ip = got.ip_proof;
                if (v != 1) {
                    CHECK(all_zero(&ip, sizeof ip), "a refused proof's ip_proof must be all zero");
                    continue;
                }
                CHECK(ip.n == n && ip.a.length == 1 && ip.b.length == 1 && ip.L.length == Lr && ip.R.length == Lr &&
                      ip.L_len == Lr, "lengths of proof %zu", k);
                CHECK(ip.a.elements && ip.b.elements && ip.L.elements && ip.R.elements, "vectors of proof %zu", k);
                CHECK(same(ip.c, p.ip_proof.c) && same(ip.x, p.ip_proof.x) && same(*ip.a.elements, P.a[k][0]) &&
                      same(*ip.b.elements, P.b[k][0]), "c, x, a, b of proof %zu", k);
                for (size_t j = 0; j < Lr; j++)
                    CHECK(same(ip.L.elements[j], P.L[k][j]) && same(ip.R.elements[j], P.R[k][j]), "L, R of proof %zu", k);
                free(ip.a.elements); free(ip.b.elements); free(ip.L.elements); free(ip.R.elements);
            }
        }
}

template <size_t N>
static void check_table(const char* what, const size_t (&got)[N], const std::vector<size_t>& want, size_t want_sum) {
    CHECK(want.size() == N, "%s: %zu buffers, want %zu", what, N, want.size());
    size_t sum = 0;
    for (size_t i = 0; i < N && i < want.size(); i++) {
        CHECK(got[i] == want[i], "%s buffer %zu: %zu bytes, want %zu", what, i, got[i], want[i]);
        sum += got[i];
    }
    CHECK(sum == want_sum, "%s: %zu bytes in all, want %zu", what, sum, want_sum);
}

static void tables() {
    using namespace bp;
    const size_t bins = MSM_BINS;
    const size_t Bn[][2] = {{1, 1}, {3, 8}, {5, 64}, {2, 128}, {2, 4096}};
    for (auto& bn : Bn) {
        const size_t B = bn[0], n = bn[1];
        for (int sort = 0; sort < 2 && n <= 128; sort++) {
            const size_t cap = B * (4 * n + 4);
            size_t sz[PB_COUNT];
            prove_sizes(B, n, sort != 0, sz);
            CHECK(prove_cap(B, n) == cap, "prover cap");
            // by name, then the whole table in the order of the issue's list
            CHECK(sz[PB_PS] == B * 4 * n * 32 && sz[PB_PTERM] == cap * 128 && sz[PB_CHAIN] == B * 4 * 128 &&
                  sz[PB_PTS] == B * 5 * 128 && sz[PB_ST] == B * 8 * 32 && sz[PB_TSC] == B * 4 * 32 && sz[PB_TT] == B * 4 * 128 &&
                  sz[PB_ACUR] == B * n * 32 && sz[PB_BCUR] == B * n * 32 && sz[PB_ISCAL] == B * 2 * n * 32 &&
                  sz[PB_CSC] == B * 2 * 32 && sz[PB_ITERM] == B * (2 * n + 2) * 128 && sz[PB_MISC] == B * 4 * 32 &&
                  sz[PB_VALID] == B && sz[PB_LIST] == 2 * cap * 4 && sz[PB_CNT] == 8 && sz[PB_CTAB] == 2 * n * 128 &&
                  sz[PB_SLIST] == (sort ? cap * 4 : 0) && sz[PB_SBINS] == (sort ? bins * 4 : 0), "prover buffers by name");
            const size_t sum = B * (8 * n + 18) * 32 + (cap + B * (2 * n + 15) + 2 * n) * 128 + B + 2 * cap * 4 + 8 +
                               (sort ? cap * 4 + bins * 4 : 0);
            check_table("prover", sz,
                        {B * 4 * n * 32, cap * 128, B * 4 * 128, B * 5 * 128, B * 8 * 32, B * 4 * 32, B * 4 * 128, B * n * 32,
                         B * n * 32, B * 2 * n * 32, B * 2 * 32, B * (2 * n + 2) * 128, B * 4 * 32, B, 2 * cap * 4, 8,
                         2 * n * 128, sort ? cap * 4 : 0, sort ? bins * 4 : 0}, sum);
        }
        {   // the IPA chunk (here B is Bc)
            const size_t cap = 2 * n + 2, per_proof = (5 * n + 6) * 32 + (2 * n + 6) * 128 + 2 * cap * 4;
            size_t sz[IB_COUNT];
            ipa_sizes(B, n, sz);
            CHECK(ipa_cap(n) == cap && ipa_per_proof(n) == per_proof, "ipa cap / per_proof");
            CHECK(sz[IB_A] == B * n * 32 && sz[IB_B] == B * n * 32 && sz[IB_PROD] == B * n * 32 && sz[IB_SC] == B * 2 * n * 32 &&
                  sz[IB_CSC] == B * 2 * 32 && sz[IB_TERM] == B * 2 * n * 128 && sz[IB_CQ] == B * 2 * 128 &&
                  sz[IB_CHAIN] == B * 4 * 128 && sz[IB_TR] == B * 32 && sz[IB_UU] == B * 2 * 32 && sz[IB_X] == B * 32 &&
                  sz[IB_SLIST] == B * cap * 4 && sz[IB_LLIST] == B * cap * 4 && sz[IB_CTL] == (bins + 2) * 4,
                  "ipa buffers by name");
            check_table("ipa", sz,
                        {B * n * 32, B * n * 32, B * n * 32, B * 2 * n * 32, B * 2 * 32, B * 2 * n * 128, B * 2 * 128, B * 4 * 128,
                         B * 32, B * 2 * 32, B * 32, B * cap * 4, B * cap * 4, (bins + 2) * 4}, B * per_proof + (bins + 2) * 4);
        }
        for (int mode = 0; mode < 3; mode++)
            for (size_t Lb : {(size_t)0, (size_t)3}) {
                const size_t Lc = Lb ? Lb : 1, m2 = mode == 2 ? B : 0;
                size_t sz[B_COUNT];
                verify_sizes(B, n, Lb, mode, sz);
                CHECK(sz[B_SG] == B * 32 && sz[B_SH] == B * n * 32 && sz[B_SC] == B * 4 * 32 && sz[B_U] == B * Lc * 32 &&
                      sz[B_UINV] == B * Lc * 32 && sz[B_IPOK] == B && sz[B_MSM_PTS] == B * 2 * n * 128 &&
                      sz[B_MSM_PART] == B * 2 * 128 && sz[B_TERMS] == B * 4 * 128 && sz[B_FOLD0] == B * 2 * n * 128 &&
                      sz[B_FOLD1] == B * 2 * n * 128 && sz[B_FIN] == B * 2 * 128 && sz[B_PIN] == B * 128 &&
                      sz[B_PSC] == m2 * 8 * 32 && sz[B_PTERM] == m2 * 8 * 128 && sz[B_LR] == m2 * 2 * 128 && sz[B_CHAL] == m2 * 32 &&
                      sz[B_M3] == m2 * 2 * 128 && sz[B_RFLAGS] == m2 && sz[B_PBASE] == m2 * 3 * 128 && sz[B_PERM] == 0,
                      "verify buffers by name, mode %d", mode);
                size_t sum = 0;
                for (size_t s : sz) sum += s;
                CHECK(sum == B * ((5 + n + 2 * Lc) * 32 + 1 + (6 * n + 9) * 128) + m2 * (9 * 32 + 15 * 128 + 1),
                      "verify slot: %zu bytes in all, mode %d", sum, mode);
            }
    }
    const size_t nc[][2] = {{1, 1}, {300, 1}, {256, 3}, {257, 2}, {4096, 5}};
    for (auto& x : nc) {
        const size_t n = x[0], count = x[1], tot = n * count, nb = count * ((n + 255) / 256);
        size_t sz[MB_COUNT];
        msm_sizes(n, count, sz);
        CHECK(sz[MB_TERMS] == tot * 128 && sz[MB_ROOT0] == nb * 128 && sz[MB_ROOT1] == nb * 128 && sz[MB_TREE0] == 0 &&
              sz[MB_TREE1] == 0 && sz[MB_ORDER] == tot * 4 && sz[MB_BINS] == bins * 4, "msm buffers by name");
        check_table("msm", sz, {tot * 128, nb * 128, nb * 128, 0, 0, tot * 4, bins * 4}, tot * 132 + nb * 256 + bins * 4);
        tree_sizes(n, sz);
        const size_t tb = (n + 255) / 256 * 128;
        check_table("tree", sz, {0, 0, 0, tb, tb, 0, 0}, 2 * tb);
    }
}

// The Pippenger part: every shape field and every buffer's bytes against the expressions
// bp_pippenger.hip computed in line before it had a table (256 threads per block, 16 buckets per
// chunk, 4 x 256 buckets per scan block, 4096 list elements per bidfill piece), over
// n x c x count x {all windows, the first, the top part [wm, W)} x key width x tail layer.
static void pippenger() {
    using namespace bp;
    const size_t ns[] = {1, 3, 4, 63, 64, 1000, 3000, 65536, (size_t)1 << 20}, counts[] = {1, 3};
    const int cs[] = {4, 8, 12}, tls[] = {1, 4, 8};
    bool seen_k32[2] = {}, seen_TT[2] = {}, seen_odd = false, seen_sparse = false, seen_nbq1 = false;
    for (size_t n : ns)
        for (int c : cs)
            for (size_t count : counts)
                for (int range = 0; range < 3; range++)
                    for (int force16 = 0; force16 < 2; force16++)
                        for (int tl : tls) {
                            const int Wt = (256 + c - 1) / c, wm = (Wt * 3) / 8 > 0 ? (Wt * 3) / 8 : 1;
                            const int w0 = range == 2 ? wm : 0, w1 = range == 1 ? 1 : Wt;
                            const size_t Wtot = range == 2 ? Wt : 0, temp = 1000 + n;   // (any byte count)
                            // the old expressions
                            const int Wp = w1 - w0;
                            const size_t W = (size_t)Wp * count;
                            const size_t NB = (size_t)1 << c, nb = W * NB, N = W * n, NC = NB / 16;
                            int ib = 0;
                            while (ib < 32 && ((size_t)1 << ib) < n) ib++;
                            const bool k32 = c + ib <= 32 && !force16;
                            int levels = 1;
                            while (levels < 31 && ((size_t)1 << levels) < n) levels++;
                            const int steps = (levels + 1) / 2, T = steps + 1;
                            const unsigned nparts = (unsigned)((nb + 1024 - 1) / 1024);
                            const size_t tot0 = N + 3 * nb, qcap = tot0 / 4 + 4 * nb;
                            const int TT = steps > tl ? tl : 0;
                            const size_t nbq = N / 4096 + 1;

                            const PipShape s = pip_shape(n, count, c, w0, w1, force16 != 0, tl);
                            CHECK(s.n == n && s.count == count && s.c == c && s.w0 == w0, "pip shape inputs");
                            CHECK(s.Wp == Wp, "pip Wp");
                            CHECK(s.W == W, "pip W");
                            CHECK(s.NB == NB, "pip NB");
                            CHECK(s.nb == nb, "pip nb");
                            CHECK(s.N == N, "pip N");
                            CHECK(s.NC == NC, "pip NC");
                            CHECK(s.ib == ib, "pip ib n=%zu", n);
                            CHECK(s.k32 == k32, "pip k32");
                            CHECK(s.levels == levels, "pip levels n=%zu", n);
                            CHECK(s.steps == steps, "pip steps");
                            CHECK(s.T == T, "pip T");
                            CHECK(s.nparts == nparts, "pip nparts");
                            CHECK(s.tot0 == tot0, "pip tot0");
                            CHECK(s.qcap == qcap, "pip qcap");
                            CHECK(s.nbq == nbq, "pip nbq");
                            CHECK(s.TT == TT, "pip TT");
                            size_t sz[PIP_COUNT];
                            pip_sizes(s, Wtot, temp, sz);
                            const size_t kb = N * (k32 ? 4 : 2);
                            CHECK(sz[PIP_KEYS_IN] == kb && sz[PIP_KEYS] == kb && sz[PIP_VALS] == (k32 ? 0 : N * 4) &&
                                  sz[PIP_START] == nb * 4 && sz[PIP_LEN0] == nb * 4 && sz[PIP_LEN1] == nb * 4 &&
                                  sz[PIP_LAY] == (size_t)3 * (T + 1) * nb * 4 && sz[PIP_PART] == (size_t)(T + 1) * nparts * 4 &&
                                  sz[PIP_BID0] == tot0 * 4 && sz[PIP_BID1] == qcap * 4 && sz[PIP_Q0] == qcap * 128 &&
                                  sz[PIP_Q1] == qcap * 128 && sz[PIP_V] == W * NC * 128 && sz[PIP_S] == nb * 128 &&
                                  sz[PIP_MAXLEN] == 12 && sz[PIP_TAILQ] == (TT ? nb * 4 : 0) && sz[PIP_BQ] == nbq * 8 &&
                                  sz[PIP_SW] == count * Wtot * 128 && sz[PIP_TMID] == (Wtot ? count * 128 : 0) &&
                                  sz[PIP_TEMP] == temp, "pip buffers by name n=%zu c=%d", n, c);
                            const size_t sum = 2 * kb + (k32 ? 0 : N * 4) + 3 * nb * 4 + 3 * (T + 1) * nb * 4 +
                                               (T + 1) * nparts * 4 + (tot0 + qcap) * 4 + (2 * qcap + W * NC + nb) * 128 + 12 +
                                               (TT ? nb * 4 : 0) + nbq * 8 + (Wtot ? count * (Wtot + 1) * 128 : 0) + temp;
                            check_table("pip", sz,
                                        {kb, kb, k32 ? 0 : N * 4, nb * 4, nb * 4, nb * 4, (size_t)3 * (T + 1) * nb * 4,
                                         (size_t)(T + 1) * nparts * 4, tot0 * 4, qcap * 4, qcap * 128, qcap * 128, W * NC * 128,
                                         nb * 128, 12, TT ? nb * 4 : 0, nbq * 8, count * Wtot * 128, Wtot ? count * 128 : 0,
                                         temp}, sum);
                            seen_k32[k32] = seen_TT[TT > 0] = true;
                            seen_odd |= n % 4 != 0;
                            seen_sparse |= n < NB / 4;
                            seen_nbq1 |= N / 4096 == 0;
                        }
    CHECK(seen_k32[0] && seen_k32[1], "pip grid: both key widths");
    CHECK(seen_TT[0] && seen_TT[1], "pip grid: with and without the LDS tail");
    CHECK(seen_odd && seen_sparse && seen_nbq1, "pip grid: n %% 4 != 0, n < 2^c / 4, N / BID_PIECE == 0");
}

// The generator view and its packed order: for n = 1, 2, 4 pack_gens followed by GenView::at gives the
// four inputs back; position k of the packed buffer is base k of the prefix-table order (G[0..n),
// H[0..n), h, g: launch_prefix_tables' bases, row 2n h's and row 2n + 1 g's); a view without g is the
// first 2n + 1 points; tab is null exactly when bits is 0.
static void gen_view() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)4}) {
        std::vector<ge25519> G(n), H(n);
        ge25519 g, h;
        fill(G.data(), n * 128); fill(H.data(), n * 128); fill(&g, 128); fill(&h, 128);
        CHECK(bp::gens_bytes(n) == (2 * n + 2) * 128 && bp::gens_bytes(n, false) == (2 * n + 1) * 128, "gens_bytes n=%zu", n);
        std::vector<ge25519> buf(2 * n + 2);   // exactly the packed set: an overrun is the sanitizer's
        bp::pack_gens(buf.data(), G.data(), H.data(), &g, &h, n);
        const bp::GenView v = bp::GenView::at(buf.data(), n);
        CHECK(v.n == n && v.tab == nullptr && v.bits == 0, "view header n=%zu", n);
        const ge25519 *vG = (const ge25519*)v.G, *vH = (const ge25519*)v.H;
        for (size_t i = 0; i < n; i++) CHECK(same(vG[i], G[i]) && same(vH[i], H[i]), "G, H [%zu] n=%zu", i, n);
        CHECK(same(*(const ge25519*)v.g, g) && same(*(const ge25519*)v.h, h), "g, h n=%zu", n);
        // the table base order, by position
        for (size_t k = 0; k < 2 * n + 2; k++) {
            const ge25519& want = k < n ? G[k] : k < 2 * n ? H[k - n] : k == 2 * n ? h : g;
            CHECK(same(buf[k], want), "packed position %zu n=%zu", k, n);
        }
        CHECK((const void*)v.G == &buf[0] && (const void*)v.H == &buf[n] && (const void*)v.h == &buf[2 * n] &&
              (const void*)v.g == &buf[2 * n + 1], "view pointers n=%zu", n);
        CHECK(bp::packed_gens_equal(buf.data(), G.data(), H.data(), &h, n), "packed_gens_equal on its own bytes");
        ge25519 h2 = h;
        ((uint8_t*)&h2)[127] ^= 1;
        CHECK(!bp::packed_gens_equal(buf.data(), G.data(), H.data(), &h2, n), "packed_gens_equal sees h's last byte");
        // without g: 2n + 1 points, g's slot untouched, the view's g null
        std::vector<ge25519> buf1(2 * n + 1);
        bp::pack_gens(buf1.data(), G.data(), H.data(), nullptr, &h, n);
        CHECK(memcmp(buf1.data(), buf.data(), (2 * n + 1) * 128) == 0, "pack without g n=%zu", n);
        const bp::GenView v1 = bp::GenView::at(buf1.data(), n, false);
        CHECK(v1.g == nullptr && (const void*)v1.h == &buf1[2 * n] && v1.without_g().g == nullptr && v.without_g().g == nullptr &&
              v.without_g().h == v.h, "view without g n=%zu", n);
        // tables: null exactly when bits == 0, whatever is passed
        const bp::ge* t = (const bp::ge*)buf.data();
        const bp::GenView w4 = v.with_tables(t, 4), w0 = v.with_tables(t, 0), wn = v.with_tables(nullptr, 4);
        CHECK(w4.tab == t && w4.bits == 4 && w4.G == v.G && w4.g == v.g && w4.n == n, "with_tables(t, 4)");
        CHECK(w0.tab == nullptr && w0.bits == 0, "bits == 0 must give a null table");
        CHECK(wn.tab == nullptr && wn.bits == 0, "a null table must give bits == 0");
        CHECK(w4.with_tables(nullptr, 0).tab == nullptr && w4.with_tables(nullptr, 0).bits == 0, "tables taken off");
        const bp::GenView loose(G.data(), H.data(), &g, &h);   // four loose pointers: no tables, no n
        CHECK((const void*)loose.G == G.data() && (const void*)loose.H == H.data() && (const void*)loose.g == &g &&
              (const void*)loose.h == &h && loose.tab == nullptr && loose.bits == 0 && loose.n == 0, "loose view");
    }
}

int main() {
    gen_view();
    offsets();
    pack_view();
    unpack();
    tables();
    pippenger();
    std::printf("%llu %llu\n", checks, fails);
    return fails ? 1 : 0;
}

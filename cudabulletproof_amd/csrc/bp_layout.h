// bp_layout.h — the flat batch layouts and the engine's workspace tables (internal to the library).
// Host-only and pure: no HIP runtime calls, so tests/layout_check.hip checks every offset, the
// pack / view / unpack round trips and every buffer size on a CPU.
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../include/cudabulletproof_hip.h"
#include "bp_kernels.h"

namespace bp {

constexpr size_t FE = 32, GE = 128;   // sizeof(fe25519), sizeof(ge25519)
static_assert(sizeof(fe25519) == FE && sizeof(ge25519) == GE, "wire record sizes");

// ------------------------------------------------------------------ verify chunk
// c proofs of one (ab_len, L_len) shape in the flat wire format, no padding:
//   V A S T1 T2 [c] | t c x [c] | a b [c abl] | L R [c Lr]
// The same bytes in pinned host memory (pack) and in device memory (view).
struct ChunkLayout {
    size_t c, abl, Lr;
    size_t o_fe() const { return 5 * c * GE; }
    size_t o_ab() const { return o_fe() + 3 * c * FE; }
    size_t o_lr() const { return o_ab() + 2 * c * abl * FE; }
    size_t bytes() const { return o_lr() + 2 * c * Lr * GE; }
    // count, ab_len, L_len and the twelve pointers of `b` over the chunk at `base` (n, taux, mu, Vp
    // are the caller's)
    void view(const void* base, hipbp_proof_batch* b) const {
        const uint8_t* q = (const uint8_t*)base;
        const ge25519* pt = (const ge25519*)q;
        const fe25519* f = (const fe25519*)(q + o_fe());
        const fe25519* ab = (const fe25519*)(q + o_ab());
        const ge25519* lr = (const ge25519*)(q + o_lr());
        b->count = c; b->ab_len = abl; b->L_len = Lr;
        b->V = pt; b->A = pt + c; b->S = pt + 2 * c; b->T1 = pt + 3 * c; b->T2 = pt + 4 * c;
        b->t = f; b->c = f + c; b->x = f + 2 * c;
        b->a = ab; b->b = ab + c * abl;
        b->L = Lr ? lr : nullptr;
        b->R = Lr ? lr + c * Lr : nullptr;
    }
    // proof k of the chunk at `base` (host memory) from ip (a, b of abl elements, L, R of at least
    // Lr), the range proof's A S T1 T2 t and V; a missing rp or V is written as zeros
    void pack(void* base, size_t k, const InnerProductProof& ip, const RangeProof* rp, const ge25519* V) const {
        uint8_t* q = (uint8_t*)base;
        ge25519* pt = (ge25519*)q;
        fe25519* f = (fe25519*)(q + o_fe());
        fe25519* ab = (fe25519*)(q + o_ab());
        ge25519* lr = (ge25519*)(q + o_lr());
        const ge25519 zp = {};
        const fe25519 zf = {};
        pt[k] = V ? *V : zp;
        pt[c + k] = rp ? rp->A : zp;
        pt[2 * c + k] = rp ? rp->S : zp;
        pt[3 * c + k] = rp ? rp->T1 : zp;
        pt[4 * c + k] = rp ? rp->T2 : zp;
        f[k] = rp ? rp->t : zf;
        f[c + k] = ip.c;
        f[2 * c + k] = ip.x;
        auto put = [](void* dst, const void* src, size_t len) {   // (a null vector: zeros, too)
            if (src) memcpy(dst, src, len);
            else memset(dst, 0, len);
        };
        put(ab + k * abl, ip.a.elements, abl * FE);
        put(ab + (c + k) * abl, ip.b.elements, abl * FE);
        if (Lr) {
            put(lr + k * Lr, ip.L.elements, Lr * GE);
            put(lr + (c + k) * Lr, ip.R.elements, Lr * GE);
        }
    }
};

// ------------------------------------------------------------------ proof vectors
// A proof's a, b (length abl: 1 from the provers) and L, R (Lr points; 1 byte when Lr = 0) malloc'ed as the reference's
// inner_product_proof_init / field_vector_copy leave them, and n and the lengths set.  False: an
// allocation failed (what was allocated is in the proof, for the caller to free).  `alloc`: malloc,
// or what stands in for it in a CPU check.
typedef void* (*AllocFn)(size_t);
inline bool proof_vectors_alloc(InnerProductProof& ip, size_t n, size_t Lr, AllocFn alloc = malloc, size_t abl = 1) {
    ip.a.elements = (fe25519*)alloc(abl * FE);
    ip.b.elements = (fe25519*)alloc(abl * FE);
    ip.L.elements = (ge25519*)alloc(Lr ? Lr * GE : 1);
    ip.R.elements = (ge25519*)alloc(Lr ? Lr * GE : 1);
    ip.n = n;
    ip.a.length = ip.b.length = abl;
    ip.L.length = ip.R.length = ip.L_len = Lr;
    return ip.a.elements && ip.b.elements && ip.L.elements && ip.R.elements;
}

// ------------------------------------------------------------------ proof output
// The prover's outputs, after `lead` bytes of the owner's own (the prove-host slot's v | gamma):
//   V A S T1 T2 | taux mu t c x a b | L R | valid
// Every region is sized for cap proofs; the arrays of the c <= cap proofs present sit packed at
// stride c at the front of each (a short last chunk).
struct OutLayout {
    size_t cap, c, Lr, lead;
    size_t o_pts() const { return lead; }
    size_t o_fe() const { return o_pts() + 5 * cap * GE; }
    size_t o_lr() const { return o_fe() + 7 * cap * FE; }
    size_t o_valid() const { return o_lr() + 2 * cap * Lr * GE; }
    size_t end() const { return o_valid() + cap; }
    size_t slot_bytes() const { return (end() + 127) & ~(size_t)127; }
    size_t used() const { return o_valid() + c - o_pts(); }   // points .. valid[c): one D2H copy
    void view(void* base, hipbp_proof_out* o) const {
        uint8_t* q = (uint8_t*)base;
        ge25519* pt = (ge25519*)(q + o_pts());
        fe25519* f = (fe25519*)(q + o_fe());
        ge25519* lr = (ge25519*)(q + o_lr());
        o->V = pt; o->A = pt + c; o->S = pt + 2 * c; o->T1 = pt + 3 * c; o->T2 = pt + 4 * c;
        o->taux = f; o->mu = f + c; o->t = f + 2 * c; o->c = f + 3 * c; o->x = f + 4 * c;
        o->a = f + 5 * c; o->b = f + 6 * c;
        o->L = Lr ? lr : nullptr;
        o->R = Lr ? lr + c * Lr : nullptr;
        o->valid = q + o_valid();
    }
    // Proof k of a host copy into p (n = 1 << Lr): 1 a valid proof, its vectors malloc'ed; 0 a refused
    // one (the five points and taux, mu, t; ip_proof all zero); -1 an allocation failed (p owns what
    // was allocated)
    int unpack(const void* base, size_t k, size_t n, RangeProof& p, AllocFn alloc = malloc) const {
        hipbp_proof_out o;
        view(const_cast<void*>(base), &o);   // (read only)
        p.V = o.V[k]; p.A = o.A[k]; p.S = o.S[k]; p.T1 = o.T1[k]; p.T2 = o.T2[k];
        p.taux = o.taux[k]; p.mu = o.mu[k]; p.t = o.t[k];
        InnerProductProof& ip = p.ip_proof;
        memset(&ip, 0, sizeof ip);
        if (!o.valid[k]) return 0;
        if (!proof_vectors_alloc(ip, n, Lr, alloc)) return -1;
        ip.c = o.c[k]; ip.x = o.x[k];
        *ip.a.elements = o.a[k]; *ip.b.elements = o.b[k];
        if (Lr) {
            memcpy(ip.L.elements, o.L + k * Lr, Lr * GE);
            memcpy(ip.R.elements, o.R + k * Lr, Lr * GE);
        }
        return 1;
    }
};

// The prover's outputs as its kernels take them, and as the batch a verifier reads: `count` proofs of
// n bits and Lr fold rounds, a and b of one element (Vp stays null: V is the proofs' own).
inline ProveOut prove_out_of(const hipbp_proof_out& o) {
    return ProveOut{(ge*)o.V, (ge*)o.A, (ge*)o.S, (ge*)o.T1, (ge*)o.T2, (fe*)o.taux, (fe*)o.mu, (fe*)o.t,
                    (fe*)o.c, (fe*)o.x, (fe*)o.a, (fe*)o.b, (ge*)o.L, (ge*)o.R, o.valid};
}
inline hipbp_proof_batch batch_of(const hipbp_proof_out& o, size_t count, size_t n, size_t Lr) {
    hipbp_proof_batch b{};
    b.count = count; b.n = n; b.ab_len = 1; b.L_len = Lr;
    b.V = o.V; b.A = o.A; b.S = o.S; b.T1 = o.T1; b.T2 = o.T2;
    b.t = o.t; b.a = o.a; b.b = o.b; b.c = o.c; b.x = o.x; b.L = o.L; b.R = o.R;
    b.taux = o.taux; b.mu = o.mu;
    return b;
}

// ------------------------------------------------------------------ generators
// A generator set as the library's functions hand it on: G[n], H[n], g, h and, optionally, their
// fixed-base prefix tables (launch_prefix_tables) of `bits` bits.  tab is null exactly when bits is
// 0: with_tables is the one way to set them and keeps that, so a consumer reads either as it is.
// g may be null where the semantics do not read it.  Packed, on the host (pack_gens) and on the
// device (at), the 2n + 2 points lie in the tables' base order
//   G[n] | H[n] | h | g
// so position k of a packed buffer is base k of its tables, and a set without g is its first 2n + 1.
inline size_t gens_bytes(size_t n, bool with_g = true) { return (2 * n + (with_g ? 2 : 1)) * GE; }
struct GenView {
    const ge *G = nullptr, *H = nullptr, *g = nullptr, *h = nullptr;
    const ge* tab = nullptr;
    int bits = 0;
    size_t n = 0;   // 0: loose bases (no G, H, or a caller that brings n itself)
    GenView() = default;
    GenView(const void* G_, const void* H_, const void* g_, const void* h_, size_t n_ = 0)
        : G((const ge*)G_), H((const ge*)H_), g((const ge*)g_), h((const ge*)h_), n(n_) {}
    static GenView at(const void* base, size_t n, bool with_g = true) {
        const uint8_t* q = (const uint8_t*)base;
        return GenView(q, q + n * GE, with_g ? q + (2 * n + 1) * GE : nullptr, q + 2 * n * GE, n);
    }
    GenView with_tables(const void* t, int k) const {
        GenView v = *this;
        const bool on = t && k > 0;
        v.tab = on ? (const ge*)t : nullptr;
        v.bits = on ? k : 0;
        return v;
    }
    GenView without_g() const {
        GenView v = *this;
        v.g = nullptr;
        return v;
    }
};
// the packed order from four host arrays (g null: its slot is left as it is) ...
inline void pack_gens(void* dst, const void* G, const void* H, const void* g, const void* h, size_t n) {
    uint8_t* q = (uint8_t*)dst;
    memcpy(q, G, n * GE);
    memcpy(q + n * GE, H, n * GE);
    memcpy(q + 2 * n * GE, h, GE);
    if (g) memcpy(q + (2 * n + 1) * GE, g, GE);
}
// ... and whether a packed G | H | h holds exactly these bytes
inline bool packed_gens_equal(const void* packed, const void* G, const void* H, const void* h, size_t n) {
    const uint8_t* q = (const uint8_t*)packed;
    return memcmp(q, G, n * GE) == 0 && memcmp(q + n * GE, H, n * GE) == 0 && memcmp(q + 2 * n * GE, h, GE) == 0;
}

// ------------------------------------------------------------------ workspace tables
// One line per device buffer: X(id, field, type, bytes) — the engine's buffer `id` backs `field`, a
// type*, of the workspace struct the kernels take, and holds `bytes` bytes.  The engine keeps one
// grow-only allocation per id (0 bytes: not needed by this call, left as it is) and fills the
// struct from the same table, BP_BUF_FIELD with the struct as `w` and the buffers as `b`.
#define BP_BUF_ID(id, field, type, bytes) id,
#define BP_BUF_SIZE(id, field, type, bytes) sz[id] = (bytes);
#define BP_BUF_FIELD(id, field, type, bytes) w.field = (type*)b[id].p;
constexpr size_t U32 = sizeof(uint32_t);

// The prover (ProveWs) for B proofs of n bits; cap = B (4n + 4), its term items.  slist, sbins: with
// terms0's heavy-list sort only.
#define BP_PROVE_BUFS(X)                               \
    X(PB_PS, ps, fe, B * 4 * n * FE)                   \
    X(PB_PTERM, pterm, ge, cap * GE)                   \
    X(PB_CHAIN, chain, ge, B * 4 * GE)                 \
    X(PB_PTS, pts, ge, B * 5 * GE)                     \
    X(PB_ST, st, fe, B * 8 * FE)                       \
    X(PB_TSC, tsc, fe, B * 4 * FE)                     \
    X(PB_TT, tt, ge, B * 4 * GE)                       \
    X(PB_ACUR, acur, fe, B * n * FE)                   \
    X(PB_BCUR, bcur, fe, B * n * FE)                   \
    X(PB_ISCAL, iscal, fe, B * 2 * n * FE)             \
    X(PB_CSC, csc, fe, B * 2 * FE)                     \
    X(PB_ITERM, iterm, ge, B * (2 * n + 2) * GE)       \
    X(PB_MISC, misc, fe, B * 4 * FE)                   \
    X(PB_VALID, valid, uint8_t, B)                     \
    X(PB_LIST, list, uint32_t, 2 * cap * U32)          \
    X(PB_CNT, cnt, unsigned, 2 * U32)                  \
    X(PB_CTAB, ctab, ge, 2 * n * GE)                   \
    X(PB_SLIST, slist, uint32_t, sort ? cap * U32 : 0) \
    X(PB_SBINS, sbins, unsigned, sort ? MSM_BINS * U32 : 0)
enum ProveBuf { BP_PROVE_BUFS(BP_BUF_ID) PB_COUNT };
inline size_t prove_cap(size_t B, size_t n) { return B * (4 * n + 4); }
inline void prove_sizes(size_t B, size_t n, bool sort, size_t (&sz)[PB_COUNT]) {
    const size_t cap = prove_cap(B, n);
    BP_PROVE_BUFS(BP_BUF_SIZE)
}

// The accepted prover's retry loop (AcceptWs; n bits, Lr fold rounds), sized at two moments of a
// round: before its verify for the m proofs it verifies (ok, blk, cnt; r = 0), and after the host
// has read back the r of them the verifier rejected (m = 0) for what the next round's r proofs
// need: both index lists (the round reads one and writes the other), their v, gamma, try keys and
// scalars (rnd | sL | sR, the seeded prover's order), and their proofs as an OutLayout of r.
// Within a call r only shrinks, so a list that a round still reads is never regrown under it.
#define BP_ACCEPT_BUFS(X)                                     \
    X(AB_OK, ok, uint8_t, m)                                  \
    X(AB_BLK, blk, uint32_t, accept_blocks(m) * U32)          \
    X(AB_CNT, cnt, uint32_t, U32)                             \
    X(AB_LIST0, list[0], uint32_t, r * U32)                   \
    X(AB_LIST1, list[1], uint32_t, r * U32)                   \
    X(AB_V, v, fe, r * FE)                                    \
    X(AB_GAMMA, gamma, fe, r * FE)                            \
    X(AB_KEYS, keys, fe, r * FE)                              \
    X(AB_SCAL, scal, fe, r * (2 * n + 4) * FE)                \
    X(AB_OUT, out, uint8_t, r ? accept_out(r, Lr).slot_bytes() : 0)
enum AcceptBuf { BP_ACCEPT_BUFS(BP_BUF_ID) AB_COUNT };
inline size_t accept_blocks(size_t m) { return (m + 255) / 256; }   // k_accept_count's blocks (ACCEPT_BLK)
inline OutLayout accept_out(size_t r, size_t Lr) { return OutLayout{r, r, Lr, 0}; }
inline void accept_sizes(size_t m, size_t r, size_t n, size_t Lr, size_t (&sz)[AB_COUNT]) {
    BP_ACCEPT_BUFS(BP_BUF_SIZE)
}

// One chunk of the stand-alone IPA prover (IpaWs): Bc proofs of n elements, cap = 2n + 2 items each.
#define BP_IPA_BUFS(X)                            \
    X(IB_A, a, fe, Bc * n * FE)                   \
    X(IB_B, b, fe, Bc * n * FE)                   \
    X(IB_PROD, prod, fe, Bc * n * FE)             \
    X(IB_SC, sc, fe, Bc * 2 * n * FE)             \
    X(IB_CSC, csc, fe, Bc * 2 * FE)               \
    X(IB_TERM, term, ge, Bc * 2 * n * GE)         \
    X(IB_CQ, cq, ge, Bc * 2 * GE)                 \
    X(IB_CHAIN, chain, ge, Bc * 4 * GE)           \
    X(IB_TR, tr, fe, Bc * FE)                     \
    X(IB_UU, uu, fe, Bc * 2 * FE)                 \
    X(IB_X, x, fe, Bc * FE)                       \
    X(IB_SLIST, slist, uint32_t, Bc * cap * U32)  \
    X(IB_LLIST, llist, uint32_t, Bc * cap * U32)  \
    X(IB_CTL, ctl, unsigned, (MSM_BINS + 2) * U32)
enum IpaBuf { BP_IPA_BUFS(BP_BUF_ID) IB_COUNT };
inline size_t ipa_cap(size_t n) { return 2 * n + 2; }
// the bytes one more proof adds to a chunk (everything but ctl): the chunking rule's unit
inline size_t ipa_per_proof(size_t n) { return (5 * n + 6) * FE + (2 * n + 6) * GE + 2 * ipa_cap(n) * U32; }
inline void ipa_sizes(size_t Bc, size_t n, size_t (&sz)[IB_COUNT]) {
    const size_t cap = ipa_cap(n);
    BP_IPA_BUFS(BP_BUF_SIZE)
}

// One chunk of Pedersen commitments (CommitWs): c commitments, two scalar-mult terms each.  order,
// bins: with the chain-length sort only (HIPBP_COMMIT_SORT).
#define BP_COMMIT_BUFS(X)                                  \
    X(CB_TERMS, terms, ge, 2 * c * GE)                     \
    X(CB_ORDER, order, uint32_t, sort ? 2 * c * U32 : 0)   \
    X(CB_BINS, bins, unsigned, sort ? 2 * MSM_BINS * U32 : 0)
enum CommitBuf { BP_COMMIT_BUFS(BP_BUF_ID) CB_COUNT };
constexpr size_t COMMIT_CHUNK = (size_t)1 << 20;       // HIPBP_COMMIT_CHUNK's default: 256 MB of terms
constexpr size_t COMMIT_CHUNK_MAX = (size_t)1 << 24;   // ... and its limit (the grid stays under 2^31 lanes)
// HIPBP_COMMIT_SORT unset: chunks of at least this many commitments are sorted (MSM_SORT_MIN's rule: below
// it the waves all run at once and the order cannot shorten the launch, while the sort's five small
// launches add ~0.25 ms to a 1.6 ms call); 1: every chunk; 0: none
constexpr size_t COMMIT_SORT_MIN = 4096;
inline bool commit_sorted(size_t chunk, const char* env) { return env ? atoi(env) != 0 : chunk >= COMMIT_SORT_MIN; }
inline void commit_sizes(size_t c, bool sort, size_t (&sz)[CB_COUNT]) {
    BP_COMMIT_BUFS(BP_BUF_SIZE)
}
// The chunk a call of `count` commitments runs in: `env` is HIPBP_COMMIT_CHUNK's value (0: unset or
// not positive), clamped to COMMIT_CHUNK_MAX, and never more than count itself.
inline size_t commit_chunk(size_t count, long long env) {
    size_t ch = env > 0 ? (size_t)env : COMMIT_CHUNK;
    if (ch > COMMIT_CHUNK_MAX) ch = COMMIT_CHUNK_MAX;
    return count < ch ? count : ch;
}

// The proof blob encoder (CodecWs, bp_codec.h) for `count` proofs: one raw count per block of 256
// proofs, and the total after them.
#define BP_CODEC_BUFS(X) X(CDB_BLK, blk, uint32_t, (codec_blocks(count) + 1) * U32)
enum CodecBuf { BP_CODEC_BUFS(BP_BUF_ID) CDB_COUNT };
inline size_t codec_blocks(size_t count) { return (count + 255) / 256; }
inline void codec_sizes(size_t count, size_t (&sz)[CDB_COUNT]) {
    BP_CODEC_BUFS(BP_BUF_SIZE)
}

// Proof ids and Merkle roots (IdsWs, bp_ids.h).  A root over `leaves` ids goes level by level through
// two buffers: level 1 (and 3, 5, ...: each smaller) in ping, level 2 (4, ...) in pong, 32 bytes a
// node; the last level is written to the caller's root.  bad: one count of failed records per block
// of 256 proofs of a blob of `count` proofs.
inline size_t merkle_level_nodes(size_t leaves, int level) {
    for (int k = 0; k < level; k++) leaves = (leaves + 1) >> 1;
    return leaves;
}
#define BP_IDS_BUFS(X)                                            \
    X(IDB_PING, ping, uint8_t, merkle_level_nodes(leaves, 1) * 32) \
    X(IDB_PONG, pong, uint8_t, merkle_level_nodes(leaves, 2) * 32) \
    X(IDB_BAD, bad, uint32_t, codec_blocks(count) * U32)
enum IdsBuf { BP_IDS_BUFS(BP_BUF_ID) IDB_COUNT };
inline void ids_sizes(size_t leaves, size_t count, size_t (&sz)[IDB_COUNT]) {
    BP_IDS_BUFS(BP_BUF_SIZE)
}

// A verify slot (VerifyWs) for B proofs of n bits with Lb fold rounds; Lc = max(Lb, 1); m2 = B in mode 2
// (range_proof_verify), whose buffers the other modes leave unallocated.  B_PERM, the lane orders,
// is no VerifyWs field: the batch's sort sets size it.
#define BP_VERIFY_BUFS(X)                         \
    X(B_SG, sG, fe, B * FE)                       \
    X(B_SH, sH, fe, B * n * FE)                   \
    X(B_SC, sc, fe, B * 4 * FE)                   \
    X(B_U, u, fe, B * Lc * FE)                    \
    X(B_UINV, uinv, fe, B * Lc * FE)              \
    X(B_IPOK, ipok, uint8_t, B)                   \
    X(B_MSM_PTS, msm_pts, ge, B * 2 * n * GE)     \
    X(B_MSM_PART, msm_part, ge, B * 2 * GE)       \
    X(B_TERMS, terms, ge, B * 4 * GE)             \
    X(B_FOLD0, fold[0], ge, B * 2 * n * GE)       \
    X(B_FOLD1, fold[1], ge, B * 2 * n * GE)       \
    X(B_FIN, fin, ge, B * 2 * GE)                 \
    X(B_PIN, Pin, ge, B * GE)                     \
    X(B_PSC, psc, fe, m2 * 8 * FE)                \
    X(B_PTERM, pterm, ge, m2 * 8 * GE)            \
    X(B_LR, lr, ge, m2 * 2 * GE)                  \
    X(B_CHAL, chal, fe, m2 * FE)                  \
    X(B_M3, m3, ge, m2 * 2 * GE)                  \
    X(B_RFLAGS, rflags, uint8_t, m2)              \
    X(B_PBASE, pbase, ge, m2 * 3 * GE)
enum VerifyBuf { BP_VERIFY_BUFS(BP_BUF_ID) B_PERM, B_COUNT };
inline void verify_sizes(size_t B, size_t n, size_t Lb, int range_mode, size_t (&sz)[B_COUNT]) {
    const size_t Lc = Lb ? Lb : 1, m2 = range_mode == 2 ? B : 0;
    BP_VERIFY_BUFS(BP_BUF_SIZE)
    sz[B_PERM] = 0;
}

// The canonical-tree MSM (launch_msm_full: `count` MSMs of n points) and the point tree
// (launch_tree_full of n points) share one per-stream set; each call sizes its own buffers.
enum MsmBuf { MB_TERMS, MB_ROOT0, MB_ROOT1, MB_TREE0, MB_TREE1, MB_ORDER, MB_BINS, MB_COUNT };
inline void msm_sizes(size_t n, size_t count, size_t (&sz)[MB_COUNT]) {
    const size_t tot = n * count, nb = count * ((n + 255) / 256);
    sz[MB_TERMS] = tot * GE;                 // per-point terms
    sz[MB_ROOT0] = sz[MB_ROOT1] = nb * GE;   // block roots
    sz[MB_TREE0] = sz[MB_TREE1] = 0;
    sz[MB_ORDER] = tot * U32;                // lane order
    sz[MB_BINS] = MSM_BINS * U32;            // its sort bins
}
inline void tree_sizes(size_t n, size_t (&sz)[MB_COUNT]) {
    for (size_t& s : sz) s = 0;
    sz[MB_TREE0] = sz[MB_TREE1] = (n + 255) / 256 * GE;   // tree ping-pong
}

// The Pippenger bucket MSM (bp_pippenger.hip).  Its kernels and the shape share these:
constexpr int PTPB = 256;                // threads per block
constexpr int PM = 16;                   // buckets per chunk
constexpr int SCAN_PER = 4;              // buckets per thread of the layout scans
constexpr int SCAN_BLK = PTPB * SCAN_PER;
constexpr uint32_t BID_PIECE = 4096;     // list elements per k_pip_bidfill wave
// One part of a call: windows [w0, w1) of `count` MSMs over n points, c-bit digits.  force16:
// HIPBP_PIP_KEYS16; tail_layer: HIPBP_PIP_TAIL_LAYER, clamped to 1 .. 8.
struct PipShape {
    size_t n, count;
    int c, w0, Wp;         // Wp: the part's windows
    size_t W, NB, nb, N;   // virtual windows (the part's windows of every MSM), buckets per window, buckets, keys
    size_t NC;             // chunks per window
    int ib;                // bits of the point index in a 32-bit key
    bool k32;              // 32-bit keys (digit << ib | i), no values; else 16-bit digit keys and values
    int levels, steps, T;  // worst-case tree depth (a bucket list is at most n long), two levels per step;
                           // layouts 0 .. steps, then the start layer T
    unsigned nparts;       // scan blocks per layer
    size_t tot0, qcap;     // step 0 reads <= N + 3 nb padded positions and writes a quarter of them (+ padding)
    size_t nbq;            // bidfill queue capacity (further pieces of long lists)
    int TT;                // the LDS tail takes over at layer TT (0: none)
};
inline PipShape pip_shape(size_t n, size_t count, int c, int w0, int w1, bool force16, int tail_layer) {
    PipShape s;
    s.n = n; s.count = count; s.c = c; s.w0 = w0;
    s.Wp = w1 - w0;
    s.W = (size_t)s.Wp * count;
    s.NB = (size_t)1 << c; s.nb = s.W * s.NB; s.N = s.W * n; s.NC = s.NB / PM;
    s.ib = 0;
    while (s.ib < 32 && ((size_t)1 << s.ib) < n) s.ib++;
    s.k32 = c + s.ib <= 32 && !force16;
    s.levels = 1;
    while (s.levels < 31 && ((size_t)1 << s.levels) < n) s.levels++;
    s.steps = (s.levels + 1) / 2; s.T = s.steps + 1;
    s.nparts = (unsigned)((s.nb + SCAN_BLK - 1) / SCAN_BLK);
    s.tot0 = s.N + 3 * s.nb; s.qcap = s.tot0 / 4 + 4 * s.nb;
    s.nbq = s.N / BID_PIECE + 1;
    s.TT = s.steps > tail_layer ? tail_layer : 0;
    return s;
}
// The part's workspace (PipWs).  lay: LEN | PAD | OFF, T + 1 layers of nb each.  Wtot: all the windows
// of an MSM where this workspace also holds the whole call's window sums and the top part's Horner
// value (msm_pippenger's top part), else 0.  sort_temp: rocPRIM's scratch, from its size query.
#define BP_PIP_BUFS(X)                                                \
    X(PIP_KEYS_IN, keys_in, void, s.N * (s.k32 ? 4 : 2))              \
    X(PIP_KEYS, keys, void, s.N * (s.k32 ? 4 : 2))                    \
    X(PIP_VALS, vals, uint32_t, s.k32 ? 0 : s.N * 4)                  \
    X(PIP_START, start, uint32_t, s.nb * 4)                           \
    X(PIP_LEN0, len[0], uint32_t, s.nb * 4)                           \
    X(PIP_LEN1, len[1], uint32_t, s.nb * 4)                           \
    X(PIP_LAY, lay, uint32_t, (size_t)3 * (s.T + 1) * s.nb * 4)       \
    X(PIP_PART, part, uint32_t, (size_t)(s.T + 1) * s.nparts * 4)     \
    X(PIP_BID0, bid[0], uint32_t, s.tot0 * 4)                         \
    X(PIP_BID1, bid[1], uint32_t, s.qcap * 4)                         \
    X(PIP_Q0, Q[0], ge, s.qcap * GE)                                  \
    X(PIP_Q1, Q[1], ge, s.qcap * GE)                                  \
    X(PIP_V, V, ge, s.W * s.NC * GE)                                  \
    X(PIP_S, S, ge, s.nb * GE)                                        \
    X(PIP_MAXLEN, maxlen, unsigned, 3 * U32)                          \
    X(PIP_TAILQ, tailq, uint32_t, s.TT ? s.nb * U32 : 0)              \
    X(PIP_BQ, bq, uint2, s.nbq * 8)                                   \
    X(PIP_SW, Sw, ge, s.count * Wtot * GE)                            \
    X(PIP_TMID, Tmid, ge, Wtot ? s.count * GE : 0)                    \
    X(PIP_TEMP, temp, void, sort_temp)
enum PipBuf { BP_PIP_BUFS(BP_BUF_ID) PIP_COUNT };
inline void pip_sizes(const PipShape& s, size_t Wtot, size_t sort_temp, size_t (&sz)[PIP_COUNT]) {
    BP_PIP_BUFS(BP_BUF_SIZE)
}

}  // namespace bp

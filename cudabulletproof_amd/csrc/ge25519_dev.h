// ge25519_dev.h — gfx950 device point arithmetic reproducing the reference's "ge25519"
// extended-coordinate operations bit for bit.
//
// Freedoms used (all bit-preserving):
//  * the q-side terms (Y2-X2), (Y2+X2) of an add are computed once per fixed point;
//  * a doubling add(r, r) computes (Y-X) and (Y+X) once and squares them (same exact
//    product, so the same bits);
//  * a scalar's leading zero bits only ever double the identity: that prefix is a
//    table lookup (ident_doublings[k] = k doublings of (0,1,1,0)).
#pragma once
#include "fe25519_dev.h"

namespace bp {

struct ge {
    fe X, Y, Z, T;
};

// q-side operands of ge25519_add: (Y-X), (Y+X), Z, T
struct geq {
    fe YmX, YpX, Z, T;
};

// curve25519_ops.cu:341-346 — LE bytes A3 78 59 13 ... 03 52 (this is d, used where 2d is meant)
BP_DEV fe k_const() {
    return fe{{0x75EB4DCA135978A3ull, 0x00700A4D4141D8ABull, 0x8CC740797779E898ull, 0x52036CEE2B6FFE73ull}};
}

// fe25519_mul(f, k) (the C = (T1 T2) k of every point operation): the same exact 512-bit product and
// fold as fe_mul(f, k_const()), with the product counting only the carries a column's running-sum
// bound allows (mul512_k_asm: 16 counts instead of 50; k's words are SGPR operands).
template <int LAT = 0>
BP_DEV fe fe_mul_k(const fe& f, uint32_t* acc = nullptr) {
#if BP_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    uint32_t a[8], w[16];
    fe_words(a, f);
    if constexpr (BP_MUL_CIN && (LAT == 0 || LAT == 3)) mul512_k_cin_asm(w, a); else mul512_k_asm(w, a);
    uint64_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = cat64(w[2 * i], w[2 * i + 1]);
    return fe_fold512<LAT>(t, acc);   // (the product by k has no gate)
#else
    return fe_mul(f, k_const());
#endif
}

BP_DEV ge ge_zero() { return ge{fe_set(0), fe_set(1), fe_set(1), fe_set(0)}; }   // curve25519_ops.cu:318

BP_DEV geq ge_prep(const ge& q) {
    return geq{fe_sub(q.Y, q.X), fe_add(q.Y, q.X), q.Z, q.T};
}

// device_ge25519_normalize (device_curve25519_ops.cuh:243-270): z_inv = 1.
BP_DEV ge ge_norm_dev(const ge& p) {
    ge r;
    r.X = fe_mul_one(p.X);
    r.Y = fe_mul_one(p.Y);
    r.Z = fe_set(1);
    r.T = fe_mul(r.X, r.Y);
    return r;
}

// ge25519_normalize (curve25519_ops.cu:574-605): keep the point when the canonical
// bytes of Z are 1, else multiply by the 13-step "invert" of Z.
BP_DEV ge ge_norm_host(const ge& p) {
    if (fe_is_one(fe_canon(p.Z))) return p;
    fe zi = fe_invert(p.Z);
    ge r;
    r.X = fe_mul(p.X, zi);
    r.Y = fe_mul(p.Y, zi);
    r.Z = fe_set(1);
    r.T = fe_mul(r.X, r.Y);
    return r;
}

BP_DEV int fe_clz256(const fe& s) {
    if (s.v[3]) return __clzll(s.v[3]);
    if (s.v[2]) return 64 + __clzll(s.v[2]);
    if (s.v[1]) return 128 + __clzll(s.v[1]);
    if (s.v[0]) return 192 + __clzll(s.v[0]);
    return 256;
}

BP_DEV ge ld_ge(const ge* p) { return *p; }

// Fixed-base prefix tables (optional, for points that are the same in every proof: the
// generators G_i, H_i, g, h).  ptab[p], p < 2^K, is the state of ge25519_scalarmult on this base
// after the top K bits of any scalar whose top K bits are p: the identity, then for each of
// those bits one add(r, r) and, for a set bit, one add(r, P).  A scalar with fewer than K
// leading zeros starts from ptab[top K bits] at bit 255 - K instead of from the identity at bit
// 255: the remaining operations are the same ones in the same order, so the result has the same
// bits.  (With K or more leading zeros the identity-doubling table dtab already covers them.)
constexpr int PREFIX_MAX_BITS = 24;
BP_DEV uint32_t prefix_index(const fe& s, int K) { return (uint32_t)(s.v[3] >> (64 - K)); }

// Length of ge25519_scalarmult's add chain past the leading zeros: the per-lane loop runs
// (256 - clz) doublings + popcount adds, and a wave runs as long as its longest lane.
BP_DEV int sm_ops(const fe& s) {
    return (256 - fe_clz256(s)) + __popcll(s.v[0]) + __popcll(s.v[1]) + __popcll(s.v[2]) + __popcll(s.v[3]);
}
// The same with a K-bit prefix table for the base (K = 0: none).
BP_DEV int sm_ops_prefix(const fe& s, int K) {
    if (K <= 0 || fe_clz256(s) >= K) return sm_ops(s);
    const uint64_t top = K == 64 ? 0 : (s.v[3] & (~0ull >> K));
    return (256 - K) + __popcll(s.v[0]) + __popcll(s.v[1]) + __popcll(s.v[2]) + __popcll(top);
}

// q-side operand access.  QLDS = true: this lane's LDS slot, read at the point of use (the
// empty asm with a memory clobber stops the compiler from hoisting the loads and keeping all
// of q in VGPRs, which would cost occupancy in the throughput kernels).  QLDS = false: a
// register copy (latency-bound kernels run one wave per SIMD, registers are free there).
template <bool QLDS>
BP_DEV fe qget(const fe* p) {
    if (QLDS) asm volatile("" ::: "memory");
    return *p;
}

// ---- the field mode of a point form ----
// Every point form below is written once and takes a mode, which says how its field blocks treat
// their two rare tests: the fix-up's rare edge inside every block (about 2^-32 of lanes) and the
// bounded product's gate before every general product and square (about 2^-27), some 22 compares,
// each with a SALU test and a branch, per point operation, whose results the step can never use.
//  * Gated: every block tests in place and takes its exact form on a hit (fe25519_dev.h LAT 0).
//  * Defer: the blocks run their fast statements only (LAT 3) and max the words those tests read
//    into the mode's two running words: acc reaches 2^32-1 exactly when a block's test would have
//    fired for this lane, gacc exceeds MUL_BOUNDED_WORD exactly when a gate would have.  A max only
//    grows and the first edge is met on operands that are still correct, so one test of the two
//    words (defer_hit) is sound wherever it is placed later; on a hit the caller drops the pass and
//    reruns the scalar multiplication from its start in the gated mode (scalarmult), so the results
//    are the same bits.  (The row form recomputes one step instead: it can keep the step's inputs
//    live; here the lane forms sit at the VGPR limit.)
// fe_mul_one keeps its in-statement test in both modes.
struct Gated {
    static constexpr int LAT = 0;
    BP_DEV uint32_t* edge() { return nullptr; }
    BP_DEV uint32_t* gate() { return nullptr; }
};
struct Defer {
    static constexpr int LAT = 3;
    uint32_t acc = 0, gacc = 0;
    BP_DEV uint32_t* edge() { return &acc; }
    BP_DEV uint32_t* gate() { return &gacc; }
};
BP_DEV bool defer_hit(const Gated&) { return false; }
BP_DEV bool defer_hit(const Defer& d) {
    return __builtin_amdgcn_ballot_w64((d.acc == 0xFFFFFFFFu) | (d.gacc > MUL_BOUNDED_WORD)) != 0;
}
template <class M> BP_DEV fe m_add(const fe& f, const fe& g, M& m) { return fe_add<M::LAT>(f, g, m.edge()); }
template <class M> BP_DEV fe m_sub(const fe& f, const fe& g, M& m) { return fe_sub<M::LAT>(f, g, m.edge()); }
template <class M> BP_DEV fe m_mul(const fe& f, const fe& g, M& m) { return fe_mul<M::LAT>(f, g, m.edge(), m.gate()); }
template <class M> BP_DEV fe m_sq(const fe& f, M& m) { return fe_sq<M::LAT>(f, m.edge(), m.gate()); }
template <class M> BP_DEV fe m_mul_k(const fe& f, M& m) { return fe_mul_k<M::LAT>(f, m.edge()); }
#ifndef BP_LANE_GATE_SEEN
#define BP_LANE_GATE_SEEN 1   // 0: every product of ge_tail puts its own gate words into the running word (A/B builds)
#endif
// A product whose two gate words an earlier product of the same form has already put into the Defer
// mode's running word (a max is idempotent): it runs on a copy of the mode whose gate word is dropped,
// and with it the statement; the edge word is carried on.  The Gated mode tests in place as everywhere.
template <class M> BP_DEV fe mul_gate_seen(const fe& f, const fe& g, M& m) {
    if constexpr (M::LAT == 3 && BP_LANE_GATE_SEEN) {
        M seen = m;
        const fe r = m_mul(f, g, seen);
        m.acc = seen.acc;
        return r;
    } else {
        return m_mul(f, g, m);
    }
}
#ifndef BP_LANE_ADDSUB
#define BP_LANE_ADDSUB 1
#endif
// E/H and F/G of ge25519_add: one fused block (fe_addsub, chains interleaved) or two calls
// (-DBP_LANE_ADDSUB=0, for A/B builds); the same bits either way.
template <class M> BP_DEV void m_addsub(const fe& f, const fe& g, fe& sum, fe& diff, M& m) {
#if BP_LANE_ADDSUB
    fe_addsub<M::LAT>(f, g, sum, diff, m.edge());
#else
    diff = fe_sub<M::LAT>(f, g, m.edge());
    sum = fe_add<M::LAT>(f, g, m.edge());
#endif
}

#ifndef BP_LANE_ADDSUB_ST1
#define BP_LANE_ADDSUB_ST1 1
#endif
// Y1 - X1 and Y1 + X1 of every stage 1: the fused block again (one running word and one chain's wait
// states fewer per step), or the two calls (-DBP_LANE_ADDSUB_ST1=0, for A/B builds); the same bits.
template <class M> BP_DEV void ymx_ypx(const ge& p, fe& ymx, fe& ypx, M& m) {
#if BP_LANE_ADDSUB_ST1
    m_addsub(p.Y, p.X, ypx, ymx, m);
#else
    ymx = m_sub(p.Y, p.X, m);
    ypx = m_add(p.Y, p.X, m);
#endif
}

// ---- ge25519_add (curve25519_ops.cu:326-378 == device_curve25519_ops.cuh:188-241) ----
// Stage 1 is A = (Y1-X1)(Y2-X2), B = (Y1+X1)(Y2+X2), C = (T1 T2) k and ZZ = Z1 Z2, in that order; the
// three shapes below differ only there.  ge_tail is stages 2 and 3, the same for all of them.
template <class M>
BP_DEV ge ge_tail(const fe& A, const fe& B, const fe& C, const fe& ZZ, M& m) {
    fe D = m_add(ZZ, ZZ, m);
    fe E, F, G, H;
    m_addsub(B, A, H, E, m);   // H = B + A, E = B - A
    m_addsub(D, C, G, F, m);   // G = D + C, F = D - C
    // A product's gate reads its first factor's word 0 and its second factor's word 7, and its 512 bits do
    // not depend on which factor is named first: with Z3 formed as G F the four gates read E0, F7, G0, H7
    // only, and the first two products have put all four into the running word already.
#if BP_LANE_GATE_SEEN
    return ge{m_mul(E, F, m), m_mul(G, H, m), mul_gate_seen(G, F, m), mul_gate_seen(E, H, m)};
#else
    return ge{m_mul(E, F, m), m_mul(G, H, m), m_mul(F, G, m), m_mul(E, H, m)};
#endif
}

// The three shapes are each their stage 1 and the one tail.  TAIL = false stops after stage 1 and hands
// back (A, B, C, ZZ) in the four slots of a ge, for the per-lane step's vote (ge_add_sel).

// add(p, p) (curve25519_ops.cu:406 / device .cuh:282): the same exact products as squares.
template <bool TAIL = true, class M>
BP_DEV ge ge_dbl(const ge& p, M& m) {
    fe ymx, ypx;
    ymx_ypx(p, ymx, ypx, m);
    fe A = m_sq(ymx, m);
    fe B = m_sq(ypx, m);
    fe C = m_mul_k(m_sq(p.T, m), m);
    fe ZZ = m_sq(p.Z, m);
    if (!TAIL) return ge{A, B, C, ZZ};
    return ge_tail(A, B, C, ZZ, m);
}

// add(p, q) with q's prepared operands.
// zone (wave-uniform): every lane's q.Z is exactly 1 (generators, host-normalized points), so
// Z1*Z2 = fold(Z1 || 0) = the conditional lossy "- p" of Z1 (fe_mul_one) — same bits, no product.
template <bool QLDS, bool TAIL = true, class M>
BP_DEV ge ge_add_qp(const ge& p, const geq* q, bool zone, M& m) {
    fe ymx, ypx;
    ymx_ypx(p, ymx, ypx, m);
    fe A = m_mul(ymx, qget<QLDS>(&q->YmX), m);
    fe B = m_mul(ypx, qget<QLDS>(&q->YpX), m);
    fe C = m_mul_k(m_mul(p.T, qget<QLDS>(&q->T), m), m);
    fe ZZ = zone ? fe_mul_one(p.Z) : m_mul(p.Z, qget<QLDS>(&q->Z), m);
    if (!TAIL) return ge{A, B, C, ZZ};
    return ge_tail(A, B, C, ZZ, m);
}

#ifndef BP_LANE_VOTE
#define BP_LANE_VOTE 1   // 0: the per-lane loop's step runs its selected stage 1 on every step (A/B builds)
#endif
// One step of the per-lane loop: add(r, r) when !use_q, add(r, q) when use_q, with a wave vote on its
// stage 1.  Lanes with the same scalar are in the same phase at every step, and after the verify's lane
// sort a fold round's wave holds few distinct scalars: when every lane still in the loop doubles, the step
// runs the doubling's stage 1 (squares, no selects), when every one adds, the add's (q's operands straight
// from the slot, no Z^2); else its own, where the select is per lane.  One ballot over the active lanes (a
// lane that has left the loop is not in exec and has no say), one scalar branch, one copy of the tail; the
// operation order is ge25519_add's in every body and each forms the same exact products, so the bits are
// the same whichever runs.  PATH forces a body (the instruction-count probes, BP_LANE_VOTE 0): 0 doubling,
// 1 add, 2 selected; -1 votes.
// ZONE (wave-uniform): every lane's q.Z is exactly 1, so the add lanes' Z1*Z2 is fe_mul_one(Z1)
// and the doubling lanes' is the square Z1^2 — both formed, one kept (the same bits as the
// general product; 150 + ~20 VALU instead of 189 + the operand select).
template <bool QLDS, bool ZONE = false, int PATH = (BP_LANE_VOTE ? -1 : 2), class M>
BP_DEV ge ge_add_sel(const ge& p, const geq* q, bool use_q, M& m) {
    const uint64_t adds = __builtin_amdgcn_ballot_w64(use_q), live = __builtin_amdgcn_ballot_w64(true);
    ge s;   // stage 1: A, B, C, ZZ
    if (PATH == 0 || (PATH < 0 && adds == 0)) {
        s = ge_dbl<false>(p, m);
    } else if (PATH == 1 || (PATH < 0 && adds == live)) {
        s = ge_add_qp<QLDS, false>(p, q, ZONE, m);
    } else {
        // q's operands are loaded unconditionally and selected as values: a select between a
        // loaded and a computed value is otherwise folded into a load through a select of
        // pointers, which forces `p` into private memory (scratch).
        fe ymx, ypx;
        ymx_ypx(p, ymx, ypx, m);
        fe qa = qget<QLDS>(&q->YmX);
        s.X = m_mul(ymx, use_q ? qa : ymx, m);
        fe qb = qget<QLDS>(&q->YpX);
        s.Y = m_mul(ypx, use_q ? qb : ypx, m);
        fe qt = qget<QLDS>(&q->T);
        s.Z = m_mul_k(m_mul(p.T, use_q ? qt : p.T, m), m);
        if (ZONE) {
            // (the square first: with fe_mul_one first, k_terms<1>'s deferred loop reloads a spilled pair
            // after this body, profiles/NOTES.md §15)
            fe d2 = m_sq(p.Z, m), d1 = fe_mul_one(p.Z);
            s.T = use_q ? d1 : d2;
        } else {
            fe qz = qget<QLDS>(&q->Z);
            s.T = m_mul(p.Z, use_q ? qz : p.Z, m);
        }
    }
    return ge_tail(s.X, s.Y, s.Z, s.T, m);
}

// The gated mode under the plain names (every caller outside the lane loops' deferred pass).
BP_DEV ge ge_dbl(const ge& p) { Gated m; return ge_dbl(p, m); }
template <bool QLDS>
BP_DEV ge ge_add_qp(const ge& p, const geq* q, bool zone = false) { Gated m; return ge_add_qp<QLDS>(p, q, zone, m); }
template <bool QLDS, bool ZONE = false, int PATH = (BP_LANE_VOTE ? -1 : 2)>
BP_DEV ge ge_add_sel(const ge& p, const geq* q, bool use_q) { Gated m; return ge_add_sel<QLDS, ZONE, PATH>(p, q, use_q, m); }
BP_DEV ge ge_add_q(const ge& p, const geq& q) { return ge_add_qp<false>(p, &q); }
BP_DEV ge ge_add(const ge& p, const ge& q) { return ge_add_q(p, ge_prep(q)); }

#ifndef BP_LANE_DEFER
#define BP_LANE_DEFER 1   // 0: scalarmult runs the gated mode only (A/B builds)
#endif
#ifndef BP_DEFER_CHUNK
#define BP_DEFER_CHUNK 32   // loop steps between two tests of the running words
#endif
constexpr int DEFER_WARM = 2;   // the per-lane loop's steps that run gated before its deferred pass (sm_lane_loop)

// MSB-first bit stream over a 256-bit scalar, kept as a shift register of limbs so that no
// array is ever indexed by a run-time value (that would place the scalar in scratch).
struct BitStream {
    uint64_t cur, n1, n2, n3;   // cur's MSB is the next bit
    int left;                   // bits left in cur
};

// Position the stream at bit i (0..255) of s.
BP_DEV BitStream bs_init(const fe& s, int i) {
    BitStream b{s.v[3], s.v[2], s.v[1], s.v[0], 0};
    int L = i >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        bool sh = k < 3 - L;
        b.cur = sh ? b.n1 : b.cur;
        b.n1 = sh ? b.n2 : b.n1;
        b.n2 = sh ? b.n3 : b.n2;
        b.n3 = sh ? 0 : b.n3;
    }
    int bi = i & 63;
    b.cur <<= (63 - bi);
    b.left = bi + 1;
    return b;
}

BP_DEV uint32_t bs_next(BitStream& b) {
    uint32_t bit = (uint32_t)(b.cur >> 63);
    b.cur <<= 1;
    if (--b.left == 0) {
        b.cur = b.n1;
        b.n1 = b.n2;
        b.n2 = b.n3;
        b.n3 = 0;
        b.left = 64;
    }
    return bit;
}

// The start of every scalar-multiplication loop: the state after the scalar's leading zeros (dtab) or
// after its top K bits (the base's prefix table, when it has one and the scalar has fewer than K
// leading zeros), and in i the index of the pending bit (-1: none, the state is the result).
// WAVE: the prefix start only when every lane has a table (the start bit must stay wave-uniform).
template <bool WAVE = false>
BP_DEV ge sm_start(const fe& s, const ge* ptab, int K, const ge* __restrict__ dtab, int& i) {
    const int lz = fe_clz256(s);
    const bool pre = K > 0 && lz < K && (WAVE ? __all(ptab != nullptr) : ptab != nullptr);
    const ge r = ld_ge(pre ? &ptab[prefix_index(s, K)] : &dtab[lz]);
    i = pre ? 255 - K : 255 - lz;
    return r;
}

// ge25519_scalarmult (curve25519_ops.cu:397-415 == device .cuh:272-290) for a scalar
// that is the same in every lane of the wave: the bit test is a scalar branch.
// `s` holds the scalar's 256 bits (limb i = bytes 8i..8i+7, little-endian); `q` holds
// ge_prep(P); `dtab` = the identity-doubling table (257 points).
// DEFER = true is the common pass in the Defer mode: false when some lane met a rare edge or a failed gate
// (tested every BP_DEFER_CHUNK steps and once after the loop; FORCE: after the first chunk whatever the
// data, the probe's recovery mode); DEFER = false is the Gated mode throughout and returns true.  The first
// steps of a deferred pass run gated: the start state from dtab is a doubled identity, whose small
// coordinates put Y - X on fe25519_sub's rare edge (word 1 of the difference is 0) in every lane, and the
// pass would be dropped in every wave; after the first add of P the state is an ordinary point.
template <bool QLDS, bool DEFER, bool FORCE = false>
BP_DEV bool sm_uniform(ge& out, const fe& s_in, const geq* q, const ge* __restrict__ dtab, const ge* ptab, int K) {
    fe s;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)s_in.v[i]);
        uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(s_in.v[i] >> 32));
        s.v[i] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    int i;
    ge r = sm_start<true>(s, ptab, K, dtab, i);
    if (i >= 0) {
        const bool zone = __all(fe_is_one(qget<QLDS>(&q->Z)));
        BitStream bs = bs_init(s, i);
        if (DEFER) {   // the top bit's step, gated (above)
            r = ge_dbl(r);
            if (bs_next(bs)) r = ge_add_qp<QLDS>(r, q, zone);
            i--;
        }
        std::conditional_t<DEFER, Defer, Gated> m;
        int n = 0;
        for (; i >= 0; i--) {
            r = ge_dbl(r, m);
            if (bs_next(bs)) r = ge_add_qp<QLDS>(r, q, zone, m);
            if (DEFER && ++n == BP_DEFER_CHUNK) {
                n = 0;
                if (FORCE || __builtin_expect(defer_hit(m), 0)) return false;
            }
        }
        if (DEFER && __builtin_expect(defer_hit(m), 0)) return false;
    }
    out = r;
    return true;
}

// The per-lane loops' bit bookkeeping after one operation: a doubling at a set bit is followed by the
// add of P, anything else by the next bit's doubling.
BP_DEV void lane_advance(bool& add_phase, uint32_t& bit, int& i, BitStream& bs) {
    if (!add_phase && bit) {
        add_phase = true;
    } else {
        add_phase = false;
        i--;
        bit = bs_next(bs);
    }
}

// Same function for a per-lane scalar: every iteration is one ge25519_add whose second
// operand is either r itself (the doubling) or P, so no lane idles on the other's branch.
template <bool QLDS, bool ZONE, bool DEFER, bool FORCE = false>
BP_DEV bool sm_lane_loop(ge& out, const fe& s, const geq* q, const ge* __restrict__ dtab, const ge* ptab, int K) {
    int i;   // index of the pending bit
    ge r = sm_start<false>(s, ptab, K, dtab, i);
    BitStream bs = bs_init(s, i < 0 ? 0 : i);
    uint32_t bit = i >= 0 ? bs_next(bs) : 0;
    bool add_phase = false;    // false: next op doubles; true: next op adds P
    // a lane's first DEFER_WARM steps (the top bit's doubling and add), gated (above sm_uniform)
    for (int warm = 0; DEFER && warm < DEFER_WARM && i >= 0; warm++) {
        r = ge_add_sel<QLDS, ZONE>(r, q, add_phase);
        lane_advance(add_phase, bit, i, bs);
    }
    if constexpr (!DEFER) {
        while (i >= 0) {
            r = ge_add_sel<QLDS, ZONE>(r, q, add_phase);
            lane_advance(add_phase, bit, i, bs);
        }
        out = r;
        return true;
    }
    std::conditional_t<DEFER, Defer, Gated> m;
    int n = 0;
    bool hit = false;
    while (i >= 0) {
        r = ge_add_sel<QLDS, ZONE>(r, q, add_phase, m);
        lane_advance(add_phase, bit, i, bs);
        if (DEFER && ++n == BP_DEFER_CHUNK) {   // n is the same in every lane still in the loop
            n = 0;
            if (FORCE || __builtin_expect(defer_hit(m), 0)) {
                hit = true;
                break;
            }
        }
    }
    // lanes that left the loop earlier did not see a later chunk's hit: one vote for the whole wave
    if (DEFER && __builtin_expect(__builtin_amdgcn_ballot_w64(hit) != 0 || defer_hit(m), 0)) return false;
    out = r;
    return true;
}

template <bool QLDS, bool FORCE = false>
BP_DEV ge sm_lane(const fe& s, const geq* q, const ge* __restrict__ dtab, const ge* ptab, int K) {
    const bool zone = __all(fe_is_one(qget<QLDS>(&q->Z)));
    ge r;
#if BP_LANE_DEFER
    if (zone ? sm_lane_loop<QLDS, true, true, FORCE>(r, s, q, dtab, ptab, K)
             : sm_lane_loop<QLDS, false, true, FORCE>(r, s, q, dtab, ptab, K))
        return r;
#endif
    if (zone) sm_lane_loop<QLDS, true, false>(r, s, q, dtab, ptab, K);
    else sm_lane_loop<QLDS, false, false>(r, s, q, dtab, ptab, K);
    return r;
}

// Wave-level dispatch: uniform scalar -> scalar-branch loop, else the per-lane loop.
// QLDS: `slot` is this lane's LDS slot and receives ge_prep(P); otherwise q stays in VGPRs.
// ptab / K: this lane's base's prefix table (nullable) and its width in bits (0: none).
// The loops first run their deferred pass (above); when it reports a rare edge or a failed gate in
// some lane the wave runs the same scalar multiplication again from its start state (s, the slot,
// dtab, ptab and K are all still there) in the gated mode.  FORCE: see sm_uniform.
template <bool QLDS, bool FORCE = false>
BP_DEV ge scalarmult(const fe& s, const ge& P, geq* slot, const ge* __restrict__ dtab, const ge* ptab = nullptr,
                     int K = 0) {
    geq qreg;
    const geq* q;
    if (QLDS) {
        fe ymx = fe_sub(P.Y, P.X), ypx = fe_add(P.Y, P.X);
#pragma unroll
        for (int k = 0; k < 4; k++) {   // limb stores: an aggregate copy would stage through scratch
            slot->YmX.v[k] = ymx.v[k];
            slot->YpX.v[k] = ypx.v[k];
            slot->Z.v[k] = P.Z.v[k];
            slot->T.v[k] = P.T.v[k];
        }
        q = slot;
    } else {
        qreg = ge_prep(P);
        q = &qreg;
    }
    uint32_t same = 1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t lo = (uint32_t)s.v[i], hi = (uint32_t)(s.v[i] >> 32);
        same &= (lo == __builtin_amdgcn_readfirstlane(lo)) & (hi == __builtin_amdgcn_readfirstlane(hi));
    }
    if (__all(same)) {
        ge r;
#if BP_LANE_DEFER
        if (sm_uniform<QLDS, true, FORCE>(r, s, q, dtab, ptab, K)) return r;
#endif
        sm_uniform<QLDS, false>(r, s, q, dtab, ptab, K);
        return r;
    }
    return sm_lane<QLDS, FORCE>(s, q, dtab, ptab, K);
}

}  // namespace bp

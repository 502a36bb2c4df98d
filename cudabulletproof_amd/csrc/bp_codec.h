// bp_codec.h — the compact proof blob ("HBPC", version 1): its layout, its header, and
// the per-lane bodies of the encoder and the decoder (internal to the library).  Pure like
// bp_layout.h: no HIP runtime calls.  The kernels of bp_codec.hip and the CPU paths of bp_api_blob.hip
// call exactly the functions below, so tests/codec_check.hip runs every one of them on a CPU, the
// malformed blobs under ASan + UBSan.
//
// All integers little-endian; a field element is its four limbs as stored.  Lr = L_len, f = 1 with
// taux and mu:
//   0 "HBPC" | 4 u16 version | 6 u16 flags | 8 u32 n | 12 u32 ab_len | 16 u32 L_len | 20 u32 R | 24 u64 count
//   32 kind[count] (0 compact, 1 raw), zero-padded to 8 | compact area: count slots of S_c (a raw
//   proof's slot is zero) | raw_index[R] u32 ascending, zero-padded to 8 | raw area: R records of S_r
//   compact slot: X|Y of V A S T1 T2 L[0..Lr) R[0..Lr) | t x | taux mu if f     (S_c = 0 when ab_len != 1)
//   raw record:   the same points whole | t c x | taux mu if f | a[ab_len] | b[ab_len]
// The blob side is addressed in 16-byte units at 8-byte alignment (the sections are padded to 8, no
// further); the flat arrays' side is 16-byte aligned, one 16-byte access per unit.
#pragma once
#include <cstring>

#include "bp_layout.h"
#include "ge25519_dev.h"

namespace bp {

constexpr uint16_t CODEC_VERSION = 1;
constexpr size_t CODEC_HEADER = 32;
constexpr size_t CODEC_MAX_COUNT = (size_t)1 << 22;
constexpr size_t CODEC_BLK = 256;                                  // proofs per block of the encoder's launches
constexpr size_t CODEC_MAX_BLOCKS = CODEC_MAX_COUNT / CODEC_BLK;   // 16384: the scan's one block takes them all

// (may_alias: the units are read and written over fe / ge objects)
struct alignas(16) __attribute__((may_alias)) u128 {
    uint64_t lo, hi;
};

BP_DEV size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

// ------------------------------------------------------------------ layout
struct CodecWs {
    uint32_t* blk;   // the raw proofs of each block of CODEC_BLK proofs, then (scanned) their offsets and the total
};

struct CodecLayout {
    size_t count, abl, Lr;
    int f;
    BP_DEV size_t npts() const { return 5 + 2 * Lr; }
    BP_DEV size_t Sc() const { return abl == 1 ? 64 * npts() + 64 + 64 * (size_t)f : 0; }
    BP_DEV size_t Sr() const { return 128 * npts() + 96 + 64 * (size_t)f + 64 * abl; }
    BP_DEV size_t o_kind() const { return CODEC_HEADER; }
    BP_DEV size_t o_compact() const { return o_kind() + pad8(count); }
    BP_DEV size_t o_rawidx() const { return o_compact() + count * Sc(); }
    BP_DEV size_t o_raw(size_t R) const { return o_rawidx() + pad8(4 * R); }
    BP_DEV size_t bytes(size_t R) const { return o_raw(R) + R * Sr(); }
    BP_DEV size_t bound() const { return bytes(count); }   // every proof raw
};

// the shapes a blob may have (the issue's limits): 0: fine, else the reason
inline const char* codec_shape_error(size_t count, size_t n, size_t abl, size_t Lr, unsigned flags) {
    if (flags & ~1u) return "unknown flag bits";
    if (count > CODEC_MAX_COUNT) return "count above 2^22";
    if (n == 0 || (n & (n - 1)) || n > 65536) return "n must be a power of two <= 65536";
    size_t lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    if (Lr > lg) return "L_len > log2(n)";
    if (abl < 1 || abl > 65536) return "ab_len must be 1..65536";
    return nullptr;
}

// ------------------------------------------------------------------ header
BP_DEV void put_le(uint8_t* p, uint64_t v, int nb) {
    for (int k = 0; k < nb; k++) p[k] = (uint8_t)(v >> (8 * k));
}
BP_DEV uint64_t get_le(const uint8_t* p, int nb) {
    uint64_t v = 0;
    for (int k = 0; k < nb; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
BP_DEV void codec_write_header(uint8_t* h, const CodecLayout& l, size_t n, size_t R) {
    h[0] = 'H'; h[1] = 'B'; h[2] = 'P'; h[3] = 'C';
    put_le(h + 4, CODEC_VERSION, 2);
    put_le(h + 6, (uint64_t)l.f, 2);
    put_le(h + 8, n, 4);
    put_le(h + 12, l.abl, 4);
    put_le(h + 16, l.Lr, 4);
    put_le(h + 20, R, 4);
    put_le(h + 24, l.count, 8);
}
inline CodecLayout codec_layout(const hipbp_proof_blob_info& i) {
    return CodecLayout{i.count, i.ab_len, i.L_len, (int)(i.flags & 1)};
}
// The 32 header bytes into *info, checked against the limits and the blob's byte length (the exact
// size the header implies).  0: fine, else the reason.
inline const char* codec_parse_header(const uint8_t* h, size_t blob_bytes, hipbp_proof_blob_info* info) {
    if (blob_bytes < CODEC_HEADER) return "blob shorter than its header";
    if (memcmp(h, "HBPC", 4) != 0) return "bad magic";
    if (get_le(h + 4, 2) != CODEC_VERSION) return "unsupported version";
    const unsigned flags = (unsigned)get_le(h + 6, 2);
    const size_t n = get_le(h + 8, 4), abl = get_le(h + 12, 4), Lr = get_le(h + 16, 4), R = get_le(h + 20, 4);
    const uint64_t count = get_le(h + 24, 8);
    if (count > CODEC_MAX_COUNT) return "count above 2^22";
    if (const char* e = codec_shape_error((size_t)count, n, abl, Lr, flags)) return e;
    if (R > count) return "raw_count above count";
    const CodecLayout l{(size_t)count, abl, Lr, (int)(flags & 1)};
    if (l.Sc() == 0 && R != count) return "ab_len != 1 but not every proof raw";
    if (l.bytes(R) != blob_bytes) return "blob size differs from the header's sections";
    info->count = (size_t)count; info->n = n; info->ab_len = abl; info->L_len = Lr;
    info->flags = flags; info->raw_count = R; info->bytes = blob_bytes;
    return nullptr;
}

// ------------------------------------------------------------------ the flat arrays
// hipbp_proof_batch's / hipbp_proof_out's arrays, for reading (encode) or writing (decode); taux, mu
// null without f.  V: the V that is encoded (the batch's Vp when it has one).
struct CodecArrays {
    ge* pt[5];   // V A S T1 T2
    fe *t, *c, *x, *taux, *mu, *a, *b;
    ge *L, *R;
};
// ... over a batch (own_V: the proofs' own V, Vp where the batch's V is a caller's; blinding: with
// its taux and mu, else null) and over a prover or decoder output
inline CodecArrays codec_arrays(const hipbp_proof_batch& b, bool own_V, bool blinding) {
    return CodecArrays{{(ge*)(own_V && b.Vp ? b.Vp : b.V), (ge*)b.A, (ge*)b.S, (ge*)b.T1, (ge*)b.T2},
                       (fe*)b.t, (fe*)b.c, (fe*)b.x, blinding ? (fe*)b.taux : nullptr, blinding ? (fe*)b.mu : nullptr,
                       (fe*)b.a, (fe*)b.b, (ge*)b.L, (ge*)b.R};
}
inline CodecArrays codec_arrays(const hipbp_proof_out& o, bool blinding) {
    return CodecArrays{{(ge*)o.V, (ge*)o.A, (ge*)o.S, (ge*)o.T1, (ge*)o.T2},
                       (fe*)o.t, (fe*)o.c, (fe*)o.x, blinding ? (fe*)o.taux : nullptr, blinding ? (fe*)o.mu : nullptr,
                       (fe*)o.a, (fe*)o.b, (ge*)o.L, (ge*)o.R};
}
BP_DEV ge* codec_point(const CodecArrays& A, const CodecLayout& l, size_t i, size_t q) {
    if (q < 5) return A.pt[q] + i;
    q -= 5;
    return q < l.Lr ? A.L + i * l.Lr + q : A.R + i * l.Lr + (q - l.Lr);
}

// 16-byte accesses: the flat side aligned, the blob side at 8 (on the host at any alignment)
BP_DEV u128 flat_ld(const void* p, size_t unit) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const u128*)p)[unit];
#else
    u128 r;
    memcpy(&r, (const uint8_t*)p + 16 * unit, 16);
    return r;
#endif
}
BP_DEV void flat_st(void* p, size_t unit, u128 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    ((u128*)p)[unit] = v;
#else
    memcpy((uint8_t*)p + 16 * unit, &v, 16);
#endif
}
BP_DEV fe fe_of(u128 a, u128 b) { return fe{{a.lo, a.hi, b.lo, b.hi}}; }
BP_DEV u128 blob_ld(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t* q = (const uint64_t*)p;
    return u128{q[0], q[1]};
#else
    u128 r;
    memcpy(&r, p, 16);
    return r;
#endif
}
BP_DEV void blob_st(uint8_t* p, u128 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t* q = (uint64_t*)p;
    q[0] = v.lo; q[1] = v.hi;
#else
    memcpy(p, &v, 16);
#endif
}

// ------------------------------------------------------------------ classify
BP_DEV bool fe_same(const fe& a, const fe& b) {
    return ((a.v[0] ^ b.v[0]) | (a.v[1] ^ b.v[1]) | (a.v[2] ^ b.v[2]) | (a.v[3] ^ b.v[3])) == 0;
}
// one point: Z limbs exactly (1, 0, 0, 0) and T limb for limb fe25519_mul(X, Y)
BP_DEV bool codec_point_compact(const ge* P) {
    u128 u[8];
    for (size_t k = 0; k < 8; k++) u[k] = flat_ld(P, k);
    return fe_same(fe_of(u[4], u[5]), fe_set(1)) && fe_same(fe_of(u[6], u[7]), fe_mul(fe_of(u[0], u[1]), fe_of(u[2], u[3])));
}
// one proof's scalars: ab_len = 1, a = t, c = t, b = (1, 0, 0, 0)
BP_DEV bool codec_scalars_compact(const CodecArrays& A, const CodecLayout& l, size_t i) {
    if (l.abl != 1) return false;
    const fe t = fe_of(flat_ld(A.t + i, 0), flat_ld(A.t + i, 1));
    return fe_same(fe_of(flat_ld(A.a + i, 0), flat_ld(A.a + i, 1)), t) &&
           fe_same(fe_of(flat_ld(A.c + i, 0), flat_ld(A.c + i, 1)), t) &&
           fe_same(fe_of(flat_ld(A.b + i, 0), flat_ld(A.b + i, 1)), fe_set(1));
}
// one proof: 0 compact, 1 raw
BP_DEV uint8_t codec_classify(const CodecArrays& A, const CodecLayout& l, size_t i) {
    if (!codec_scalars_compact(A, l, i)) return 1;
    for (size_t q = 0; q < l.npts(); q++)
        if (!codec_point_compact(codec_point(A, l, i, q))) return 1;
    return 0;
}

// ------------------------------------------------------------------ encode
// the field elements after the points, as 16-byte units: the compact slot's t x [taux mu], the raw
// record's t c x [taux mu] a[] b[]
BP_DEV u128 codec_tail_unit(const CodecArrays& A, const CodecLayout& l, size_t i, size_t w, bool raw) {
    const size_t e = w / 2, h = w % 2;
    const fe* src;
    if (!raw) {
        src = e == 0 ? A.t + i : e == 1 ? A.x + i : e == 2 ? A.taux + i : A.mu + i;
    } else {
        const size_t nf = 3 + 2 * (size_t)l.f;
        if (e < 3) src = e == 0 ? A.t + i : e == 1 ? A.c + i : A.x + i;
        else if (e < nf) src = e == 3 ? A.taux + i : A.mu + i;
        else if (e < nf + l.abl) src = A.a + i * l.abl + (e - nf);
        else src = A.b + i * l.abl + (e - nf - l.abl);
    }
    return flat_ld(src, h);
}
// unit w (of S_c / 16) of proof i's compact slot
BP_DEV u128 codec_compact_unit(const CodecArrays& A, const CodecLayout& l, size_t i, size_t w) {
    const size_t np = l.npts();
    if (w < 4 * np) return flat_ld(codec_point(A, l, i, w / 4), w % 4);   // X | Y: the point's first 64 bytes
    return codec_tail_unit(A, l, i, w - 4 * np, false);
}
// unit w (of S_r / 16) of proof i's raw record
BP_DEV u128 codec_raw_unit(const CodecArrays& A, const CodecLayout& l, size_t i, size_t w) {
    const size_t np = l.npts();
    if (w < 8 * np) return flat_ld(codec_point(A, l, i, w / 8), w % 8);
    return codec_tail_unit(A, l, i, w - 8 * np, true);
}
// proof i's compact slot (zeros for a raw proof) / its raw record at dst
BP_DEV void codec_write_compact(uint8_t* dst, const CodecArrays& A, const CodecLayout& l, size_t i, uint8_t kind) {
    for (size_t w = 0; w < l.Sc() / 16; w++) blob_st(dst + 16 * w, kind ? u128{0, 0} : codec_compact_unit(A, l, i, w));
}
BP_DEV void codec_write_raw(uint8_t* dst, const CodecArrays& A, const CodecLayout& l, size_t i) {
    for (size_t w = 0; w < l.Sr() / 16; w++) blob_st(dst + 16 * w, codec_raw_unit(A, l, i, w));
}

// ------------------------------------------------------------------ decode
// What a decoder reads: the four sections of a blob, or of a slice of one (proofs [base, base +
// count) and the raw records that belong to them), each with the number of whole entries that lie
// inside the bytes the caller holds.  Every index a body takes from the blob is checked against
// these before it is used.
struct BlobView {
    const uint8_t *kind, *compact, *rawidx, *raw;
    size_t count, R, base;                      // proofs, raw records, the proof index of entry 0
    size_t kind_n, compact_n, rawidx_n, raw_n;  // entries in range
};
BP_DEV size_t codec_fit(size_t bytes, size_t off, size_t each, size_t want) {
    if (bytes <= off || each == 0) return 0;
    const size_t n = (bytes - off) / each;
    return n < want ? n : want;
}
// the view of a whole blob of `bytes` bytes whose header gave l and R
BP_DEV BlobView codec_view(const uint8_t* blob, size_t bytes, const CodecLayout& l, size_t R) {
    BlobView v;
    v.kind = blob + l.o_kind(); v.compact = blob + l.o_compact(); v.rawidx = blob + l.o_rawidx(); v.raw = blob + l.o_raw(R);
    v.count = l.count; v.R = R; v.base = 0;
    v.kind_n = codec_fit(bytes, l.o_kind(), 1, l.count);
    v.compact_n = codec_fit(bytes, l.o_compact(), l.Sc(), l.count);
    v.rawidx_n = codec_fit(bytes, l.o_rawidx(), 4, R);
    v.raw_n = codec_fit(bytes, l.o_raw(R), l.Sr(), R);
    return v;
}
// the first j in [0, rawidx_n) with raw_index[j] >= key (raw_index ascending)
BP_DEV size_t codec_raw_lower(const uint8_t* rawidx, size_t n, uint64_t key) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (get_le(rawidx + 4 * mid, 4) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
BP_DEV void codec_read_tail(const uint8_t* src, const CodecArrays& A, const CodecLayout& l, size_t i, bool raw) {
    auto take = [&](fe* dst) {
        if (dst) { flat_st(dst, 0, blob_ld(src)); flat_st(dst, 1, blob_ld(src + 16)); }
        src += 32;
    };
    if (!raw) {
        const u128 t0 = blob_ld(src), t1 = blob_ld(src + 16), one{1, 0}, zero{0, 0};
        take(A.t + i);
        take(A.x + i);
        if (l.f) { take(A.taux ? A.taux + i : nullptr); take(A.mu ? A.mu + i : nullptr); }
        flat_st(A.a + i, 0, t0); flat_st(A.a + i, 1, t1);
        flat_st(A.c + i, 0, t0); flat_st(A.c + i, 1, t1);
        flat_st(A.b + i, 0, one); flat_st(A.b + i, 1, zero);
    } else {
        take(A.t + i); take(A.c + i); take(A.x + i);
        if (l.f) { take(A.taux ? A.taux + i : nullptr); take(A.mu ? A.mu + i : nullptr); }
        for (size_t k = 0; k < l.abl; k++) take(A.a + i * l.abl + k);
        for (size_t k = 0; k < l.abl; k++) take(A.b + i * l.abl + k);
    }
}
// Item q of proof i (view-relative) of the compact pass: q < npts its q-th point (Z = 1, T = X Y
// recomputed), q = npts its field elements.  Returns 1 when the proof's record is skipped by a
// failed check (counted once per proof, by the q = npts item): a kind out of range or above 1, a
// compact kind with no compact slot in range, or a raw kind that raw_index does not name.
BP_DEV unsigned codec_read_compact_item(const BlobView& v, const CodecArrays& A, const CodecLayout& l, size_t i,
                                        size_t q) {
    const size_t np = l.npts();
    const bool last = q == np;
    if (i >= v.kind_n) return last;
    const uint8_t k = v.kind[i];
    if (k > 1) return last;
    if (k == 1) {
        if (!last) return 0;
        const size_t j = codec_raw_lower(v.rawidx, v.rawidx_n, v.base + i);
        return !(j < v.rawidx_n && get_le(v.rawidx + 4 * j, 4) == v.base + i);
    }
    if (i >= v.compact_n) return last;
    const uint8_t* slot = v.compact + i * l.Sc();
    if (last) {
        codec_read_tail(slot + 64 * np, A, l, i, false);
        return 0;
    }
    ge* P = codec_point(A, l, i, q);
    u128 u[4];
    for (size_t k = 0; k < 4; k++) flat_st(P, k, u[k] = blob_ld(slot + 64 * q + 16 * k));
    const fe T = fe_mul(fe_of(u[0], u[1]), fe_of(u[2], u[3]));
    flat_st(P, 4, u128{1, 0}); flat_st(P, 5, u128{0, 0});
    flat_st(P, 6, u128{T.v[0], T.v[1]}); flat_st(P, 7, u128{T.v[2], T.v[3]});
    return 0;
}
// Item q of raw record j (view-relative) of the raw pass, the same items.  A record is skipped, and
// counted by its q = npts item, when its raw_index entry or its bytes are out of range, when the
// entry is not above its predecessor, names no proof of the view or names one whose kind is not 1.
BP_DEV unsigned codec_read_raw_item(const BlobView& v, const CodecArrays& A, const CodecLayout& l, size_t j, size_t q) {
    const size_t np = l.npts();
    const bool last = q == np;
    if (j >= v.rawidx_n || j >= v.raw_n) return last;
    const uint64_t idx = get_le(v.rawidx + 4 * j, 4);
    if (j > 0 && get_le(v.rawidx + 4 * (j - 1), 4) >= idx) return last;
    if (idx < v.base || idx - v.base >= v.count) return last;
    const size_t i = (size_t)(idx - v.base);
    if (i >= v.kind_n || v.kind[i] != 1) return last;
    const uint8_t* rec = v.raw + j * l.Sr();
    if (last) {
        codec_read_tail(rec + 128 * np, A, l, i, true);
        return 0;
    }
    ge* P = codec_point(A, l, i, q);
    for (size_t u = 0; u < 8; u++) flat_st(P, u, blob_ld(rec + 128 * q + 16 * u));
    return 0;
}

// ------------------------------------------------------------------ CPU encode / decode / parse
// The whole blob of the arrays' l.count proofs at `blob` (l.bound() bytes available); returns its size.
inline size_t codec_encode_cpu(uint8_t* blob, const CodecArrays& A, const CodecLayout& l, size_t n) {
    uint8_t* kind = blob + l.o_kind();
    memset(kind, 0, pad8(l.count));
    size_t R = 0;
    for (size_t i = 0; i < l.count; i++) R += kind[i] = codec_classify(A, l, i);
    uint8_t* ridx = blob + l.o_rawidx();
    memset(ridx, 0, pad8(4 * R));
    size_t j = 0;
    for (size_t i = 0; i < l.count; i++) {
        codec_write_compact(blob + l.o_compact() + i * l.Sc(), A, l, i, kind[i]);
        if (!kind[i]) continue;
        put_le(ridx + 4 * j, i, 4);
        codec_write_raw(blob + l.o_raw(R) + j * l.Sr(), A, l, i);
        j++;
    }
    codec_write_header(blob, l, n, R);
    return l.bytes(R);
}
// Every item of both passes over the view; returns the number of skipped records.
inline size_t codec_decode_cpu(const BlobView& v, const CodecArrays& A, const CodecLayout& l) {
    size_t bad = 0;
    for (size_t i = 0; i < v.count; i++)
        for (size_t q = 0; q <= l.npts(); q++) bad += codec_read_compact_item(v, A, l, i, q);
    for (size_t j = 0; j < v.R; j++)
        for (size_t q = 0; q <= l.npts(); q++) bad += codec_read_raw_item(v, A, l, j, q);
    return bad;
}
// Full validation of a host blob: the header, the exact size, every kind <= 1, R the number of
// kind-1 bytes, raw_index strictly ascending and naming exactly those proofs, zero padding and zero
// slots of raw proofs.  0: fine, else the reason.
inline const char* codec_parse(const uint8_t* blob, size_t bytes, hipbp_proof_blob_info* info) {
    if (!blob) return "null blob";
    if (const char* e = codec_parse_header(blob, bytes, info)) return e;
    const CodecLayout l = codec_layout(*info);
    const size_t R = info->raw_count;
    const uint8_t* kind = blob + l.o_kind();
    const uint8_t* ridx = blob + l.o_rawidx();
    size_t j = 0;
    for (size_t i = 0; i < l.count; i++) {
        if (kind[i] > 1) return "kind byte above 1";
        if (!kind[i]) continue;
        if (j >= R) return "more raw proofs than raw_count";
        if (get_le(ridx + 4 * j, 4) != i) return "raw_index does not name the raw proofs in ascending order";
        const uint8_t* slot = blob + l.o_compact() + i * l.Sc();
        for (size_t k = 0; k < l.Sc(); k++)
            if (slot[k]) return "non-zero compact slot of a raw proof";
        j++;
    }
    if (j != R) return "raw_count differs from the number of raw proofs";
    for (size_t k = l.count; k < pad8(l.count); k++)
        if (kind[k]) return "non-zero padding after kind";
    for (size_t k = 4 * R; k < pad8(4 * R); k++)
        if (ridx[k]) return "non-zero padding after raw_index";
    return nullptr;
}

// ------------------------------------------------------------------ the launches (bp_codec.hip)
// Encode: classify, scan, write; blk: the stream's block counts (CodecWs, bp_layout.h's BP_CODEC_BUFS).
void launch_codec_encode(const CodecArrays& A, const CodecLayout& l, size_t n, uint8_t* blob, const CodecWs& w,
                         uint64_t* bytes_out, hipStream_t s);
// Decode: the compact pass over v.count proofs, the raw pass over v.R records; *bad += the skipped.
void launch_codec_decode(const BlobView& v, const CodecArrays& A, const CodecLayout& l, uint32_t* bad, hipStream_t s);

}  // namespace bp

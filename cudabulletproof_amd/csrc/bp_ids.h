// bp_ids.h — proof ids and the batch Merkle root: the hashed messages and the per-lane
// bodies (internal to the library).  Pure like bp_codec.h: no HIP runtime calls.  The kernels of
// bp_ids.hip and the CPU paths of bp_api_blob.hip call exactly the functions below, so tests/ids_check.hip
// runs every one of them on a CPU, the malformed blobs under ASan + UBSan.
//
// All integers little-endian; a proof's record is what the blob stores for it (bp_codec.h):
//   hdr  = "hipbpProofIdV1" | u8 kind | u8 f | u32 n | u32 ab_len | u32 L_len | u32 0      (32 bytes)
//   id   = SHA-256(hdr | record)        compact: == 32 mod 64 bytes, raw: == 0 mod 64
//   leaf = SHA-256(0x00 | id)           node = SHA-256(0x01 | left | right)
//   root = RFC 6962 MTH over the ids as the leaf inputs; no ids: SHA-256("")
// The message is a sequence of 32-byte pieces at 32-byte offsets: piece 2j fills words 0..7 of the
// block, piece 2j + 1 fills words 8..15 and compresses; the two tails (a half-filled last block, a
// whole padding block) are the only other shapes, so no byte is placed at a run-time position and
// the state and the block stay in registers.
#pragma once
#include "bp_codec.h"
#include "sha256_dev.h"

namespace bp {

constexpr size_t ID_BYTES = 32;
constexpr size_t MERKLE_MAX_COUNT = (size_t)1 << 24;
constexpr size_t MERKLE_MAX_PATH = 22;   // entries of an audit path for count <= 2^22 (the header's bound)
constexpr int IDS_BLK = 256;             // lanes per block of every launch

// ------------------------------------------------------------------ SHA-256 over 32-byte pieces
#if !defined(__HIP_DEVICE_COMPILE__)
// the host form of sha_compress (sha256_dev.h's is device code): FIPS 180-4 §6.2.2
inline uint32_t ids_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline void ids_compress_host(uint32_t st[8], const uint32_t in[16]) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64], s[8];
    for (int i = 0; i < 16; i++) w[i] = in[i];
    for (int i = 16; i < 64; i++) {
        const uint32_t s0 = ids_ror(w[i - 15], 7) ^ ids_ror(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = ids_ror(w[i - 2], 17) ^ ids_ror(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    for (int i = 0; i < 8; i++) s[i] = st[i];
    for (int i = 0; i < 64; i++) {
        const uint32_t t1 = s[7] + (ids_ror(s[4], 6) ^ ids_ror(s[4], 11) ^ ids_ror(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[i] + w[i];
        const uint32_t t2 = (ids_ror(s[0], 2) ^ ids_ror(s[0], 13) ^ ids_ror(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
        for (int k = 7; k > 0; k--) s[k] = s[k - 1];
        s[4] += t1;
        s[0] = t1 + t2;
    }
    for (int i = 0; i < 8; i++) st[i] += s[i];
}
#endif

struct IdSha {
    uint32_t st[8];
    uint32_t b[16];   // the current block
};
BP_DEV void ids_compress(IdSha& h) {
#if defined(__HIP_DEVICE_COMPILE__)
    sha_compress(h.st, h.b);
#else
    ids_compress_host(h.st, h.b);
#endif
}
BP_DEV void ids_init(IdSha& h) {
    h.st[0] = 0x6a09e667; h.st[1] = 0xbb67ae85; h.st[2] = 0x3c6ef372; h.st[3] = 0xa54ff53a;
    h.st[4] = 0x510e527f; h.st[5] = 0x9b05688c; h.st[6] = 0x1f83d9ab; h.st[7] = 0x5be0cd19;
}
// the 32 message bytes of (a, b) as eight big-endian words at words W .. W + 7 of the block
template <int W>
BP_DEV void ids_piece(IdSha& h, u128 a, u128 b) {
    h.b[W + 0] = __builtin_bswap32((uint32_t)a.lo); h.b[W + 1] = __builtin_bswap32((uint32_t)(a.lo >> 32));
    h.b[W + 2] = __builtin_bswap32((uint32_t)a.hi); h.b[W + 3] = __builtin_bswap32((uint32_t)(a.hi >> 32));
    h.b[W + 4] = __builtin_bswap32((uint32_t)b.lo); h.b[W + 5] = __builtin_bswap32((uint32_t)(b.lo >> 32));
    h.b[W + 6] = __builtin_bswap32((uint32_t)b.hi); h.b[W + 7] = __builtin_bswap32((uint32_t)(b.hi >> 32));
}
BP_DEV void ids_even(IdSha& h, u128 a, u128 b) { ids_piece<0>(h, a, b); }                    // piece 2j
BP_DEV void ids_odd(IdSha& h, u128 a, u128 b) { ids_piece<8>(h, a, b); ids_compress(h); }    // piece 2j + 1
// the tails of a message of `pieces` 32-byte pieces: after an even piece the block is half full,
// after an odd one the padding takes a block of its own
BP_DEV void ids_finish(IdSha& h, uint64_t pieces) {
    const uint64_t bits = pieces * 256;
    if (pieces & 1) {
        h.b[8] = 0x80000000u;
#pragma unroll
        for (int k = 9; k < 14; k++) h.b[k] = 0;
    } else {
        h.b[0] = 0x80000000u;
#pragma unroll
        for (int k = 1; k < 14; k++) h.b[k] = 0;
    }
    h.b[14] = (uint32_t)(bits >> 32);
    h.b[15] = (uint32_t)bits;
    ids_compress(h);
}

// a digest's 32 bytes (its state words big-endian) at a 4-byte aligned address; on the host at any
BP_DEV void ids_store(uint8_t* p, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 0; k < 8; k++) ((uint32_t*)p)[k] = __builtin_bswap32(w[k]);
#else
    for (int k = 0; k < 8; k++) {
        const uint32_t v = __builtin_bswap32(w[k]);
        memcpy(p + 4 * k, &v, 4);
    }
#endif
}
BP_DEV void ids_load(const uint8_t* p, uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = __builtin_bswap32(((const uint32_t*)p)[k]);
#else
    for (int k = 0; k < 8; k++) {
        uint32_t v;
        memcpy(&v, p + 4 * k, 4);
        w[k] = __builtin_bswap32(v);
    }
#endif
}
BP_DEV void ids_store_zero(uint8_t* p) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ids_store(p, z);
}

// ------------------------------------------------------------------ a proof's id
// hdr as the message's piece 0
BP_DEV void ids_header(IdSha& h, uint8_t kind, const CodecLayout& l, size_t n) {
    h.b[0] = 0x68697062u;                                                  // "hipb"
    h.b[1] = 0x7050726Fu;                                                  // "pPro"
    h.b[2] = 0x6F664964u;                                                  // "ofId"
    h.b[3] = 0x56310000u | ((uint32_t)kind << 8) | (uint32_t)(l.f & 1);    // "V1" kind f
    h.b[4] = __builtin_bswap32((uint32_t)n);
    h.b[5] = __builtin_bswap32((uint32_t)l.abl);
    h.b[6] = __builtin_bswap32((uint32_t)l.Lr);
    h.b[7] = 0;
}
// SHA-256(hdr | the record's P pieces); piece(r, a, b) gives piece r as two 16-byte units.  The next
// pair of pieces is taken before the current one is compressed, so its loads run under the rounds.
template <class Piece>
BP_DEV void ids_hash_record(uint8_t kind, const CodecLayout& l, size_t n, size_t P, const Piece& piece, uint32_t digest[8]) {
    IdSha h;
    ids_init(h);
    ids_header(h, kind, l, n);
    const size_t pairs = P / 2;
    u128 c[4], nx[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (pairs) { piece(0, nx[0], nx[1]); piece(1, nx[2], nx[3]); }
    for (size_t j = 0; j < pairs; j++) {
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = nx[k];
        if (j + 1 < pairs) { piece(2 * j + 2, nx[0], nx[1]); piece(2 * j + 3, nx[2], nx[3]); }
        ids_odd(h, c[0], c[1]);
        ids_even(h, c[2], c[3]);
    }
    if (P & 1) {
        piece(P - 1, c[0], c[1]);
        ids_odd(h, c[0], c[1]);
    }
    ids_finish(h, P + 1);
#pragma unroll
    for (int k = 0; k < 8; k++) digest[k] = h.st[k];
}
// the pieces of a record: compact S_c / 32, raw S_r / 32
BP_DEV size_t ids_pieces(const CodecLayout& l, uint8_t kind) { return (kind ? l.Sr() : l.Sc()) / 32; }

// Proof i of the flat arrays: classified as the encoder does, its record enumerated in the encoder's
// unit order.  The id at out (32 bytes); returns the kind.
BP_DEV uint8_t ids_flat_proof(const CodecArrays& A, const CodecLayout& l, size_t n, size_t i, uint8_t* out) {
    const uint8_t kind = codec_classify(A, l, i);
    uint32_t d[8];
    if (kind)
        ids_hash_record(kind, l, n, ids_pieces(l, 1), [&](size_t r, u128& a, u128& b) {
            a = codec_raw_unit(A, l, i, 2 * r); b = codec_raw_unit(A, l, i, 2 * r + 1); }, d);
    else
        ids_hash_record(kind, l, n, ids_pieces(l, 0), [&](size_t r, u128& a, u128& b) {
            a = codec_compact_unit(A, l, i, 2 * r); b = codec_compact_unit(A, l, i, 2 * r + 1); }, d);
    ids_store(out, d);
    return kind;
}

// Proof i (view-relative) of a blob: its kind byte, then its compact slot or the raw record that
// raw_index names for it (binary search), under the decoder's checks: a kind out of range or above 1,
// a compact kind with no slot in range, a raw kind whose raw_index entry or record is out of range,
// is missing, or is not above its predecessor.  A record that fails gets the all-zero id; returns 1
// for it, else 0.
BP_DEV unsigned ids_blob_proof(const BlobView& v, const CodecLayout& l, size_t n, size_t i, uint8_t* out) {
    const uint8_t* rec = nullptr;
    uint8_t kind = 0;
    if (i < v.kind_n && (kind = v.kind[i]) <= 1) {
        if (kind == 0) {
            if (i < v.compact_n && l.Sc()) rec = v.compact + i * l.Sc();
        } else {
            const uint64_t key = v.base + i;
            const size_t j = codec_raw_lower(v.rawidx, v.rawidx_n, key);
            if (j < v.rawidx_n && j < v.raw_n && get_le(v.rawidx + 4 * j, 4) == key &&
                (j == 0 || get_le(v.rawidx + 4 * (j - 1), 4) < key))
                rec = v.raw + j * l.Sr();
        }
    }
    if (!rec) {
        ids_store_zero(out);
        return 1;
    }
    uint32_t d[8];
    ids_hash_record(kind, l, n, ids_pieces(l, kind), [&](size_t r, u128& a, u128& b) {
        a = blob_ld(rec + 32 * r); b = blob_ld(rec + 32 * r + 16); }, d);
    ids_store(out, d);
    return 0;
}

// ------------------------------------------------------------------ the Merkle tree (RFC 6962 §2.1)
// digests as their eight state words.  leaf: one block, node: two
BP_DEV void merkle_leaf(const uint32_t id[8], uint32_t out[8]) {
    IdSha h;
    ids_init(h);
    h.b[0] = id[0] >> 8;   // 0x00 | id
#pragma unroll
    for (int k = 1; k < 8; k++) h.b[k] = (id[k - 1] << 24) | (id[k] >> 8);
    h.b[8] = (id[7] << 24) | 0x00800000u;
#pragma unroll
    for (int k = 9; k < 15; k++) h.b[k] = 0;
    h.b[15] = 33 * 8;
    ids_compress(h);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = h.st[k];
}
BP_DEV void merkle_node(const uint32_t l[8], const uint32_t r[8], uint32_t out[8]) {
    IdSha h;
    ids_init(h);
    h.b[0] = 0x01000000u | (l[0] >> 8);   // 0x01 | left | right
#pragma unroll
    for (int k = 1; k < 8; k++) h.b[k] = (l[k - 1] << 24) | (l[k] >> 8);
    h.b[8] = (l[7] << 24) | (r[0] >> 8);
#pragma unroll
    for (int k = 1; k < 8; k++) h.b[8 + k] = (r[k - 1] << 24) | (r[k] >> 8);
    ids_compress(h);
    h.b[0] = (r[7] << 24) | 0x00800000u;
#pragma unroll
    for (int k = 1; k < 15; k++) h.b[k] = 0;
    h.b[15] = 65 * 8;
    ids_compress(h);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = h.st[k];
}
BP_DEV void merkle_empty(uint32_t out[8]) {   // SHA-256("")
    IdSha h;
    ids_init(h);
    ids_finish(h, 0);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = h.st[k];
}
BP_DEV size_t merkle_up(size_t m) { return (m + 1) >> 1; }   // the nodes of the level above m nodes
// Node k of the level above the m nodes at `in`: the pair (2k, 2k + 1) hashed, an unpaired last node
// promoted unchanged.  LEAF: `in` holds ids, each hashed as a leaf first (level 0 fused).
template <bool LEAF>
BP_DEV void merkle_level_in(const uint8_t* in, size_t j, uint32_t w[8]) {
    uint32_t id[8];
    ids_load(in + ID_BYTES * j, LEAF ? id : w);
    if (LEAF) merkle_leaf(id, w);
}
template <bool LEAF>
BP_DEV void merkle_level_node(const uint8_t* in, size_t m, size_t k, uint8_t* out) {
    uint32_t a[8], b[8], d[8];
    merkle_level_in<LEAF>(in, 2 * k, a);
    if (2 * k + 1 < m) {
        merkle_level_in<LEAF>(in, 2 * k + 1, b);
        merkle_node(a, b, d);
        ids_store(out + ID_BYTES * k, d);
    } else {
        ids_store(out + ID_BYTES * k, a);
    }
}

// ------------------------------------------------------------------ CPU root / path / verify
// Every level of the tree over count >= 1 ids through the bodies above: lv[0] the leaf hashes,
// lv.back() the root alone.  `lv` is any container of byte vectors (std::vector<std::vector<uint8_t>>).
template <class Levels>
inline void merkle_levels_cpu(const uint8_t* ids, size_t count, Levels& lv) {
    lv.clear();
    lv.emplace_back(count * ID_BYTES);
    for (size_t i = 0; i < count; i++) {
        uint32_t a[8], d[8];
        ids_load(ids + ID_BYTES * i, a);
        merkle_leaf(a, d);
        ids_store(lv[0].data() + ID_BYTES * i, d);
    }
    for (size_t m = count; m > 1; m = merkle_up(m)) {
        lv.emplace_back(merkle_up(m) * ID_BYTES);
        const size_t top = lv.size() - 1;
        for (size_t k = 0; k < merkle_up(m); k++) merkle_level_node<false>(lv[top - 1].data(), m, k, lv[top].data());
    }
}
// the audit path of `index` (RFC 6962 §2.1.1), bottom-up, from the levels; returns its length
template <class Levels>
inline size_t merkle_path_cpu(const Levels& lv, size_t count, size_t index, uint8_t* path) {
    size_t len = 0, i = index, lev = 0;
    for (size_t m = count; m > 1; m = merkle_up(m), i >>= 1, lev++) {
        if (!(i & 1) && i == m - 1) continue;   // promoted: no entry
        memcpy(path + ID_BYTES * len++, lv[lev].data() + ID_BYTES * (i ^ 1), ID_BYTES);
    }
    return len;
}
// the root recomputed from (id, index, count, path): true when exactly path_len entries are consumed
// and the result is `root`
inline bool merkle_verify_cpu(const uint8_t* id, size_t index, size_t count, const uint8_t* path, size_t path_len,
                              const uint8_t* root) {
    if (index >= count) return false;
    uint32_t h[8], s[8], d[8];
    ids_load(id, s);
    merkle_leaf(s, h);
    size_t used = 0, i = index;
    for (size_t m = count; m > 1; m = merkle_up(m), i >>= 1) {
        if (!(i & 1) && i == m - 1) continue;
        if (used == path_len) return false;
        ids_load(path + ID_BYTES * used++, s);
        if (i & 1) merkle_node(s, h, d);
        else merkle_node(h, s, d);
        for (int k = 0; k < 8; k++) h[k] = d[k];
    }
    uint8_t got[ID_BYTES];
    ids_store(got, h);
    return used == path_len && memcmp(got, root, ID_BYTES) == 0;
}

// ------------------------------------------------------------------ the launches (bp_ids.hip)
struct IdsWs {
    uint8_t *ping, *pong;   // the Merkle levels 1, 3, ... and 2, 4, ...
    uint32_t* bad;          // hipbp_blob_proof_ids: the failed records of each block
};
// ids[32 i ..) = the id of proof i of the arrays, kind[i] its kind when kind is not null
void launch_proof_ids(const CodecArrays& A, const CodecLayout& l, size_t n, uint8_t* ids, uint8_t* kind, hipStream_t s);
// ... of proof i of the view; *bad = the records that failed their checks
void launch_blob_ids(const BlobView& v, const CodecLayout& l, size_t n, uint8_t* ids, const IdsWs& w, uint32_t* bad,
                     hipStream_t s);
// root[0 .. 32) = the root over count ids, level by level through w.ping / w.pong
void launch_merkle_root(const uint8_t* ids, size_t count, uint8_t* root, const IdsWs& w, hipStream_t s);

}  // namespace bp

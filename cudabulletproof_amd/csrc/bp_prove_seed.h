// bp_prove_seed.h — the seeded prover's nonce derivation: every random scalar of a
// batch of range proofs from one 32-byte secret seed, by SHA-256.  Byte-exact contract, all
// integers little-endian:
//
//   key_p  = SHA-256("hipbpProverKeyV1" || seed[32] || v_p || gamma_p || LE64(index_base + p) || LE32(n))
//   d      = SHA-256("hipbpProverRndV1" || key_p || LE32(slot))
//   d[0] &= 0xF8; d[31] &= 0x7F; d[31] |= 0x40        (generate_random_scalar's masks, rp.cu:153-159)
//   scalar = d as 4 LE u64 limbs
//
// v_p, gamma_p: the 32 bytes of the four u64 limbs as stored (not canonicalised); the index sum
// wraps mod 2^64.  slot 0..3 = alpha, rho, tau1, tau2 (the order of hipbp_prove_input::rnd),
// 4 + i = sL[i], 4 + n + i = sR[i].
//
// The accepted prover's retries draw fresh scalars for attempt a >= 1 of proof p from
//
//   key_{p,a} = SHA-256("hipbpProverTryV1" || key_p || LE32(a))          (52 bytes, one block)
//
// in place of key_p (key_{p,0} = key_p): scalar(p, a, slot) is seed_scalar on key_{p,a}.
//
// Both layouts are __host__ __device__ and written once.  Every field of both messages starts on
// a 4-byte boundary, so a message is a sequence of big-endian words at compile-time positions.
// In the device pass the context is sha256_dev.h's register-resident `shaw` (shaw_put,
// shaw_final_limbs, sha_compress: state and block stay in VGPRs).  Those are __device__-only and
// rotate with alignbit, so the host pass restates the word-aligned subset of them here with a
// portable rotate; sha256_dev.h itself is unchanged.  tests/test_prove_seed_host.py checks the
// host pass against hashlib, the -m gpu tests check the device pass.
#pragma once
#include "ge25519_dev.h"   // sha256_dev.h's challenge messages take points
#include "sha256_dev.h"
#include "bp_kernels.h"    // ProveOut

namespace bp {

#define BP_SEED_HD __host__ __device__ __forceinline__

// the seed as the eight big-endian message words of its 32 bytes: a kernel argument by value
struct SeedWords {
    uint32_t w[8];
};
inline SeedWords seed_words(const uint8_t seed32[32]) {
    SeedWords s;
    for (int k = 0; k < 8; k++)
        s.w[k] = (uint32_t)seed32[4 * k] << 24 | (uint32_t)seed32[4 * k + 1] << 16 | (uint32_t)seed32[4 * k + 2] << 8 |
                 (uint32_t)seed32[4 * k + 3];
    return s;
}

#if defined(__HIP_DEVICE_COMPILE__)
using seedw = shaw;
#else
struct seedw {
    uint32_t st[8];
    uint32_t b[16];
};
inline uint32_t seed_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// FIPS 180-4 §6.2.2, the host pass's compression function
inline void seed_compress_host(uint32_t st[8], const uint32_t in[16]) {
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
    for (int i = 0; i < 16; i++) w[i] = in[i];
    for (int i = 16; i < 64; i++) {
        uint32_t s0 = seed_ror(w[i - 15], 7) ^ seed_ror(w[i - 15], 18) ^ (w[i - 15] >> 3);
        uint32_t s1 = seed_ror(w[i - 2], 17) ^ seed_ror(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; i++) {
        uint32_t t1 = h + (seed_ror(e, 6) ^ seed_ror(e, 11) ^ seed_ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        uint32_t t2 = (seed_ror(a, 2) ^ seed_ror(a, 13) ^ seed_ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
#endif

BP_SEED_HD void seed_init(seedw& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    shaw_init(c);
#else
    c.st[0] = 0x6a09e667; c.st[1] = 0xbb67ae85; c.st[2] = 0x3c6ef372; c.st[3] = 0xa54ff53a;
    c.st[4] = 0x510e527f; c.st[5] = 0x9b05688c; c.st[6] = 0x1f83d9ab; c.st[7] = 0x5be0cd19;
#endif
}

// one big-endian message word at byte offset P (a multiple of 4); the word that fills a block
// compresses it
template <int P>
BP_SEED_HD void seed_put(seedw& c, uint32_t w) {
    static_assert(P % 4 == 0, "the seeded prover's messages are word-aligned");
#if defined(__HIP_DEVICE_COMPILE__)
    shaw_put<P>(c, w);
#else
    c.b[(P >> 2) & 15] = w;
    if ((P & 63) == 60) seed_compress_host(c.st, c.b);
#endif
}

// padding and length of an L-byte message (L a multiple of 4); the digest as 4 LE u64 limbs
template <int L>
BP_SEED_HD void seed_final(seedw& c, uint64_t out[4]) {
    static_assert(L % 4 == 0, "the seeded prover's messages are word-aligned");
#if defined(__HIP_DEVICE_COMPILE__)
    shaw_final_limbs<L>(c, out);
#else
    seed_put<L>(c, 0x80000000u);
    constexpr int w0 = ((L + 4) & 63) / 4;   // first unassigned word of the current block
    if (w0 > 14) {                           // no room for the length: a block of its own
        for (int k = w0; k < 16; k++) c.b[k] = 0;
        seed_compress_host(c.st, c.b);
        for (int k = 0; k < 14; k++) c.b[k] = 0;
    } else {
        for (int k = w0; k < 14; k++) c.b[k] = 0;
    }
    c.b[14] = 0;
    c.b[15] = (uint32_t)L * 8u;
    seed_compress_host(c.st, c.b);
    for (int i = 0; i < 4; i++)
        out[i] = (uint64_t)__builtin_bswap32(c.st[2 * i]) | ((uint64_t)__builtin_bswap32(c.st[2 * i + 1]) << 32);
#endif
}

// ------------------------------------------------------------------ the layouts (both passes)
// a 16-character tag at byte offset P
template <int P, int I = 0>
BP_SEED_HD void seed_tag(seedw& c, const char (&s)[17]) {
    if constexpr (I < 16) {
        seed_put<P + I>(c, (uint32_t)(uint8_t)s[I] << 24 | (uint32_t)(uint8_t)s[I + 1] << 16 |
                               (uint32_t)(uint8_t)s[I + 2] << 8 | (uint32_t)(uint8_t)s[I + 3]);
        seed_tag<P, I + 4>(c, s);
    }
}
// a little-endian u32 at byte offset P
template <int P>
BP_SEED_HD void seed_le32(seedw& c, uint32_t x) {
    seed_put<P>(c, __builtin_bswap32(x));
}
// 4 little-endian u64 limbs (32 bytes as stored) at byte offset P
template <int P>
BP_SEED_HD void seed_limbs(seedw& c, const uint64_t v[4]) {
    seed_le32<P + 0>(c, (uint32_t)v[0]);  seed_le32<P + 4>(c, (uint32_t)(v[0] >> 32));
    seed_le32<P + 8>(c, (uint32_t)v[1]);  seed_le32<P + 12>(c, (uint32_t)(v[1] >> 32));
    seed_le32<P + 16>(c, (uint32_t)v[2]); seed_le32<P + 20>(c, (uint32_t)(v[2] >> 32));
    seed_le32<P + 24>(c, (uint32_t)v[3]); seed_le32<P + 28>(c, (uint32_t)(v[3] >> 32));
}

// key_p: 124 bytes, three compressions.  index = index_base + p, already wrapped mod 2^64.
BP_SEED_HD void seed_key(uint64_t key[4], const SeedWords& seed, const uint64_t v[4], const uint64_t gamma[4],
                         uint64_t index, uint32_t n) {
    seedw c;
    seed_init(c);
    seed_tag<0>(c, "hipbpProverKeyV1");
    seed_put<16>(c, seed.w[0]); seed_put<20>(c, seed.w[1]); seed_put<24>(c, seed.w[2]); seed_put<28>(c, seed.w[3]);
    seed_put<32>(c, seed.w[4]); seed_put<36>(c, seed.w[5]); seed_put<40>(c, seed.w[6]); seed_put<44>(c, seed.w[7]);
    seed_limbs<48>(c, v);
    seed_limbs<80>(c, gamma);
    seed_le32<112>(c, (uint32_t)index);
    seed_le32<116>(c, (uint32_t)(index >> 32));
    seed_le32<120>(c, n);
    seed_final<124>(c, key);
}

// one scalar: 52 bytes, one compression, then generate_random_scalar's masks
BP_SEED_HD void seed_scalar(uint64_t out[4], const uint64_t key[4], uint32_t slot) {
    seedw c;
    seed_init(c);
    seed_tag<0>(c, "hipbpProverRndV1");
    seed_limbs<16>(c, key);
    seed_le32<48>(c, slot);
    seed_final<52>(c, out);
    out[0] &= ~7ull;                                                         // d[0] &= 0xF8
    out[3] = (out[3] & 0x7FFFFFFFFFFFFFFFull) | 0x4000000000000000ull;       // d[31] &= 0x7F; d[31] |= 0x40
}

// key_{p,a}, the key of attempt a of a proof: key_p itself for a = 0, else 52 bytes, one compression
BP_SEED_HD void seed_try_key(uint64_t out[4], const uint64_t key[4], uint32_t a) {
    if (a == 0) {
        out[0] = key[0]; out[1] = key[1]; out[2] = key[2]; out[3] = key[3];
        return;
    }
    seedw c;
    seed_init(c);
    seed_tag<0>(c, "hipbpProverTryV1");
    seed_limbs<16>(c, key);
    seed_le32<48>(c, a);
    seed_final<52>(c, out);
}

// ------------------------------------------------------------------ the derive kernels (bp_prove_seed.hip)
// keys[B] (workspace), then rnd[B*4], sL[B*n], sR[B*n] in hipbp_prove_input's layout; B (2n + 4) < 2^32.
// Asynchronous on s; the seed travels in the kernel arguments.
void launch_seed_derive(const SeedWords& seed, const fe* v, const fe* gamma, uint64_t index_base, uint32_t B,
                        uint32_t n, fe* keys, fe* sL, fe* sR, fe* rnd, hipStream_t s);
// ... its two launches alone: keys[B], and the scalars of B proofs from keys[B] (key_p or try keys)
void launch_seed_keys(const SeedWords& seed, const fe* v, const fe* gamma, uint64_t index_base, uint32_t B, uint32_t n,
                      fe* keys, hipStream_t s);
void launch_seed_scalars(const fe* keys, uint32_t B, uint32_t n, fe* sL, fe* sR, fe* rnd, hipStream_t s);

// ------------------------------------------------------------------ the accepted prover's kernels
// out[j] = key_{list[j], a} from keys[] (the batch's key_p), j < m: the retry loop's form.
void launch_try_keys_list(const fe* keys, const uint32_t* list, uint32_t m, uint32_t a, fe* out, hipStream_t s);
// out[p] = key_{p, attempt[p]}, p < B (attempt 0 copies the key): the audit entry point's form.
void launch_try_keys_at(const fe* keys, const uint8_t* attempt, uint32_t B, fe* out, hipStream_t s);

// One round's verdicts.  ok[m], valid[m]: the verifier's verdicts and the prover's valid flags over
// the round's proofs, proof i of the round being proof src[i] of the batch (src null: i itself, the
// whole batch in round 1).  A proof with valid and ok is accepted: attempts[p] = round.  One with
// valid and not ok is rejected; round 1 also writes attempts[p] = 0 for every proof it does not
// accept.  Two steps with the host's read of *cnt between them:
//   launch_accept_count: attempts, the rejected proofs per block of 256 into blk[], their exclusive
//     scan in place and the total into *cnt;
//   launch_accept_fill: list[k] = the k-th rejected proof's batch index p, ascending, and its
//     v[p] | gamma[p] gathered into cv[k], cg[k], for k < *cnt.
// Every output is a function of ok, valid and src alone: no atomics, no launch-to-launch order.
constexpr uint32_t ACCEPT_BLK = 256;   // proofs per block (the size of blk[] follows: bp_layout.h)
// the loop's workspace (buffers and sizes: bp_layout.h, BP_ACCEPT_BUFS)
struct AcceptWs {
    uint8_t* ok;         // the round's verdicts
    uint32_t *blk, *cnt;
    uint32_t* list[2];   // the rejected proofs' batch indices, read and written in turn
    fe *v, *gamma, *keys, *scal;
    uint8_t* out;        // the retried proofs, an OutLayout
};
void launch_accept_count(const uint8_t* ok, const uint8_t* valid, const uint32_t* src, uint32_t m, uint32_t round,
                         uint8_t* attempts, uint32_t* blk, uint32_t* cnt, hipStream_t s);
void launch_accept_fill(const uint8_t* ok, const uint8_t* valid, const uint32_t* src, uint32_t m, const uint32_t* blk,
                        const fe* v, const fe* gamma, uint32_t* list, fe* cv, fe* cg, hipStream_t s);

// The proofs of a compact sub-batch (src: OutLayout::view with c = m, so the five point arrays, the
// seven scalar arrays and L | R each lie back to back at stride m) into rows list[j] of the caller's
// output, all of hipbp_proof_out's fields, in 16-byte pieces.  m (54 + 16 Lr) < 2^32.
void launch_accept_scatter(const ProveOut& src, const ProveOut& dst, const uint32_t* list, uint32_t m, uint32_t Lr,
                           hipStream_t s);

}  // namespace bp

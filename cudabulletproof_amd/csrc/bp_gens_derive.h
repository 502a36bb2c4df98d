// bp_gens_derive.h — generators derived from 32-byte seeds: the two lane bodies and the
// launches over them (internal to the library).  Pure like bp_ids.h: no HIP runtime calls.  The
// kernels of bp_gens_derive.hip and the CPU entry points call exactly the functions below, so
// tests/gens_derive_check.hip runs both on a CPU, under ASan + UBSan too.
//
// The rule is the reference test driver's (complete_bulletproof_test.cu:33-109), bit for bit:
//   vector form, point i:  X = le(SHA-256(seed | BE32(i)))   Y = le(SHA-256(the 32 bytes of X))
//                          Z = 1                             T = fe25519_mul(X, Y)
//   single form (g, h):    X = le(SHA-256(seed))             Y = Z = 1     T = fe25519_mul(X, 1)
// le() is a plain little-endian load of the digest: bit 255 is kept, nothing is reduced.  T is a
// product in the reference's arithmetic, also in the single form (X * 1 != X when X has bit 255).
// Only the low 32 bits of i are hashed, so the entry points require first + count <= 2^32.
//
// Every hash is one compression of a fixed layout, so no byte is placed at a run-time position and
// the state and the block stay in registers:
//   seed | BE32(i):  words 0..7 the seed, 8 the index, 9 the padding bit, 15 = 288 bits
//   digest / seed:   words 0..7 the message, 8 the padding bit, 15 = 256 bits
// The first digest's state words are the second message's words as they are; bytes are swapped only
// where X and Y are formed.
#pragma once
#include "bp_ids.h"
#include "ge25519_dev.h"

namespace bp {

constexpr int GENS_BLK = 256;                        // lanes per block of both launches
constexpr uint64_t GENS_INDEX_END = 1ull << 32;      // first + count may reach it, not pass it

// a seed's 32 bytes as the eight big-endian message words they are hashed as
struct GenSeed {
    uint32_t w[8];
};
inline GenSeed gens_seed_words(const uint8_t seed[32]) {
    GenSeed s;
    ids_load(seed, s.w);
    return s;
}

// a digest's 32 bytes (its state words big-endian) loaded as four little-endian limbs
BP_DEV fe gens_fe_of_digest(const uint32_t st[8]) {
    fe r;
#pragma unroll
    for (int k = 0; k < 4; k++)
        r.v[k] = (uint64_t)__builtin_bswap32(st[2 * k]) | ((uint64_t)__builtin_bswap32(st[2 * k + 1]) << 32);
    return r;
}
// SHA-256 of the 32 bytes in h.b[0..7]; the digest in h.st
BP_DEV void gens_hash32(IdSha& h) {
    ids_init(h);
    h.b[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 15; k++) h.b[k] = 0;
    h.b[15] = 256;
    ids_compress(h);
}

BP_DEV ge derive_base_point(const GenSeed& seed, uint32_t index) {
    IdSha h;
    ids_init(h);
#pragma unroll
    for (int k = 0; k < 8; k++) h.b[k] = seed.w[k];
    h.b[8] = index;
    h.b[9] = 0x80000000u;
#pragma unroll
    for (int k = 10; k < 15; k++) h.b[k] = 0;
    h.b[15] = 288;
    ids_compress(h);
    ge p;
    p.X = gens_fe_of_digest(h.st);
#pragma unroll
    for (int k = 0; k < 8; k++) h.b[k] = h.st[k];
    gens_hash32(h);
    p.Y = gens_fe_of_digest(h.st);
    p.Z = fe_set(1);
    p.T = fe_mul(p.X, p.Y);
    return p;
}

BP_DEV ge derive_single_point(const GenSeed& seed) {
    IdSha h;
#pragma unroll
    for (int k = 0; k < 8; k++) h.b[k] = seed.w[k];
    gens_hash32(h);
    ge p;
    p.X = gens_fe_of_digest(h.st);
    p.Y = fe_set(1);
    p.Z = fe_set(1);
    p.T = fe_mul(p.X, p.Y);
    return p;
}

// ------------------------------------------------------------------ the launches (bp_gens_derive.hip)
// out[k] = point first + k of the seed's vector, k < count (first + count <= 2^32)
void launch_derive_base_points(ge* out, const GenSeed& seed, uint64_t first, uint64_t count, hipStream_t s);
// out[0] = the seed's single point
void launch_derive_single_point(ge* out, const GenSeed& seed, hipStream_t s);

}  // namespace bp

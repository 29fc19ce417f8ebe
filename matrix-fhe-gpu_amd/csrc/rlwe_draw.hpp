// rlwe_draw.hpp -- the seeded draws of the RLWE client side (rlwe.hip; include/mfhe.h mfhe_rlwe_*), one definition for
// host and device: the ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter), the nonce layout, and
// the maps from a block's words to a uniform residue, a ternary digit and a centred-binomial noise value.  Integer
// arithmetic only, standard library only (tests/cpp/rlwe_draw_main.cpp includes this file with a host compiler alone).
//
//   key    : the caller's 256-bit seed, eight little-endian words
//   nonce  : word 0 = stream | limb << 8 (limb: the row's limb index in the context for the mask, 0 for every other
//            stream), words 1 and 2 = the low and high halves of the 64-bit polynomial id
//   mask   : coefficient i is block i >> 2, words 4 (i & 3) .. 4 (i & 3) + 3 as a little-endian 128-bit integer, reduced
//            mod q (bias below q / 2^128)
//   small  : coefficient i is block i >> 3, the 64-bit word w = out[2 k] | out[2 k + 1] << 32, k = i & 7, the same on
//            every row; ternary floor(3 w / 2^64) - 1; noise popcount(w & (2^21 - 1)) - popcount((w >> 21) & (2^21 - 1)),
//            variance 10.5, |e| <= 21
// No draw branches on or indexes memory by a sampled value.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MFHE_RLWE_HD __host__ __device__
#else
#define MFHE_RLWE_HD
#endif

namespace mfhe {

enum {
    kRlweMask = 1,        // uniform a
    kRlweNoise = 2,       // noise e
    kRlweSecret = 3,      // ternary secret
    kRlweEphemeral = 4,   // ternary u
    kRlweNoise0 = 5,      // public-key encryption noise 0
    kRlweNoise1 = 6,      // public-key encryption noise 1
};
constexpr int kRlweNoiseBits = 21;   // the centred binomial's half width: |e| <= 21

MFHE_RLWE_HD inline bool rlwe_stream_is_small(int stream) { return stream >= kRlweNoise && stream <= kRlweNoise1; }
MFHE_RLWE_HD inline bool rlwe_stream_is_ternary(int stream) { return stream == kRlweSecret || stream == kRlweEphemeral; }

MFHE_RLWE_HD inline uint32_t rlwe_rotl(uint32_t x, int n) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateleft32)
    return __builtin_rotateleft32(x, (uint32_t)n);
#else
    return (x << n) | (x >> (32 - n));
#endif
#else
    return (x << n) | (x >> (32 - n));
#endif
}

#define MFHE_RLWE_QR(a, b, c, d)              \
    do {                                      \
        a += b; d ^= a; d = rlwe_rotl(d, 16); \
        c += d; b ^= c; b = rlwe_rotl(b, 12); \
        a += b; d ^= a; d = rlwe_rotl(d, 8);  \
        c += d; b ^= c; b = rlwe_rotl(b, 7);  \
    } while (0)

// RFC 8439 section 2.3: the 16 output words of (key, counter, nonce)
MFHE_RLWE_HD inline void chacha20_block(const uint32_t (&key)[8], uint32_t counter, const uint32_t (&nonce)[3],
                                        uint32_t (&out)[16]) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                             key[4],      key[5],      key[6],      key[7],      counter, nonce[0], nonce[1], nonce[2]};
    uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
    uint32_t x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        MFHE_RLWE_QR(x0, x4, x8, x12);
        MFHE_RLWE_QR(x1, x5, x9, x13);
        MFHE_RLWE_QR(x2, x6, x10, x14);
        MFHE_RLWE_QR(x3, x7, x11, x15);
        MFHE_RLWE_QR(x0, x5, x10, x15);
        MFHE_RLWE_QR(x1, x6, x11, x12);
        MFHE_RLWE_QR(x2, x7, x8, x13);
        MFHE_RLWE_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + in[0];    out[1] = x1 + in[1];    out[2] = x2 + in[2];    out[3] = x3 + in[3];
    out[4] = x4 + in[4];    out[5] = x5 + in[5];    out[6] = x6 + in[6];    out[7] = x7 + in[7];
    out[8] = x8 + in[8];    out[9] = x9 + in[9];    out[10] = x10 + in[10]; out[11] = x11 + in[11];
    out[12] = x12 + in[12]; out[13] = x13 + in[13]; out[14] = x14 + in[14]; out[15] = x15 + in[15];
}
#undef MFHE_RLWE_QR

// the nonce of (stream, limb, polynomial id)
MFHE_RLWE_HD inline void rlwe_nonce(int stream, int limb, uint64_t id, uint32_t (&nonce)[3]) {
    nonce[0] = (uint32_t)stream | ((uint32_t)limb << 8);
    nonce[1] = (uint32_t)id;
    nonce[2] = (uint32_t)(id >> 32);
}

// the 128-bit integer of mask coefficient k (0..3) of a block, as (lo, hi)
MFHE_RLWE_HD inline void rlwe_mask_word(const uint32_t (&out)[16], int k, uint64_t& lo, uint64_t& hi) {
    lo = (uint64_t)out[4 * k] | ((uint64_t)out[4 * k + 1] << 32);
    hi = (uint64_t)out[4 * k + 2] | ((uint64_t)out[4 * k + 3] << 32);
}
// the 64-bit word of small coefficient k (0..7) of a block
MFHE_RLWE_HD inline uint64_t rlwe_small_word(const uint32_t (&out)[16], int k) {
    return (uint64_t)out[2 * k] | ((uint64_t)out[2 * k + 1] << 32);
}

// floor(3 w / 2^64) - 1: -1, 0, 1, each with probability 1/3 up to 2^-64
MFHE_RLWE_HD inline int rlwe_ternary(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__umul64hi(w, 3ull) - 1;
#else
    return (int)(uint64_t)(((unsigned __int128)w * 3u) >> 64) - 1;
#endif
}
// the centred binomial of 2 x 21 bits
MFHE_RLWE_HD inline int rlwe_noise(uint64_t w) {
    const uint64_t m = (1ull << kRlweNoiseBits) - 1;
    return __builtin_popcountll(w & m) - __builtin_popcountll((w >> kRlweNoiseBits) & m);
}
// the small integer of `stream` from its word
MFHE_RLWE_HD inline int rlwe_small_value(int stream, uint64_t w) {
    return rlwe_stream_is_ternary(stream) ? rlwe_ternary(w) : rlwe_noise(w);
}
// v (|v| < q) on a row of modulus q: v or q + v, without a branch
MFHE_RLWE_HD inline uint64_t rlwe_small_residue(int v, uint64_t q) {
    const int64_t x = v;
    return (uint64_t)x + (q & (uint64_t)(x >> 63));
}

// the draws of one coefficient, for the host (the kernels expand a whole block at a time)
inline void rlwe_mask_draw(const uint32_t (&seed)[8], int limb, uint64_t id, uint64_t i, uint64_t& lo, uint64_t& hi) {
    uint32_t nonce[3], out[16];
    rlwe_nonce(kRlweMask, limb, id, nonce);
    chacha20_block(seed, (uint32_t)(i >> 2), nonce, out);
    rlwe_mask_word(out, (int)(i & 3), lo, hi);
}
inline uint64_t rlwe_small_draw(const uint32_t (&seed)[8], int stream, uint64_t id, uint64_t i) {
    uint32_t nonce[3], out[16];
    rlwe_nonce(stream, 0, id, nonce);
    chacha20_block(seed, (uint32_t)(i >> 3), nonce, out);
    return rlwe_small_word(out, (int)(i & 7));
}

}  // namespace mfhe

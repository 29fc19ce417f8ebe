// Prints the draws of csrc/rlwe_draw.hpp for tests/test_rlwe_cpu.py: built from that header alone with a host
// compiler under the address and undefined-behaviour sanitizers.  The seed is the bytes 00 .. 1f.
//   rfc   w0 .. w15                          the block of RFC 8439 2.3.2 (counter 1, nonce 09000000 4a000000 00000000)
//   block stream limb id counter w0 .. w15   a block under this header's nonce layout
//   mask  limb id i lo hi                    the 128-bit integer of mask coefficient i
//   small stream id i w ternary noise value  the word of small coefficient i, both maps, and the stream's own
//   res   v q r                              a small integer's residue
#include <cinttypes>
#include <cstdio>

#include "rlwe_draw.hpp"

using namespace mfhe;

static void print_block(const uint32_t (&out)[16]) {
    for (int i = 0; i < 16; ++i) std::printf(" %08" PRIx32, out[i]);
    std::printf("\n");
}

int main() {
    uint32_t seed[8];
    for (uint32_t i = 0; i < 8; ++i)
        seed[i] = (4 * i) | ((4 * i + 1) << 8) | ((4 * i + 2) << 16) | ((4 * i + 3) << 24);
    uint32_t out[16];
    {
        const uint32_t nonce[3] = {0x09000000u, 0x4a000000u, 0u};
        chacha20_block(seed, 1u, nonce, out);
        std::printf("rfc");
        print_block(out);
    }
    const uint64_t ids[] = {0ull, 0xffffffffull, 0x100000000ull, 0xffffffffffffffffull, 0x0123456789abcdefull};
    {
        uint32_t nonce[3];
        rlwe_nonce(kRlweMask, 3, ids[1], nonce);
        chacha20_block(seed, 5u, nonce, out);
        std::printf("block %d %d %" PRIu64 " %u", kRlweMask, 3, ids[1], 5u);
        print_block(out);
    }
    // i on both sides of the block edges: 4 mask coefficients and 8 small ones to a block; the last block of N = 2^16
    const uint64_t is[] = {0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 1023, 1024, 65535};
    const int limbs[] = {0, 3, 13, 255};
    for (uint64_t id : ids)
        for (int limb : limbs)
            for (uint64_t i : is) {
                uint64_t lo, hi;
                rlwe_mask_draw(seed, limb, id, i, lo, hi);
                std::printf("mask %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", limb, id, i, lo, hi);
            }
    for (int stream = kRlweNoise; stream <= kRlweNoise1; ++stream)
        for (uint64_t id : ids)
            for (uint64_t i : is) {
                const uint64_t w = rlwe_small_draw(seed, stream, id, i);
                std::printf("small %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %d %d\n", stream, id, i, w, rlwe_ternary(w),
                            rlwe_noise(w), rlwe_small_value(stream, w));
            }
    // the extremes of both maps
    const uint64_t ws[] = {0ull, ~0ull, 0x5555555555555555ull, 0x5555555555555556ull, 0xaaaaaaaaaaaaaaaaull,
                           0xaaaaaaaaaaaaaaabull, (1ull << 21) - 1, ((1ull << 21) - 1) << 21, 1ull << 42};
    for (uint64_t w : ws) std::printf("map %" PRIu64 " %d %d\n", w, rlwe_ternary(w), rlwe_noise(w));
    const uint64_t qs[] = {97ull, (1ull << 61) - 1, 0x3fffffffffffffffull};
    const int vs[] = {-21, -1, 0, 1, 21};
    for (uint64_t q : qs)
        for (int v : vs)
            std::printf("res %d %" PRIu64 " %" PRIu64 "\n", v, q, rlwe_small_residue(v, q));
    return 0;
}

// galois.hpp -- the slot permutation of a Galois automorphism in the evaluation domain, and the launcher of the
// automorphism kernel (galois.hip).  The index function is plain integer code, usable from host code, device code and
// a stand-alone program (tests/cpp/galois_perm_main.cpp includes this file with a host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "mfhe_ctx.hpp"
#define MFHE_GALOIS_HD __host__ __device__
#else
#define MFHE_GALOIS_HD
#endif

namespace mfhe {

// the low `bits` bits of x reversed (bits in [0, 32]; higher bits of x ignored)
MFHE_GALOIS_HD inline uint32_t galois_brev(uint32_t x, int bits) {
    if (bits <= 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x) >> (32 - bits);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return x >> (32 - bits);
#endif
}

// Slot i of a phantom-convention transform of length N = 2^log_n holds a(psi^(2 brev(i) + 1)), so
// sigma_g : X -> X^g (g odd, 1 <= g < 2N) is the gather out[i] = in[pi_g(i)] with
//   pi_g(i) = brev(((2 brev(i) + 1) g mod 2N - 1) / 2).
// The product wraps mod 2^32, a multiple of 2N for log_n <= 30, so 32-bit arithmetic is exact.  An aligned block of
// 2^m consecutive i maps into one aligned block of 2^m sources; for m = 1: pi_g(2c + 1) = pi_g(2c) ^ 1.
MFHE_GALOIS_HD inline uint32_t galois_perm_index(uint32_t i, uint32_t g, int log_n) {
    const uint32_t mask = (2u << log_n) - 1u;
    const uint32_t e = ((2u * galois_brev(i, log_n) + 1u) * g) & mask;
    return galois_brev(e >> 1, log_n);
}

#if defined(__HIPCC__)
// One launch, out of place: out[p][r][i] = in[p][r][pi_g(i)] for npoly polynomials of `rows` rows of N words, poly
// strides in words.  The 16-byte pair form is chosen here when N and both strides are even and both buffers 16-byte
// aligned (an output pair (2c, 2c + 1) is the source pair pi(2c) >> 1, swapped when pi(2c) is odd), else the scalar
// form.  Arguments already checked.
int launch_automorphism(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                        size_t npoly, int rows, uint32_t galois_elt, hipStream_t st);
#endif

}  // namespace mfhe

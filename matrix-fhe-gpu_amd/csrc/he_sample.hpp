// he_sample.hpp -- the encrypt's sampler draws, one definition each: the Gaussian noise (he.hip gaussian_kernel,
// gaussian_compact_kernel, gaussian_i8_kernel) and the uniform a (he.hip uniform_kernel; wcrt_digitize.hpp
// mfma_digitize_fold_kernel<D, 2> evaluates the same words inside the W-CRT's digitize).  The encrypt is bit-exact
// across MFHE_OPT_WCRT_MFMA / MFHE_OPT_ENC_E_SMALL because every path draws through these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhe {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// gaussian_noise_kernel HE.cu:581-627: the centred noise integer of coefficient `pos` (< n^2) of polynomial w,
// sigma = 3.2 by Box-Muller on two splitmix64 words.  |result| <= 27 (u1 >= 2^-53).  The expression order is part of
// the result: the build keeps -ffp-contract=off.
__device__ __forceinline__ long long gauss_draw(uint64_t w, uint64_t pos, int log_n) {
    const uint64_t n2 = 1ull << (2 * log_n);
    const uint64_t r1 = splitmix64(0xD6E8FEB86659FD93ULL ^ (w * n2 + pos));
    const uint64_t r2 = splitmix64(r1);
    const double inv53 = 1.0 / 9007199254740992.0;
    const double u1 = ((double)(r1 >> 11) + 1.0) * inv53;
    const double u2 = ((double)(r2 >> 11) + 1.0) * inv53;
    const double mag = 3.2 * sqrt(-2.0 * log(u1));
    const double z = mag * cos(6.283185307179586 * u2);
    return llround(z);
}

// uniform_random_kernel HE.cu:564-578: one LCG step on the element's index in the WHOLE parameter set
// ([phi][Ltot][n^2]; global_limb = the shard's limb_base + its limb), so a residue shard draws its limbs of the
// unsharded a.  The word is affine in w: row w + 1's is row w's + (Ltot << 2 log_n) * kUniformLcgA (the digitize
// steps rows that way).
constexpr uint64_t kUniformSeed0 = 123456789ULL;
constexpr uint64_t kUniformLcgA = 6364136223846793005ULL;
constexpr uint64_t kUniformLcgC = 1442695040888963407ULL;
__device__ __forceinline__ uint64_t uniform_seed(uint64_t w, uint64_t global_limb, uint64_t Ltot, int log_n,
                                                 uint64_t pos) {
    return (kUniformSeed0 + ((w * Ltot + global_limb) << (2 * log_n)) + pos) * kUniformLcgA + kUniformLcgC;
}
// seed mod q by Barrett (mu = floor(2^64 / q)).  Two selects where one suffices (mod128.hpp mod_u128_fold has the
// bound): kept as the sampler was written, the result is the same.
__device__ __forceinline__ uint64_t uniform_reduce(uint64_t seed, uint64_t q, uint64_t mu) {
    uint64_t r = seed - __umul64hi(seed, mu) * q;
    r = r >= q ? r - q : r;
    return r >= q ? r - q : r;
}

}  // namespace mfhe

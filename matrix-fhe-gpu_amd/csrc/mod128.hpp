// mod128.hpp -- device modular reductions, one definition each:
//   shoup_mul, barrett128 (against the DModulus constants of d_dmod) and Lane: the RNS kernels (bconv.hip,
//     keyswitch.hip, galois.hip, lintrans.hip, ctmul.hip, ctmat.hip, slot.hip)
//   mod_u128_fold (against d_rns_mu and d_r64): he.hip mul_s_kernel and ct_mul_kernel, wcrt_gemm.hip mod_gemm_kernel,
//     trace.hip's u128 kernel
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhe {

using u128 = unsigned __int128;

__device__ __forceinline__ uint64_t shoup_mul(uint64_t x, uint64_t w, uint64_t ws, uint64_t q) {
    const uint64_t r = x * w - __umul64hi(x, ws) * q;   // [0, 2q)
    return r >= q ? r - q : r;
}

// x mod q for any 128-bit x, (r0, r1) = floor(2^128 / q): the quotient estimate floor(x (r0, r1) / 2^128) is exact or
// one low, so one conditional subtraction canonicalises
__device__ __forceinline__ uint64_t barrett128(u128 x, uint64_t q, uint64_t r0, uint64_t r1) {
    const uint64_t x0 = (uint64_t)x, x1 = (uint64_t)(x >> 64);
    const u128 a = (u128)x0 * r1 + __umul64hi(x0, r0);
    const u128 b = (u128)x1 * r0 + (uint64_t)a;
    const uint64_t qhat = x1 * r1 + (uint64_t)(a >> 64) + (uint64_t)(b >> 64);
    const uint64_t r = x0 - qhat * q;
    return r >= q ? r - q : r;
}

// (hi:lo) mod q for q < 2^63: fold hi down with r64 = 2^64 mod q until it is zero (each round's value is congruent and
// smaller), then one Barrett step with mu = floor(2^64 / q).  For lo < 2^64, lo / q - lo mu / 2^64 < lo / 2^64 < 1,
// so the quotient estimate floor(lo mu / 2^64) is at most one low and r < 2q: one select canonicalises.
__device__ __forceinline__ uint64_t mod_u128_fold(uint64_t hi, uint64_t lo, uint64_t q, uint64_t mu, uint64_t r64) {
    while (hi) {
        const u128 t = (u128)hi * r64 + lo;
        hi = (uint64_t)(t >> 64);
        lo = (uint64_t)t;
    }
    const uint64_t r = lo - __umul64hi(lo, mu) * q;
    return r >= q ? r - q : r;
}
// a b mod q for any 64-bit a, b
__device__ __forceinline__ uint64_t mulmod_fold(uint64_t a, uint64_t b, uint64_t q, uint64_t mu, uint64_t r64) {
    const u128 v = (u128)a * b;
    return mod_u128_fold((uint64_t)(v >> 64), (uint64_t)v, q, mu, r64);
}

// V coefficients per thread: one u64, or two with a 16-byte load / store
template <int V>
struct Lane;
template <>
struct Lane<1> {
    using T = uint64_t;
    static __device__ __forceinline__ void load(const T* p, uint64_t (&x)[1]) { x[0] = *p; }
    static __device__ __forceinline__ void store(T* p, const uint64_t (&x)[1]) { *p = x[0]; }
};
template <>
struct Lane<2> {
    using T = ulonglong2;
    static __device__ __forceinline__ void load(const T* p, uint64_t (&x)[2]) {
        const T v = *p;
        x[0] = v.x;
        x[1] = v.y;
    }
    static __device__ __forceinline__ void store(T* p, const uint64_t (&x)[2]) { *p = make_ulonglong2(x[0], x[1]); }
};

}  // namespace mfhe

// mod128.hpp -- device modular reductions shared by the RNS kernels (bconv.hip, keyswitch.hip): a Shoup multiply
// and the 128-bit Barrett reduction against the DModulus constants of d_dmod.
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

// ctmul.hpp -- ciphertext products on the key switch's layout (ctmul.hip): the kernel arguments and the launcher of
// the summed tensor product.
#pragma once
#include "keyswitch.hpp"

namespace mfhe {

// most terms of one tensor sum
constexpr int kCtmulMaxTerms = 64;

// Kernel arguments of the summed tensor product.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2 the
// 16-byte form).  a0, a1 [nterms][npoly][level][ncoeff] with a term stride and a poly stride, b0, b1 the same with
// their own strides (both null: the square form, the b strides unread); d0, d1 [npoly][level][ncoeff] with one poly
// stride, d2 with its own.
struct CtmulArgs {
    const void *a0, *a1, *b0, *b1;
    void *d0, *d1, *d2;
    uint64_t a_term, a_poly, b_term, b_poly, d01_poly, d2_poly;
    uint64_t ncoeff;   // elements per row
    uint64_t npoly;
    int nterms, level;
};

// One launch: d0 = sum_t a0[t] b0[t], d1 = sum_t (a0[t] b1[t] + a1[t] b0[t]), d2 = sum_t a1[t] b1[t] mod q_r on rows
// r < level (limb r is row r); with b0 = b1 = null, d0 = sum a0^2, d1 = 2 sum a0 a1, d2 = sum a1^2.  Strides and
// ncoeff given in words; the 16-byte form is chosen here when ncoeff and every stride are even and every buffer
// 16-byte aligned.  Arguments already checked.
int launch_ctmul_tensor(mfhe_ctx* c, CtmulArgs a, hipStream_t st);

}  // namespace mfhe

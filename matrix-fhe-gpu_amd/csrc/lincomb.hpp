// lincomb.hpp -- scalar linear combinations of ciphertexts on the key switch's layout (lincomb.hip): the kernel
// arguments and the launcher, shared with the polynomial driver (poly.hip).
#pragma once
#include "keyswitch.hpp"

namespace mfhe {

// most terms of one sum: the index arrays travel in the kernel arguments
constexpr int kLincombMaxTerms = 64;

// Kernel arguments of the linear combination.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2 the 16-byte
// form), k_stride always in words.  x0, x1 [nsrc][npoly][>= level rows][ncoeff] with a source stride and a poly stride,
// k [nk][>= level] canonical residues, o0, o1 [npoly][level][ncoeff] with one poly stride.
struct LincombArgs {
    const void *x0, *x1;
    const uint64_t* k;
    void *o0, *o1;
    uint64_t src_stride, x_poly, o_poly, k_stride;
    uint64_t ncoeff;        // elements per row
    uint64_t npairs, prun;  // (polynomial, component) pairs = 2 npoly; pairs one thread walks (grid z = ceil(npairs / prun))
    int nterms, level, addend_k;   // addend_k < 0: no addend
    int term_x[kLincombMaxTerms], term_k[kLincombMaxTerms];   // source and constant of term t, by value: nothing is copied
};

// One launch: o_c[p][r] = sum_t k[term_k[t]][r] x_c[term_x[t]][p][r] + [c == 0, addend_k >= 0] k[addend_k][r] mod q_r on
// rows r < level (limb r is row r).  Strides and ncoeff given in words; the 16-byte form is chosen here when ncoeff and
// every stride are even and the four buffers 16-byte aligned.  Arguments already checked.
int launch_ct_lincomb(mfhe_ctx* c, LincombArgs a, size_t npoly, hipStream_t st);

}  // namespace mfhe

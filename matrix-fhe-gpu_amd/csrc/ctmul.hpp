// ctmul.hpp -- ciphertext products on the key switch's layout (ctmul.hip): the kernel arguments and the launcher of
// the summed tensor product, and what the matrix product (ctmat.hip) shares with it: the term of the three sums, the
// argument checks and the relinearise and rescale tail of the driver.
#pragma once
#include <string>

#include "keyswitch.hpp"
#include "mod128.hpp"

namespace mfhe {

// most terms of one tensor sum
constexpr int kCtmulMaxTerms = 64;
// terms between two reductions of the running sums
constexpr int kCtmulFold = 8;

// one term into the three sums: four products, or three in the square form (s1 then holds sum a0 a1, doubled at the
// reduction)
template <int V, bool SQ>
static __device__ __forceinline__ void ct_term(const uint64_t (&x0)[V], const uint64_t (&x1)[V],
                                               const uint64_t (&y0)[V], const uint64_t (&y1)[V], u128 (&s0)[V],
                                               u128 (&s1)[V], u128 (&s2)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (SQ) {
            s0[k] += (u128)x0[k] * x0[k];
            s1[k] += (u128)x0[k] * x1[k];
            s2[k] += (u128)x1[k] * x1[k];
        } else {
            s0[k] += (u128)x0[k] * y0[k];
            s1[k] += (u128)x0[k] * y1[k];
            s1[k] += (u128)x1[k] * y0[k];
            s2[k] += (u128)x1[k] * y1[k];
        }
    }
}

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

// ---- shared with ctmat.hip ----
// the flags of a driver: unknown ones, and MFHE_CTMUL_RESCALE at level 1
int ctmul_check_flags(const char* what, int flags, int level);
// ks_prepare for a driver's block of the workspace: the key switch's block (the rescale's scratch, 2 npoly level N
// words, reuses it), then d2 [npoly][level][N]; with MFHE_CTMUL_RESCALE the rescale's table as well
int ctmul_prepare(mfhe_ctx* c, size_t npoly, const KsGeom& g, int alpha, int flags, KsTables& t);
// d2 of a driver, dense behind the key switch's block
inline uint64_t* ctmul_d2(const mfhe_ctx* c, size_t npoly, int beta, const KsGeom& g) {
    return (uint64_t*)c->ws + ks_ws(npoly, beta, (size_t)g.rows(), c->N).end;
}
// The tail of a driver once the tensor sum has left d0, d1 in the outputs ([npoly][level][N] at out_poly_stride) and
// d2 dense at ctmul_d2: the body of mfhe_keyswitch with MFHE_KS_ADD on d2, then with MFHE_CTMUL_RESCALE the ModDown of
// both outputs by limb level - 1 in place.  ctmul_prepare done by the caller.
int ctmul_relin_rescale(mfhe_ctx* c, const uint64_t* d_rlk, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride,
                        size_t npoly, const KsGeom& g, int alpha, const KsTables& t, int flags, hipStream_t st);
// ---- shared with poly.hip ----
// The rescale half of that tail alone: the ModDown of both outputs ([npoly][level][N] at out_poly_stride) by limb
// level - 1 in place, scratch the key switch's block (2 npoly level N words), t.rescale built (kKsRescale).
int ctmul_rescale(mfhe_ctx* c, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride, size_t npoly,
                  const KsGeom& g, const KsTables& t, hipStream_t st);

}  // namespace mfhe

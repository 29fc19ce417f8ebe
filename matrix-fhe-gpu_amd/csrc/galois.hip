// galois.hip -- Galois automorphisms and hoisted rotations for gfx950 (include/mfhe.h mfhe_ntt_automorphism,
// mfhe_keyswitch_raise, mfhe_galois_apply_raised, mfhe_galois_apply, mfhe_galois_reserve; mfhe_ksk_inner_product_galois
// is in keyswitch.hip, beside the kernel it shares).
//
// Everything is in the evaluation domain (phantom NTT) and canonical, on the geometry of keyswitch.hip.  Slot i of a
// transformed row holds a(psi^(2 brev(i) + 1)), so sigma_g : X -> X^g is the gather out[i] = in[pi_g(i)] of
// galois.hpp: the same for every limb, no modular arithmetic, no table.  An aligned block of 2^m outputs reads one
// aligned block of 2^m sources, so a thread moves a 16-byte pair (swapped when pi(2c) is odd) and a wave that writes
// 1 KiB reads exactly one aligned 1 KiB.
//
//   automorphism : out[p][r][i] = in[p][r][pi_g(i)], one launch
//   raise        : the ModUp of every digit (the hoisted part: no key, no g)
//   apply_raised : out0 = sigma_g(c0) + k0, out1 = k1, (k0, k1) = ModDown_P(sum_j sigma_g(raised_j) gk_j); the gather is
//                  fused into the inner product (keyswitch.hip, the PERM instantiations of its kernel)
//   apply        : raise c1 into the workspace, then the body of apply_raised
#include "galois.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "keyswitch.hpp"
#include "mod128.hpp"

namespace mfhe {

// One thread per output element (V words) of one row; the row (polynomial p, row r) is the folded y/z index.
template <int V>
__global__ __launch_bounds__(256) void automorphism_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                           uint64_t in_stride, uint64_t out_stride, uint64_t ncoeff,
                                                           uint32_t rows, uint64_t total_rows, uint32_t galois_elt,
                                                           int log_n) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t pr = blockIdx.z * (uint64_t)gridDim.y + blockIdx.y;
    if (c >= ncoeff || pr >= total_rows) return;
    const uint64_t p = pr / rows, r = pr - p * rows;
    const uint32_t src = galois_perm_index((uint32_t)c * V, galois_elt, log_n);
    uint64_t x[V];
    Lane<V>::load((const T*)in + p * in_stride + r * ncoeff + (V == 2 ? src >> 1 : src), x);
    if (V == 2 && (src & 1u)) {
        const uint64_t t = x[0];
        x[0] = x[V - 1];
        x[V - 1] = t;
    }
    Lane<V>::store((T*)out + p * out_stride + r * ncoeff + c, x);
}

int launch_automorphism(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                        size_t npoly, int rows, uint32_t galois_elt, hipStream_t st) {
    uint64_t ncoeff = c->N;
    if (npoly == 0 || rows == 0) return MFHE_OK;
    const bool wide = ks_wide({&ncoeff, &in_stride, &out_stride}, {d_in, d_out});
    const KsRowGrid rg = ks_row_grid(ncoeff);
    // (polynomial, row) folded over y and z so that neither exceeds 65535
    const uint64_t total = (uint64_t)npoly * (uint64_t)rows;
    const KsFold f = ks_fold(total);
    if (rg.bx > 0x7fffffffull || f.gz > 65535) return set_error(MFHE_EINVAL, "ntt_automorphism: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)f.gy, (uint32_t)f.gz);
    if (wide)
        hipLaunchKernelGGL(automorphism_kernel<2>, grid, dim3(rg.block), 0, st, (const void*)d_in, (void*)d_out,
                           (uint64_t)in_stride, (uint64_t)out_stride, ncoeff, (uint32_t)rows, total, galois_elt,
                           c->logN);
    else
        hipLaunchKernelGGL(automorphism_kernel<1>, grid, dim3(rg.block), 0, st, (const void*)d_in, (void*)d_out,
                           (uint64_t)in_stride, (uint64_t)out_stride, ncoeff, (uint32_t)rows, total, galois_elt,
                           c->logN);
    MFHE_CHECK_LAUNCH("automorphism_kernel");
    return MFHE_OK;
}

// automorphism of c0 into out0, then the gathered inner product of x and the ModDown of the pair, with out0 as the
// addend of component 0
static int apply_body(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const KsRaised& x, const uint64_t* d_gk,
                      uint64_t* d_out0, uint64_t* d_out1, size_t out_stride, size_t npoly, const KsGeom& g,
                      const KsTables& t, uint32_t galois_elt, hipStream_t st) {
    RC(launch_automorphism(c, d_c0, in_stride, d_out0, out_stride, npoly, g.level, galois_elt, st));
    return ks_apply_raised(c, x, d_gk, {d_out0, d_out1, out_stride, 1}, npoly, g, t, galois_elt, st);
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ntt_automorphism(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out,
                                     size_t out_stride, size_t npoly, int rows, int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_in || !d_out) return set_error(MFHE_EINVAL, "ntt_automorphism: null pointer");
    if (rows < 0) return set_error(MFHE_EINVAL, "ntt_automorphism: rows < 0");
    RC(ks_check_galois(c, galois_elt, "ntt_automorphism"));
    const size_t words = (size_t)rows * c->N;
    if (in_stride < words || out_stride < words)
        return set_error(MFHE_EINVAL, "ntt_automorphism: poly stride smaller than rows * N");
    RC(ks_check_overlap("ntt_automorphism", {{d_in, ks_span(npoly, in_stride, words)}},
                        {{d_out, ks_span(npoly, out_stride, words)}}));   // out of place only
    return launch_automorphism(c, d_in, in_stride, d_out, out_stride, npoly, rows, (uint32_t)galois_elt,
                               (hipStream_t)s);
}

extern "C" int mfhe_galois_reserve(mfhe_ctx* c, size_t npoly, int level, int key_level, int alpha, int special_start,
                                   int nspecial) {
    return ks_reserve(c, npoly, {level, key_level, special_start, nspecial}, alpha, "galois_reserve");
}

extern "C" int mfhe_keyswitch_raise(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_raised,
                                    size_t digit_stride, size_t poly_stride, size_t npoly, int level, int alpha,
                                    int special_start, int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_in || !d_raised) return set_error(MFHE_EINVAL, "keyswitch_raise: null pointer");
    const KsGeom g{level, level, special_start, nspecial};   // no key enters: any key_level >= level gives the same digits
    RC(ks_check_digits(c, alpha, g, "keyswitch_raise"));
    const size_t N = c->N, rows = (size_t)g.rows(), pw = rows * N, lw = (size_t)level * N;
    const int beta = ks_beta(level, alpha);
    if (in_stride < lw) return set_error(MFHE_EINVAL, "keyswitch_raise: input poly stride smaller than level * N");
    if (poly_stride < pw) return set_error(MFHE_EINVAL, "keyswitch_raise: poly stride smaller than rows * N");
    const size_t dsp = ks_span(npoly, poly_stride, pw);
    if (npoly && digit_stride < dsp)
        return set_error(MFHE_EINVAL, "keyswitch_raise: digit stride smaller than the polynomials of a digit");
    RC(ks_check_overlap("keyswitch_raise", {{d_in, ks_span(npoly, in_stride, lw)}},
                        {{d_raised, ks_span(beta, digit_stride, dsp)}}));
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_prepare(c, g, alpha, 0, ks_ws_words(npoly, beta, rows, N), t));
    return raise_body(c, d_in, in_stride, d_raised, digit_stride, poly_stride, npoly, g, alpha, t,
                      (uint64_t*)c->ws + ks_ws(npoly, beta, rows, N).scratch, (hipStream_t)s);
}

extern "C" int mfhe_galois_apply_raised(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const uint64_t* d_raised,
                                        size_t digit_stride, size_t poly_stride, const uint64_t* d_gk, uint64_t* d_out0,
                                        uint64_t* d_out1, size_t out_stride, size_t npoly, int level, int key_level,
                                        int alpha, int special_start, int nspecial, int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_raised || !d_gk || !d_out0 || !d_out1)
        return set_error(MFHE_EINVAL, "galois_apply_raised: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "galois_apply_raised"));
    RC(ks_check_galois(c, galois_elt, "galois_apply_raised"));
    const size_t N = c->N, rows = (size_t)g.rows(), pw = rows * N, lw = (size_t)level * N;
    const int beta = ks_beta(level, alpha);
    if (in_stride < lw || out_stride < lw)
        return set_error(MFHE_EINVAL, "galois_apply_raised: poly stride smaller than level * N");
    if (poly_stride < pw) return set_error(MFHE_EINVAL, "galois_apply_raised: raised poly stride smaller than rows * N");
    const size_t dsp = ks_span(npoly, poly_stride, pw);
    if (npoly && digit_stride < dsp)
        return set_error(MFHE_EINVAL, "galois_apply_raised: digit stride smaller than the polynomials of a digit");
    const size_t osp = ks_span(npoly, out_stride, lw);
    RC(ks_check_overlap("galois_apply_raised",
                        {{d_c0, ks_span(npoly, in_stride, lw)}, {d_raised, ks_span(beta, digit_stride, dsp)}},
                        {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_prepare(c, g, alpha, 0, ks_ws_words(npoly, beta, rows, N), t));
    return apply_body(c, d_c0, in_stride, {d_raised, digit_stride, poly_stride}, d_gk, d_out0, d_out1, out_stride,
                      npoly, g, t, (uint32_t)galois_elt, (hipStream_t)s);
}

extern "C" int mfhe_galois_apply(mfhe_ctx* c, const uint64_t* d_c0, const uint64_t* d_c1, size_t in_stride,
                                 const uint64_t* d_gk, uint64_t* d_out0, uint64_t* d_out1, size_t out_stride,
                                 size_t npoly, int level, int key_level, int alpha, int special_start, int nspecial,
                                 int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_c1 || !d_gk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "galois_apply: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "galois_apply"));
    RC(ks_check_galois(c, galois_elt, "galois_apply"));
    const size_t N = c->N, lw = (size_t)level * N;
    if (in_stride < lw || out_stride < lw)
        return set_error(MFHE_EINVAL, "galois_apply: poly stride smaller than level * N");
    const size_t isp = ks_span(npoly, in_stride, lw), osp = ks_span(npoly, out_stride, lw);
    RC(ks_check_overlap("galois_apply", {{d_c0, isp}, {d_c1, isp}}, {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_prepare(c, g, alpha, 0, ks_ws_words(npoly, ks_beta(level, alpha), (size_t)g.rows(), N), t));
    hipStream_t st = (hipStream_t)s;
    RC(ks_raise_ws(c, d_c1, in_stride, npoly, g, alpha, t, st));
    return apply_body(c, d_c0, in_stride, ks_ws_raised(c, npoly, g), d_gk, d_out0, d_out1, out_stride, npoly, g, t,
                      (uint32_t)galois_elt, st);
}


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
    const bool wide = ncoeff % 2 == 0 && in_stride % 2 == 0 && out_stride % 2 == 0 &&
                      (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;
    if (wide) {
        ncoeff /= 2;
        in_stride /= 2;
        out_stride /= 2;
    }
    const uint32_t block = ncoeff >= 256 ? 256 : (uint32_t)((ncoeff + 63) / 64 * 64);
    const uint64_t bx = (ncoeff + block - 1) / block;
    // (polynomial, row) folded over y and z so that neither exceeds 65535
    const uint64_t total = (uint64_t)npoly * (uint64_t)rows;
    const uint64_t gy = total < 65535 ? total : 65535, gz = (total + gy - 1) / gy;
    if (bx > 0x7fffffffull || gz > 65535) return set_error(MFHE_EINVAL, "ntt_automorphism: too large for one launch");
    const dim3 grid((uint32_t)bx, (uint32_t)gy, (uint32_t)gz);
    if (wide)
        hipLaunchKernelGGL(automorphism_kernel<2>, grid, dim3(block), 0, st, (const void*)d_in, (void*)d_out,
                           (uint64_t)in_stride, (uint64_t)out_stride, ncoeff, (uint32_t)rows, total, galois_elt,
                           c->logN);
    else
        hipLaunchKernelGGL(automorphism_kernel<1>, grid, dim3(block), 0, st, (const void*)d_in, (void*)d_out,
                           (uint64_t)in_stride, (uint64_t)out_stride, ncoeff, (uint32_t)rows, total, galois_elt,
                           c->logN);
    MFHE_CHECK_LAUNCH("automorphism_kernel");
    return MFHE_OK;
}

// the workspace of the Galois calls, the key switch's block: [beta][npoly][rows][N] raised digits (mfhe_galois_apply
// alone uses them), [npoly][2][rows][N] accumulators, 2 npoly rows N words of the inner steps' scratch
struct GaloisWs {
    uint64_t *raised, *acc, *scratch;
};
static GaloisWs galois_ws(mfhe_ctx* c, size_t npoly, int beta, size_t pw) {
    GaloisWs w;
    w.raised = (uint64_t*)c->ws;
    w.acc = w.raised + (size_t)beta * npoly * pw;
    w.scratch = w.acc + 2 * npoly * pw;
    return w;
}

}  // namespace mfhe

using namespace mfhe;

#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

extern "C" int mfhe_ntt_automorphism(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out,
                                     size_t out_stride, size_t npoly, int rows, int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_in || !d_out) return set_error(MFHE_EINVAL, "ntt_automorphism: null pointer");
    if (rows < 0) return set_error(MFHE_EINVAL, "ntt_automorphism: rows < 0");
    RC(ks_check_galois(c, galois_elt, "ntt_automorphism"));
    const size_t words = (size_t)rows * c->N;
    if (in_stride < words || out_stride < words)
        return set_error(MFHE_EINVAL, "ntt_automorphism: poly stride smaller than rows * N");
    if (ks_ranges_overlap(d_in, ks_span(npoly, in_stride, words), d_out, ks_span(npoly, out_stride, words)))
        return set_error(MFHE_EINVAL, "ntt_automorphism: the input overlaps the output (out of place only)");
    return launch_automorphism(c, d_in, in_stride, d_out, out_stride, npoly, rows, (uint32_t)galois_elt,
                               (hipStream_t)s);
}

extern "C" int mfhe_galois_reserve(mfhe_ctx* c, size_t npoly, int level, int key_level, int alpha, int special_start,
                                   int nspecial) {
    RC(ks_check_ctx(c));
    if (alpha < 1) return set_error(MFHE_EINVAL, "galois_reserve: alpha < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_geom(c, g, "galois_reserve"));
    KsTables t;
    RC(ks_tables(c, g, alpha, t));
    return grow_ws(c, ks_ws_words(npoly, t.beta, (size_t)g.rows(), c->N) * 8);
}

// ModUp of every digit of d_in into raised [beta][npoly][rows][N] (strides in words); scratch: npoly rows N words
int mfhe::raise_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* raised, size_t digit_stride,
                     size_t poly_stride, size_t npoly, const KsGeom& g, int alpha, const KsTables& t,
                     uint64_t* scratch, hipStream_t st) {
    for (int j = 0; j < t.beta; ++j) {
        const int ds = j * alpha, dc = g.level - ds < alpha ? g.level - ds : alpha;
        RC(ntt_modup_body(c, d_in, in_stride, raised + (size_t)j * digit_stride, poly_stride, npoly, ds, dc, t.plan[j],
                          &t.tab[(size_t)3 * j], scratch, st));
    }
    return MFHE_OK;
}

// automorphism of c0 into out0, the gathered inner product, ModDown of both components as one batch, one tail per
// component with out0 as the addend of component 0
static int apply_body(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const uint64_t* raised, size_t digit_stride,
                      size_t poly_stride, const uint64_t* d_gk, uint64_t* d_out0, uint64_t* d_out1, size_t out_stride,
                      size_t npoly, const KsGeom& g, const KsTables& t, uint32_t galois_elt, const GaloisWs& w,
                      hipStream_t st) {
    const size_t N = c->N, pw = (size_t)g.rows() * N, lw = (size_t)g.level * N;
    RC(launch_automorphism(c, d_c0, in_stride, d_out0, out_stride, npoly, g.level, galois_elt, st));
    KsipArgs a{};
    a.raised = raised; a.ksk = d_gk; a.acc = w.acc;
    a.digit_stride = digit_stride; a.poly_stride = poly_stride; a.acc_stride = 2 * pw;
    a.ncoeff = N; a.npoly = npoly; a.ndigits = t.beta; a.g = g; a.galois_elt = galois_elt;
    RC(launch_ksk_inner_product(c, a, st));
    const uint64_t* cen = nullptr;
    RC(ntt_moddown_center(c, w.acc, pw, 2 * npoly, g.level, g.special_start, g.nspecial, t.down, w.scratch, &cen, st));
    uint64_t* outs[2] = {d_out0, d_out1};
    for (int k = 0; k < 2; ++k)
        RC(launch_sub_scale(c, w.acc + (size_t)k * pw, 2 * pw, cen + (size_t)k * lw, 2 * lw, outs[k], out_stride,
                            k == 0 ? d_out0 : nullptr, npoly, g.level, g.nspecial, t.down, st));
    return MFHE_OK;
}

extern "C" int mfhe_keyswitch_raise(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_raised,
                                    size_t digit_stride, size_t poly_stride, size_t npoly, int level, int alpha,
                                    int special_start, int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_in || !d_raised) return set_error(MFHE_EINVAL, "keyswitch_raise: null pointer");
    if (alpha < 1) return set_error(MFHE_EINVAL, "keyswitch_raise: alpha < 1");
    const KsGeom g{level, level, special_start, nspecial};   // no key enters: any key_level >= level gives the same digits
    RC(ks_check_geom(c, g, "keyswitch_raise"));
    const size_t N = c->N, pw = (size_t)g.rows() * N, lw = (size_t)level * N;
    const int beta = (level + alpha - 1) / alpha;
    if (in_stride < lw) return set_error(MFHE_EINVAL, "keyswitch_raise: input poly stride smaller than level * N");
    if (poly_stride < pw) return set_error(MFHE_EINVAL, "keyswitch_raise: poly stride smaller than rows * N");
    const size_t dsp = ks_span(npoly, poly_stride, pw);
    if (npoly && digit_stride < dsp)
        return set_error(MFHE_EINVAL, "keyswitch_raise: digit stride smaller than the polynomials of a digit");
    if (ks_ranges_overlap(d_in, ks_span(npoly, in_stride, lw), d_raised, ks_span(beta, digit_stride, dsp)))
        return set_error(MFHE_EINVAL, "keyswitch_raise: the input overlaps the raised digits");
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_tables(c, g, alpha, t));
    RC(grow_ws(c, ks_ws_words(npoly, t.beta, (size_t)g.rows(), N) * 8));
    const GaloisWs w = galois_ws(c, npoly, t.beta, pw);
    return raise_body(c, d_in, in_stride, d_raised, digit_stride, poly_stride, npoly, g, alpha, t, w.scratch,
                      (hipStream_t)s);
}

extern "C" int mfhe_galois_apply_raised(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const uint64_t* d_raised,
                                        size_t digit_stride, size_t poly_stride, const uint64_t* d_gk, uint64_t* d_out0,
                                        uint64_t* d_out1, size_t out_stride, size_t npoly, int level, int key_level,
                                        int alpha, int special_start, int nspecial, int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_raised || !d_gk || !d_out0 || !d_out1)
        return set_error(MFHE_EINVAL, "galois_apply_raised: null pointer");
    if (alpha < 1) return set_error(MFHE_EINVAL, "galois_apply_raised: alpha < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_geom(c, g, "galois_apply_raised"));
    RC(ks_check_galois(c, galois_elt, "galois_apply_raised"));
    const size_t N = c->N, pw = (size_t)g.rows() * N, lw = (size_t)level * N;
    const int beta = (level + alpha - 1) / alpha;
    if (in_stride < lw || out_stride < lw)
        return set_error(MFHE_EINVAL, "galois_apply_raised: poly stride smaller than level * N");
    if (poly_stride < pw) return set_error(MFHE_EINVAL, "galois_apply_raised: raised poly stride smaller than rows * N");
    const size_t dsp = ks_span(npoly, poly_stride, pw);
    if (npoly && digit_stride < dsp)
        return set_error(MFHE_EINVAL, "galois_apply_raised: digit stride smaller than the polynomials of a digit");
    const size_t isp = ks_span(npoly, in_stride, lw), osp = ks_span(npoly, out_stride, lw);
    const size_t rsp = ks_span(beta, digit_stride, dsp);
    uint64_t* outs[2] = {d_out0, d_out1};
    for (uint64_t* o : outs)
        if (ks_ranges_overlap(d_c0, isp, o, osp) || ks_ranges_overlap(d_raised, rsp, o, osp))
            return set_error(MFHE_EINVAL, "galois_apply_raised: an input overlaps an output");
    if (ks_ranges_overlap(d_out0, osp, d_out1, osp))
        return set_error(MFHE_EINVAL, "galois_apply_raised: the outputs overlap");
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_tables(c, g, alpha, t));
    RC(grow_ws(c, ks_ws_words(npoly, t.beta, (size_t)g.rows(), N) * 8));
    const GaloisWs w = galois_ws(c, npoly, t.beta, pw);
    return apply_body(c, d_c0, in_stride, d_raised, digit_stride, poly_stride, d_gk, d_out0, d_out1, out_stride, npoly,
                      g, t, (uint32_t)galois_elt, w, (hipStream_t)s);
}

extern "C" int mfhe_galois_apply(mfhe_ctx* c, const uint64_t* d_c0, const uint64_t* d_c1, size_t in_stride,
                                 const uint64_t* d_gk, uint64_t* d_out0, uint64_t* d_out1, size_t out_stride,
                                 size_t npoly, int level, int key_level, int alpha, int special_start, int nspecial,
                                 int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_c1 || !d_gk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "galois_apply: null pointer");
    if (alpha < 1) return set_error(MFHE_EINVAL, "galois_apply: alpha < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_geom(c, g, "galois_apply"));
    RC(ks_check_galois(c, galois_elt, "galois_apply"));
    const size_t N = c->N, pw = (size_t)g.rows() * N, lw = (size_t)level * N;
    if (in_stride < lw || out_stride < lw)
        return set_error(MFHE_EINVAL, "galois_apply: poly stride smaller than level * N");
    const size_t isp = ks_span(npoly, in_stride, lw), osp = ks_span(npoly, out_stride, lw);
    uint64_t* outs[2] = {d_out0, d_out1};
    for (uint64_t* o : outs)
        if (ks_ranges_overlap(d_c0, isp, o, osp) || ks_ranges_overlap(d_c1, isp, o, osp))
            return set_error(MFHE_EINVAL, "galois_apply: an input overlaps an output");
    if (ks_ranges_overlap(d_out0, osp, d_out1, osp)) return set_error(MFHE_EINVAL, "galois_apply: the outputs overlap");
    if (npoly == 0) return MFHE_OK;
    KsTables t;
    RC(ks_tables(c, g, alpha, t));
    RC(grow_ws(c, ks_ws_words(npoly, t.beta, (size_t)g.rows(), N) * 8));
    const GaloisWs w = galois_ws(c, npoly, t.beta, pw);
    hipStream_t st = (hipStream_t)s;
    RC(raise_body(c, d_c1, in_stride, w.raised, npoly * pw, pw, npoly, g, alpha, t, w.scratch, st));
    return apply_body(c, d_c0, in_stride, w.raised, npoly * pw, pw, d_gk, d_out0, d_out1, out_stride, npoly, g, t,
                      (uint32_t)galois_elt, w, st);
}

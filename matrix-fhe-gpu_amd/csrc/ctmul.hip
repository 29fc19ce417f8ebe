// ctmul.hip -- ciphertext products for gfx950 on the layout of the key switch: the summed tensor product and the
// driver that chains it with relinearisation and rescale (include/mfhe.h mfhe_ctmul_tensor, mfhe_ctmul_apply,
// mfhe_ctmul_reserve).
//
// Everything is in the evaluation domain (phantom NTT) and canonical, on the geometry of keyswitch.hip; a ciphertext
// is a pair of [level][N] polynomials and limb r is row r.
//
//   tensor : d0 = sum_t a0[t] b0[t], d1 = sum_t (a0[t] b1[t] + a1[t] b0[t]), d2 = sum_t a1[t] b1[t] mod q_r, one launch;
//            the square form (no B) is d0 = sum a0^2, d1 = 2 sum a0 a1, d2 = sum a1^2
//   apply  : tensor with d0, d1 in the outputs and d2 in the workspace, the body of mfhe_keyswitch on d2 with the
//            outputs as the addends of ModDown's tails (lazy relinearisation: one key switch per sum, not per term),
//            then with MFHE_CTMUL_RESCALE the ModDown of both outputs by limb level - 1, in place
//
// Tensor design, as the multiply-accumulate of lintrans.hip: one thread owns one (row, coefficient) -- two adjacent
// coefficients with 16-byte accesses when the layout allows -- and walks the polynomials blockIdx.z, blockIdx.z +
// gridDim.z, ...  The three sums are unreduced u128 and each ends in one 128-bit Barrett reduction.  d1 takes two
// products per term and 16 products of canonical residues below 2^62 plus one residue fit a u128, so sums fold every
// kCtmulFold = 8 terms (the reduced residues are carried in); the square form keeps the chunk, its 2 sum over 8 terms
// is below 2^128 as well.  Term counts up to kCtmulUnroll are template-unrolled with every load issued before the
// first product; longer sums run the chunked loop.  The row is the grid's y index, so the modulus constants are
// scalar loads.
#include "ctmul.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "mod128.hpp"

namespace mfhe {

// largest term count whose operands stay in registers (DESIGN.md §3.12 has the resource table behind it)
constexpr int kCtmulUnroll = 6;

// NT: terms (template-unrolled, every operand in registers) or 0 (chunked loop over a.nterms); V: coefficients per
// thread; SQ: the square form, b0 and b1 unread.  dmod is indexed by the block's row: scalar loads.
template <int NT, int V, bool SQ>
__global__ __launch_bounds__(256) void ctmul_tensor_kernel(CtmulArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t q = dmod[3 * r], r0 = dmod[3 * r + 1], r1 = dmod[3 * r + 2];
    const uint64_t ro = (uint64_t)r * a.ncoeff + c;
    const T* a0 = (const T*)a.a0 + ro;
    const T* a1 = (const T*)a.a1 + ro;
    const T* b0 = SQ ? a0 : (const T*)a.b0 + ro;
    const T* b1 = SQ ? a1 : (const T*)a.b1 + ro;
    T* d0 = (T*)a.d0 + ro;
    T* d1 = (T*)a.d1 + ro;
    T* d2 = (T*)a.d2 + ro;

    for (uint64_t p = blockIdx.z; p < a.npoly; p += gridDim.z) {
        const uint64_t ao = p * a.a_poly, bo = SQ ? 0 : p * a.b_poly;
        uint64_t o0[V], o1[V], o2[V];
        if (NT) {
            constexpr int NK = NT ? NT : 1, NB = SQ ? 1 : NK;
            uint64_t x0[NK][V], x1[NK][V], y0[NB][V], y1[NB][V];
#pragma unroll
            for (int t = 0; t < NK; ++t) {
                Lane<V>::load(a0 + (uint64_t)t * a.a_term + ao, x0[t]);
                Lane<V>::load(a1 + (uint64_t)t * a.a_term + ao, x1[t]);
                if (!SQ) {
                    Lane<V>::load(b0 + (uint64_t)t * a.b_term + bo, y0[t % NB]);
                    Lane<V>::load(b1 + (uint64_t)t * a.b_term + bo, y1[t % NB]);
                }
            }
            u128 s0[V], s1[V], s2[V];
#pragma unroll
            for (int k = 0; k < V; ++k) s0[k] = s1[k] = s2[k] = 0;
#pragma unroll
            for (int t = 0; t < NK; ++t)
                ct_term<V, SQ>(x0[t], x1[t], SQ ? x0[t] : y0[t % NB], SQ ? x1[t] : y1[t % NB], s0, s1, s2);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                o0[k] = barrett128(s0[k], q, r0, r1);
                o1[k] = barrett128(SQ ? s1[k] << 1 : s1[k], q, r0, r1);
                o2[k] = barrett128(s2[k], q, r0, r1);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) o0[k] = o1[k] = o2[k] = 0;
            // general form: 16 products < 2^124 and a residue < 2^62 fit a u128; square form: 2 (8 products) and a
            // residue do
            for (int t0 = 0; t0 < a.nterms; t0 += kCtmulFold) {
                u128 s0[V], s1[V], s2[V];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    s0[k] = o0[k];
                    s1[k] = SQ ? 0 : o1[k];
                    s2[k] = o2[k];
                }
                const int t1 = t0 + kCtmulFold < a.nterms ? t0 + kCtmulFold : a.nterms;
                for (int t = t0; t < t1; ++t) {
                    uint64_t x0[V], x1[V], y0[V], y1[V];
                    Lane<V>::load(a0 + (uint64_t)t * a.a_term + ao, x0);
                    Lane<V>::load(a1 + (uint64_t)t * a.a_term + ao, x1);
                    if (!SQ) {
                        Lane<V>::load(b0 + (uint64_t)t * a.b_term + bo, y0);
                        Lane<V>::load(b1 + (uint64_t)t * a.b_term + bo, y1);
                    }
                    ct_term<V, SQ>(x0, x1, SQ ? x0 : y0, SQ ? x1 : y1, s0, s1, s2);
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    o0[k] = barrett128(s0[k], q, r0, r1);
                    o1[k] = barrett128(SQ ? (s1[k] << 1) + o1[k] : s1[k], q, r0, r1);
                    o2[k] = barrett128(s2[k], q, r0, r1);
                }
            }
        }
        Lane<V>::store(d0 + p * a.d01_poly, o0);
        Lane<V>::store(d1 + p * a.d01_poly, o1);
        Lane<V>::store(d2 + p * a.d2_poly, o2);
    }
}

using CtmulKernel = void (*)(CtmulArgs, const uint64_t*);

template <int V, bool SQ>
static CtmulKernel pick_ctmul(int nt) {
    switch (nt) {
        case 1: return ctmul_tensor_kernel<1, V, SQ>;
        case 2: return ctmul_tensor_kernel<2, V, SQ>;
        case 3: return ctmul_tensor_kernel<3, V, SQ>;
        case 4: return ctmul_tensor_kernel<4, V, SQ>;
        case 5: return ctmul_tensor_kernel<5, V, SQ>;
        case 6: return ctmul_tensor_kernel<6, V, SQ>;
        default: return ctmul_tensor_kernel<0, V, SQ>;
    }
}
static_assert(kCtmulUnroll == 6 && kCtmulUnroll <= kCtmulFold, "pick_ctmul lists the unrolled term counts");

int launch_ctmul_tensor(mfhe_ctx* c, CtmulArgs a, hipStream_t st) {
    if (a.npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    const bool sq = !a.b0;
    if (sq) a.b_term = a.b_poly = 0;   // unread, and they do not bear on the form
    const bool wide = ks_wide({&a.ncoeff, &a.a_term, &a.a_poly, &a.b_term, &a.b_poly, &a.d01_poly, &a.d2_poly},
                              {a.a0, a.a1, a.b0, a.b1, a.d0, a.d1, a.d2});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull || a.level > 65535) return set_error(MFHE_EINVAL, "ctmul_tensor: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)a.level, (uint32_t)(a.npoly < 65535 ? a.npoly : 65535));
    const CtmulKernel k = wide ? (sq ? pick_ctmul<2, true>(a.nterms) : pick_ctmul<2, false>(a.nterms))
                               : (sq ? pick_ctmul<1, true>(a.nterms) : pick_ctmul<1, false>(a.nterms));
    hipLaunchKernelGGL(k, grid, dim3(rg.block), 0, st, a, (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ctmul_tensor_kernel");
    return MFHE_OK;
}

// The operands of a product as the entry points take them.
struct CtmulOperands {
    const uint64_t *a0, *a1;
    size_t a_term, a_poly;
    const uint64_t *b0, *b1;
    size_t b_term, b_poly;
    int nterms;
};

// Pointers, term count and strides of the operands (lw = level * N); in[0 .. *nin) = the ranges they span.
static int ctmul_check_operands(const std::string& w, const CtmulOperands& o, size_t npoly, size_t lw, KsRange in[4],
                                int* nin) {
    if (!o.a0 || !o.a1) return set_error(MFHE_EINVAL, w + ": null pointer");
    if (!o.b0 != !o.b1) return set_error(MFHE_EINVAL, w + ": exactly one of d_b0, d_b1 is null");
    if (o.nterms < 1 || o.nterms > kCtmulMaxTerms) return set_error(MFHE_EINVAL, w + ": nterms outside [1, 64]");
    if (o.a_poly < lw || (o.b0 && o.b_poly < lw)) return set_error(MFHE_EINVAL, w + ": poly stride smaller than level * N");
    const size_t apsp = ks_span(npoly, o.a_poly, lw), bpsp = o.b0 ? ks_span(npoly, o.b_poly, lw) : 0;
    if (npoly && (o.a_term < apsp || (o.b0 && o.b_term < bpsp)))
        return set_error(MFHE_EINVAL, w + ": term stride smaller than the polynomials of a term");
    const size_t asp = ks_span(o.nterms, o.a_term, apsp), bsp = ks_span(o.nterms, o.b_term, bpsp);
    *nin = 0;
    in[(*nin)++] = {o.a0, asp};
    in[(*nin)++] = {o.a1, asp};
    if (o.b0) {
        in[(*nin)++] = {o.b0, bsp};
        in[(*nin)++] = {o.b1, bsp};
    }
    return MFHE_OK;
}

static CtmulArgs ctmul_args(const CtmulOperands& o, uint64_t* d0, uint64_t* d1, size_t d01_poly, uint64_t* d2,
                            size_t d2_poly, size_t npoly, int level, size_t N) {
    CtmulArgs a{};
    a.a0 = o.a0; a.a1 = o.a1; a.b0 = o.b0; a.b1 = o.b1;
    a.d0 = d0; a.d1 = d1; a.d2 = d2;
    a.a_term = o.a_term; a.a_poly = o.a_poly; a.b_term = o.b0 ? o.b_term : 0; a.b_poly = o.b0 ? o.b_poly : 0;
    a.d01_poly = d01_poly; a.d2_poly = d2_poly;
    a.ncoeff = N; a.npoly = npoly; a.nterms = o.nterms; a.level = level;
    return a;
}

int ctmul_check_flags(const char* what, int flags, int level) {
    const std::string w(what);
    if (flags & ~MFHE_CTMUL_RESCALE) return set_error(MFHE_EINVAL, w + ": unknown flag");
    if ((flags & MFHE_CTMUL_RESCALE) && level == 1)
        return set_error(MFHE_EINVAL, w + ": MFHE_CTMUL_RESCALE at level 1 leaves no limb");
    return MFHE_OK;
}

int ctmul_prepare(mfhe_ctx* c, size_t npoly, const KsGeom& g, int alpha, int flags, KsTables& t) {
    const size_t words = ks_ws_words(npoly, ks_beta(g.level, alpha), (size_t)g.rows(), c->N) + npoly * g.level * c->N;
    return ks_prepare(c, g, alpha, (flags & MFHE_CTMUL_RESCALE) ? kKsRescale : 0, words, t);
}

int ctmul_relin_rescale(mfhe_ctx* c, const uint64_t* d_rlk, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride,
                        size_t npoly, const KsGeom& g, int alpha, const KsTables& t, int flags, hipStream_t st) {
    const size_t N = c->N, lw = (size_t)g.level * N;
    // the body of mfhe_keyswitch with MFHE_KS_ADD on d2
    RC(ks_switch_body(c, ctmul_d2(c, npoly, t.beta, g), lw, d_rlk, {d_out0, d_out1, out_poly_stride, 3}, npoly, g, alpha,
                      t, st));
    if (!(flags & MFHE_CTMUL_RESCALE)) return MFHE_OK;
    return ctmul_rescale(c, d_out0, d_out1, out_poly_stride, npoly, g, t, st);
}

int ctmul_rescale(mfhe_ctx* c, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride, size_t npoly,
                  const KsGeom& g, const KsTables& t, hipStream_t st) {
    const size_t N = c->N;
    // The rescale: mfhe_ntt_moddown(keep = level - 1, drop = limb level - 1) in place on each output, its scratch the
    // key switch's block.  The two outputs are one batch of 2 npoly polynomials when one follows the other at the
    // poly stride (any two single polynomials do); the work per polynomial is the same either way.
    const int keep = g.level - 1;
    const size_t kw = (size_t)keep * N;
    const uint64_t *rs = t.rescale, *cen = nullptr;
    uint64_t* lo = d_out0 < d_out1 ? d_out0 : d_out1;
    const size_t gap = (size_t)((d_out0 < d_out1 ? d_out1 : d_out0) - lo);
    const size_t batch_stride = npoly == 1 ? gap : gap == npoly * out_poly_stride ? out_poly_stride : 0;
    uint64_t* ws = (uint64_t*)c->ws;
    if (batch_stride) {
        RC(ntt_moddown_center(c, lo, batch_stride, 2 * npoly, keep, keep, 1, rs, ws, &cen, st));
        return launch_sub_scale(c, lo, batch_stride, cen, kw, lo, batch_stride, nullptr, 2 * npoly, keep, 1, rs, st);
    }
    for (uint64_t* o : {d_out0, d_out1}) {
        RC(ntt_moddown_center(c, o, out_poly_stride, npoly, keep, keep, 1, rs, ws, &cen, st));
        RC(launch_sub_scale(c, o, out_poly_stride, cen, kw, o, out_poly_stride, nullptr, npoly, keep, 1, rs, st));
    }
    return MFHE_OK;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ctmul_tensor(mfhe_ctx* c, const uint64_t* d_a0, const uint64_t* d_a1, size_t a_term_stride,
                                 size_t a_poly_stride, const uint64_t* d_b0, const uint64_t* d_b1, size_t b_term_stride,
                                 size_t b_poly_stride, int nterms, uint64_t* d_d0, uint64_t* d_d1,
                                 size_t d01_poly_stride, uint64_t* d_d2, size_t d2_poly_stride, size_t npoly, int level,
                                 mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_d0 || !d_d1 || !d_d2) return set_error(MFHE_EINVAL, "ctmul_tensor: null pointer");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ctmul_tensor: level outside the context");
    const size_t N = c->N, lw = (size_t)level * N;
    const CtmulOperands o{d_a0, d_a1, a_term_stride, a_poly_stride, d_b0, d_b1, b_term_stride, b_poly_stride, nterms};
    KsRange in[4];
    int nin = 0;
    RC(ctmul_check_operands("ctmul_tensor", o, npoly, lw, in, &nin));
    if (d01_poly_stride < lw || d2_poly_stride < lw)
        return set_error(MFHE_EINVAL, "ctmul_tensor: output poly stride smaller than level * N");
    const size_t osp = ks_span(npoly, d01_poly_stride, lw);
    const KsRange out[3] = {{d_d0, osp}, {d_d1, osp}, {d_d2, ks_span(npoly, d2_poly_stride, lw)}};
    RC(ks_check_overlap("ctmul_tensor", in, nin, out, 3));
    if (npoly == 0) return MFHE_OK;
    return launch_ctmul_tensor(c, ctmul_args(o, d_d0, d_d1, d01_poly_stride, d_d2, d2_poly_stride, npoly, level, N),
                               (hipStream_t)s);
}

extern "C" int mfhe_ctmul_reserve(mfhe_ctx* c, size_t npoly, int level, int key_level, int alpha, int special_start,
                                  int nspecial, int flags) {
    RC(ks_check_ctx(c));
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "ctmul_reserve"));
    RC(ctmul_check_flags("ctmul_reserve", flags, level));
    KsTables t;
    return ctmul_prepare(c, npoly, g, alpha, flags, t);
}

extern "C" int mfhe_ctmul_apply(mfhe_ctx* c, const uint64_t* d_a0, const uint64_t* d_a1, size_t a_term_stride,
                                size_t a_poly_stride, const uint64_t* d_b0, const uint64_t* d_b1, size_t b_term_stride,
                                size_t b_poly_stride, int nterms, const uint64_t* d_rlk, uint64_t* d_out0,
                                uint64_t* d_out1, size_t out_poly_stride, size_t npoly, int level, int key_level,
                                int alpha, int special_start, int nspecial, int flags, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_rlk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "ctmul_apply: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "ctmul_apply"));
    RC(ctmul_check_flags("ctmul_apply", flags, level));
    const size_t N = c->N, lw = (size_t)level * N;
    const CtmulOperands o{d_a0, d_a1, a_term_stride, a_poly_stride, d_b0, d_b1, b_term_stride, b_poly_stride, nterms};
    KsRange in[5];
    int nin = 0;
    RC(ctmul_check_operands("ctmul_apply", o, npoly, lw, in, &nin));
    if (out_poly_stride < lw) return set_error(MFHE_EINVAL, "ctmul_apply: output poly stride smaller than level * N");
    in[nin++] = {d_rlk, (size_t)ks_beta(level, alpha) * 2 * g.key_rows() * N};   // the key's digits read here
    const size_t osp = ks_span(npoly, out_poly_stride, lw);
    const KsRange out[2] = {{d_out0, osp}, {d_out1, osp}};
    RC(ks_check_overlap("ctmul_apply", in, nin, out, 2));
    if (npoly == 0) return MFHE_OK;
    // every table and the workspace before the first launch (nothing to do after mfhe_ctmul_reserve)
    KsTables t;
    RC(ctmul_prepare(c, npoly, g, alpha, flags, t));
    hipStream_t st = (hipStream_t)s;
    uint64_t* d2 = ctmul_d2(c, npoly, t.beta, g);   // [npoly][level][N]
    RC(launch_ctmul_tensor(c, ctmul_args(o, d_out0, d_out1, out_poly_stride, d2, lw, npoly, level, N), st));
    return ctmul_relin_rescale(c, d_rlk, d_out0, d_out1, out_poly_stride, npoly, g, alpha, t, flags, st);
}

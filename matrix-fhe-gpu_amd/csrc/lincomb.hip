// lincomb.hip -- scalar linear combinations of ciphertexts for gfx950 on the layout of the key switch: ciphertext x
// scalar, additions at a level and the constant term of a polynomial in one launch (include/mfhe.h mfhe_ct_lincomb).
//
// Everything is in the evaluation domain (phantom NTT) and canonical; a ciphertext is a pair of [level][N] polynomials
// and limb r is row r.
//
//   out_c[p][r][i] = sum_t K[term_k[t]][r] x_c[term_x[t]][p][r][i] + [c == 0, addend_k >= 0] K[addend_k][r]   mod q_r
//
// The constants are per-limb scalars: a constant polynomial is constant in the evaluation domain too, so the addend
// goes to every point of component 0 and to nothing of component 1.
//
// Design, as the multiply-accumulate of lintrans.hip: one thread owns one (row, coefficient) -- two adjacent
// coefficients with 16-byte accesses when the layout allows -- and walks a run of (polynomial, component) pairs.  The
// row is the grid's y index, so the modulus constants and the constants of the sum are scalar loads, made once per
// thread (nterms <= kLincombUnroll; longer sums re-read them per pair, from the scalar cache).  The sum is an
// unreduced u128: 16 products of canonical residues below 2^62 are below 2^128 - 2^67, so a carried residue (the
// addend at first) fits beside them; longer sums fold every 16 terms, and every sum ends in one 128-bit Barrett
// reduction.  The term index arrays are kernel arguments, so nothing is copied to the device.
#include "lincomb.hpp"

#include <hip/hip_runtime.h>

#include "mod128.hpp"

namespace mfhe {

// largest term count whose operands stay in registers (DESIGN.md §3.15 has the resource table behind it)
constexpr int kLincombUnroll = 8;
// terms between two reductions of the running sum
constexpr int kLincombFold = 16;
// shortest run of (polynomial, component) pairs one thread walks with its constants (the whole batch when smaller)
constexpr uint64_t kLincombMinRun = 4;

// NT: terms (template-unrolled, every operand in registers) or 0 (folded loop over a.nterms); V: coefficients per
// thread.  dmod and k are indexed by the block's row: scalar loads, as are the term indices (kernel arguments).
template <int NT, int V>
__global__ __launch_bounds__(256) void ct_lincomb_kernel(LincombArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t q = dmod[3 * r], r0 = dmod[3 * r + 1], r1 = dmod[3 * r + 2];
    const uint64_t* kp = a.k + r;
    const uint64_t ro = (uint64_t)r * a.ncoeff + c;
    const T* x0 = (const T*)a.x0 + ro;
    const T* x1 = (const T*)a.x1 + ro;
    T* o0 = (T*)a.o0 + ro;
    T* o1 = (T*)a.o1 + ro;
    const uint64_t add = a.addend_k >= 0 ? kp[(uint64_t)a.addend_k * a.k_stride] : 0;
    const uint64_t pc0 = blockIdx.z * a.prun;
    const uint64_t pc1 = pc0 + a.prun < a.npairs ? pc0 + a.prun : a.npairs;

    if (NT) {
        constexpr int NK = NT ? NT : 1;
        uint64_t w[NK];
#pragma unroll
        for (int t = 0; t < NK; ++t) w[t] = kp[(uint64_t)a.term_k[t] * a.k_stride];
        for (uint64_t pc = pc0; pc < pc1; ++pc) {
            const uint64_t p = pc >> 1;
            const bool one = pc & 1;
            const T* xp = (one ? x1 : x0) + p * a.x_poly;
            uint64_t x[NK][V];
#pragma unroll
            for (int t = 0; t < NK; ++t) Lane<V>::load(xp + (uint64_t)a.term_x[t] * a.src_stride, x[t]);
            u128 s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = one ? 0 : add;
#pragma unroll
            for (int t = 0; t < NK; ++t)
#pragma unroll
                for (int k = 0; k < V; ++k) s[k] += (u128)x[t][k] * w[t];
            uint64_t o[V];
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = barrett128(s[k], q, r0, r1);
            Lane<V>::store((one ? o1 : o0) + p * a.o_poly, o);
        }
    } else {
        for (uint64_t pc = pc0; pc < pc1; ++pc) {
            const uint64_t p = pc >> 1;
            const bool one = pc & 1;
            const T* xp = (one ? x1 : x0) + p * a.x_poly;
            uint64_t o[V];
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = one ? 0 : add;
            for (int t0 = 0; t0 < a.nterms; t0 += kLincombFold) {   // 16 products and a residue fit a u128
                u128 s[V];
#pragma unroll
                for (int k = 0; k < V; ++k) s[k] = o[k];
                const int t1 = t0 + kLincombFold < a.nterms ? t0 + kLincombFold : a.nterms;
                for (int t = t0; t < t1; ++t) {
                    uint64_t x[V];
                    Lane<V>::load(xp + (uint64_t)a.term_x[t] * a.src_stride, x);
                    const uint64_t w = kp[(uint64_t)a.term_k[t] * a.k_stride];
#pragma unroll
                    for (int k = 0; k < V; ++k) s[k] += (u128)x[k] * w;
                }
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = barrett128(s[k], q, r0, r1);
            }
            Lane<V>::store((one ? o1 : o0) + p * a.o_poly, o);
        }
    }
}

using LincombKernel = void (*)(LincombArgs, const uint64_t*);

template <int V>
static LincombKernel pick_lincomb(int nt) {
    switch (nt) {
        case 1: return ct_lincomb_kernel<1, V>;
        case 2: return ct_lincomb_kernel<2, V>;
        case 3: return ct_lincomb_kernel<3, V>;
        case 4: return ct_lincomb_kernel<4, V>;
        case 5: return ct_lincomb_kernel<5, V>;
        case 6: return ct_lincomb_kernel<6, V>;
        case 7: return ct_lincomb_kernel<7, V>;
        case 8: return ct_lincomb_kernel<8, V>;
        default: return ct_lincomb_kernel<0, V>;
    }
}
static_assert(kLincombUnroll == 8 && kLincombUnroll <= kLincombFold, "pick_lincomb lists the unrolled term counts");

int launch_ct_lincomb(mfhe_ctx* c, LincombArgs a, size_t npoly, hipStream_t st) {
    if (npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    const bool wide = ks_wide({&a.ncoeff, &a.src_stride, &a.x_poly, &a.o_poly}, {a.x0, a.x1, a.o0, a.o1});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull || a.level > 65535) return set_error(MFHE_EINVAL, "ct_lincomb: too large for one launch");
    a.npairs = 2 * (uint64_t)npoly;
    const KsRuns run = ks_runs(a.npairs, rg.bx, (uint64_t)a.level, kLincombMinRun);   // a thread keeps its constants across a run
    a.prun = run.prun;
    const LincombKernel k = wide ? pick_lincomb<2>(a.nterms) : pick_lincomb<1>(a.nterms);
    hipLaunchKernelGGL(k, dim3((uint32_t)rg.bx, (uint32_t)a.level, (uint32_t)run.runs), dim3(rg.block), 0, st, a,
                       (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ct_lincomb_kernel");
    return MFHE_OK;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ct_lincomb(mfhe_ctx* c, const uint64_t* d_x0, const uint64_t* d_x1, size_t src_stride,
                               size_t x_poly_stride, int nsrc, const uint64_t* d_k, size_t k_stride, int nk,
                               const int* term_x, const int* term_k, int nterms, int addend_k, uint64_t* d_out0,
                               uint64_t* d_out1, size_t out_poly_stride, size_t npoly, int level, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_x0 || !d_x1 || !d_k || !d_out0 || !d_out1 || !term_x || !term_k)
        return set_error(MFHE_EINVAL, "ct_lincomb: null pointer");
    if (nterms < 1 || nterms > kLincombMaxTerms) return set_error(MFHE_EINVAL, "ct_lincomb: nterms outside [1, 64]");
    if (nsrc < 1 || nk < 1) return set_error(MFHE_EINVAL, "ct_lincomb: nsrc or nk < 1");
    for (int t = 0; t < nterms; ++t)
        if (term_x[t] < 0 || term_x[t] >= nsrc || term_k[t] < 0 || term_k[t] >= nk)
            return set_error(MFHE_EINVAL, "ct_lincomb: a term index is out of range");
    if (addend_k < -1 || addend_k >= nk) return set_error(MFHE_EINVAL, "ct_lincomb: addend_k outside [-1, nk)");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ct_lincomb: level outside the context");
    const size_t N = c->N, lw = (size_t)level * N;
    if (x_poly_stride < lw || out_poly_stride < lw)
        return set_error(MFHE_EINVAL, "ct_lincomb: poly stride smaller than level * N");
    const size_t xsp = ks_span(npoly, x_poly_stride, lw);
    if (npoly && src_stride < xsp)
        return set_error(MFHE_EINVAL, "ct_lincomb: source stride smaller than the polynomials of a source");
    if (k_stride < (size_t)level) return set_error(MFHE_EINVAL, "ct_lincomb: constant stride smaller than level");
    const size_t ssp = ks_span(nsrc, src_stride, xsp), osp = ks_span(npoly, out_poly_stride, lw);
    RC(ks_check_overlap("ct_lincomb", {{d_x0, ssp}, {d_x1, ssp}, {d_k, ks_span(nk, k_stride, level)}},
                        {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    LincombArgs a{};
    a.x0 = d_x0; a.x1 = d_x1; a.k = d_k; a.o0 = d_out0; a.o1 = d_out1;
    a.src_stride = src_stride; a.x_poly = x_poly_stride; a.o_poly = out_poly_stride; a.k_stride = k_stride;
    a.ncoeff = N; a.nterms = nterms; a.level = level; a.addend_k = addend_k;
    for (int t = 0; t < nterms; ++t) {
        a.term_x[t] = term_x[t];
        a.term_k[t] = term_k[t];
    }
    return launch_ct_lincomb(c, a, npoly, (hipStream_t)s);
}

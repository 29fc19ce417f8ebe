// ctmat.hip -- products of matrices of ciphertexts for gfx950 on the layout of the key switch: the tiled tensor sum
// and the driver that chains it with one relinearisation and one rescale over the whole product (include/mfhe.h
// mfhe_ctmat_tensor, mfhe_ctmat_apply, mfhe_ctmat_reserve).
//
// Domain, geometry and conventions are ctmul.hip's.  C = A B for an m x k matrix A and a k x n matrix B of
// ciphertexts, every entry npoly polynomials per component:
//
//   tensor : d0[i][j] = sum_t a0[i][t] b0[t][j], d1[i][j] = sum_t (a0[i][t] b1[t][j] + a1[i][t] b0[t][j]),
//            d2[i][j] = sum_t a1[i][t] b1[t][j] mod q_r, one launch; bit-identical to m n calls of mfhe_ctmul_tensor
//   apply  : tensor with d0, d1 in the outputs [m][n][npoly][level][N] and d2 in the workspace, then the tail of
//            mfhe_ctmul_apply once over the m n npoly polynomials: one key switch and one rescale per product
//
// Tensor design: ctmul_tensor_kernel's thread -- one (row, coefficient), or two adjacent coefficients with 16-byte
// accesses -- owns a TM x TN tile of outputs.  Per term it loads the TM entries of A and the TN entries of B once and
// forms all TM TN 4 products, 2 (TM + TN) / (TM TN) loads per term per output where separate dot products take 4.  The
// sums are unreduced u128 and fold every kCtmulFold terms with the reduced residues carried in, as ctmul.hip's chunked
// loop.  Tiles x polynomials fold over blockIdx.z; the row is the grid's y index, so the modulus constants are scalar
// loads.  A tile at the edge of the product (m or n no multiple of the tile) runs the instantiation of its own shape,
// chosen on a condition uniform over the block: nothing outside the operands is read and no lane is predicated inside
// the product loop.
#include "ctmat.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "mod128.hpp"

namespace mfhe {

// The tile, rows of A by columns of B, and the build knobs behind the trials of DESIGN.md §3.13 (make EXTRA=-D...;
// the product library is built at these defaults): MFHE_CTMAT_WIDE 0 keeps the scalar form on every layout,
// MFHE_CTMAT_UNROLL unrolls the term loop, MFHE_CTMAT_WAVES is the waves per SIMD the register allocator must leave
// room for (unbounded, it spends 168 to 256 registers on hoisted loads; above 3 the 16-byte form spills).
#ifndef MFHE_CTMAT_TM
#define MFHE_CTMAT_TM 2
#endif
#ifndef MFHE_CTMAT_TN
#define MFHE_CTMAT_TN 2
#endif
#ifndef MFHE_CTMAT_WIDE
#define MFHE_CTMAT_WIDE 1
#endif
#ifndef MFHE_CTMAT_UNROLL
#define MFHE_CTMAT_UNROLL 1
#endif
#ifndef MFHE_CTMAT_WAVES
#define MFHE_CTMAT_WAVES 3
#endif
constexpr int kCtmatTM = MFHE_CTMAT_TM, kCtmatTN = MFHE_CTMAT_TN;
static_assert(kCtmatTM >= 2 && kCtmatTN >= 2, "the tile is at least 2 x 2 outputs");

// A block's view of a tile of one polynomial on its row: the operands at (i0, 0) and (0, j0), the outputs at (i0, j0).
// Everything here is uniform over the block and computed in scalar registers; a lane adds its 32-bit offset in bytes.
template <int V>
struct CtmatTile {
    using T = typename Lane<V>::T;
    const T *a0, *a1, *b0, *b1;
    T *d0, *d1, *d2;
    uint64_t q, r0, r1;
    static __device__ __forceinline__ const T* at(const T* p, uint32_t off) {
        return (const T*)((const char*)p + off);
    }
    static __device__ __forceinline__ T* at(T* p, uint32_t off) { return (T*)((char*)p + off); }
};

// RM x RN outputs of one (row, coefficient): every entry of A and B is loaded once per term
template <int V, int RM, int RN>
static __device__ __forceinline__ void ctmat_tile(const CtmatArgs& a, const CtmatTile<V>& x, uint32_t off) {
    using X = CtmatTile<V>;
    uint64_t o0[RM][RN][V], o1[RM][RN][V], o2[RM][RN][V];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) o0[i][j][v] = o1[i][j][v] = o2[i][j][v] = 0;
    // 16 products < 2^124 and a residue < 2^62 fit a u128
    for (int t0 = 0; t0 < a.k; t0 += kCtmulFold) {
        u128 s0[RM][RN][V], s1[RM][RN][V], s2[RM][RN][V];
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    s0[i][j][v] = o0[i][j][v];
                    s1[i][j][v] = o1[i][j][v];
                    s2[i][j][v] = o2[i][j][v];
                }
        const int t1 = t0 + kCtmulFold < a.k ? t0 + kCtmulFold : a.k;
#pragma unroll MFHE_CTMAT_UNROLL
        for (int t = t0; t < t1; ++t) {
            uint64_t x0[RM][V], x1[RM][V], y0[RN][V], y1[RN][V];
#pragma unroll
            for (int i = 0; i < RM; ++i) {
                Lane<V>::load(X::at(x.a0 + i * a.a_row + t * a.a_col, off), x0[i]);
                Lane<V>::load(X::at(x.a1 + i * a.a_row + t * a.a_col, off), x1[i]);
            }
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                Lane<V>::load(X::at(x.b0 + t * a.b_row + j * a.b_col, off), y0[j]);
                Lane<V>::load(X::at(x.b1 + t * a.b_row + j * a.b_col, off), y1[j]);
            }
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
                    ct_term<V, false>(x0[i], x1[i], y0[j], y1[j], s0[i][j], s1[i][j], s2[i][j]);
        }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    o0[i][j][v] = barrett128(s0[i][j][v], x.q, x.r0, x.r1);
                    o1[i][j][v] = barrett128(s1[i][j][v], x.q, x.r0, x.r1);
                    o2[i][j][v] = barrett128(s2[i][j][v], x.q, x.r0, x.r1);
                }
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            Lane<V>::store(X::at(x.d0 + i * a.d01_row + j * a.d01_col, off), o0[i][j]);
            Lane<V>::store(X::at(x.d1 + i * a.d01_row + j * a.d01_col, off), o1[i][j]);
            Lane<V>::store(X::at(x.d2 + i * a.d2_row + j * a.d2_col, off), o2[i][j]);
        }
}

// the instantiation of a tile's own shape, rm <= RM rows and rn <= RN columns (both uniform over the block)
template <int V, int RM, int RN>
static __device__ __forceinline__ void ctmat_cols(const CtmatArgs& a, const CtmatTile<V>& x, uint32_t off, int rn) {
    if (rn == RN)
        ctmat_tile<V, RM, RN>(a, x, off);
    else if constexpr (RN > 1)
        ctmat_cols<V, RM, RN - 1>(a, x, off, rn);
}
template <int V, int RM, int TN>
static __device__ __forceinline__ void ctmat_rows(const CtmatArgs& a, const CtmatTile<V>& x, uint32_t off, int rm,
                                                  int rn) {
    if (rm == RM)
        ctmat_cols<V, RM, TN>(a, x, off, rn);
    else if constexpr (RM > 1)
        ctmat_rows<V, RM - 1, TN>(a, x, off, rm, rn);
}

// V: coefficients per thread; TM x TN: the tile.  Work item w = tile * npoly + polynomial, tiles row-major over
// ceil(m / TM) x ceil(n / TN).  dmod is indexed by the block's row: scalar loads.
template <int V, int TM, int TN>
__global__ __launch_bounds__(256, MFHE_CTMAT_WAVES) void ctmat_tensor_kernel(CtmatArgs a,
                                                                             const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t ro = (uint64_t)r * a.ncoeff;                  // the row: uniform
    const uint32_t off = (uint32_t)c * (uint32_t)sizeof(T);      // the lane: below 2^32 bytes, the launcher checks
    const uint32_t tn = ((uint32_t)a.n + TN - 1) / TN;
    CtmatTile<V> x;
    x.q = dmod[3 * r];
    x.r0 = dmod[3 * r + 1];
    x.r1 = dmod[3 * r + 2];

    for (uint64_t w = blockIdx.z; w < a.nwork; w += gridDim.z) {
        // 32-bit divisions of uniform values, kept in scalar registers (nwork < 2^32, the launcher checks)
        const uint32_t tile = __builtin_amdgcn_readfirstlane((uint32_t)w / (uint32_t)a.npoly);
        const uint32_t p = (uint32_t)w - tile * (uint32_t)a.npoly;
        const uint32_t ti = __builtin_amdgcn_readfirstlane(tile / tn), tj = tile - ti * tn;
        const uint64_t i0 = (uint64_t)ti * TM, j0 = (uint64_t)tj * TN;
        const int rm = a.m - (int)i0 < TM ? a.m - (int)i0 : TM, rn = a.n - (int)j0 < TN ? a.n - (int)j0 : TN;
        const uint64_t ao = ro + i0 * a.a_row + (uint64_t)p * a.a_poly;
        const uint64_t bo = ro + j0 * a.b_col + (uint64_t)p * a.b_poly;
        const uint64_t o01 = ro + i0 * a.d01_row + j0 * a.d01_col + (uint64_t)p * a.d01_poly;
        x.a0 = (const T*)a.a0 + ao;
        x.a1 = (const T*)a.a1 + ao;
        x.b0 = (const T*)a.b0 + bo;
        x.b1 = (const T*)a.b1 + bo;
        x.d0 = (T*)a.d0 + o01;
        x.d1 = (T*)a.d1 + o01;
        x.d2 = (T*)a.d2 + ro + i0 * a.d2_row + j0 * a.d2_col + (uint64_t)p * a.d2_poly;
        ctmat_rows<V, TM, TN>(a, x, off, rm, rn);
    }
}

int launch_ctmat_tensor(mfhe_ctx* c, CtmatArgs a, hipStream_t st) {
    if (a.npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    const bool wide = MFHE_CTMAT_WIDE &&
                      ks_wide({&a.ncoeff, &a.a_row, &a.a_col, &a.a_poly, &a.b_row, &a.b_col, &a.b_poly, &a.d01_row,
                               &a.d01_col, &a.d01_poly, &a.d2_row, &a.d2_col, &a.d2_poly},
                              {a.a0, a.a1, a.b0, a.b1, a.d0, a.d1, a.d2});
    const uint64_t tiles = (((uint64_t)a.m + kCtmatTM - 1) / kCtmatTM) * (((uint64_t)a.n + kCtmatTN - 1) / kCtmatTN);
    a.nwork = tiles * a.npoly;
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull || a.level > 65535 || a.ncoeff > (1ull << 28) || a.nwork / tiles != a.npoly ||
        a.nwork > 0xffffffffull)
        return set_error(MFHE_EINVAL, "ctmat_tensor: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)a.level, (uint32_t)(a.nwork < 65535 ? a.nwork : 65535));
    if (wide)
        hipLaunchKernelGGL((ctmat_tensor_kernel<2, kCtmatTM, kCtmatTN>), grid, dim3(rg.block), 0, st, a,
                           (const uint64_t*)c->d_dmod);
    else
        hipLaunchKernelGGL((ctmat_tensor_kernel<1, kCtmatTM, kCtmatTN>), grid, dim3(rg.block), 0, st, a,
                           (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ctmat_tensor_kernel");
    return MFHE_OK;
}

// The operands of a matrix product as the entry points take them.
struct CtmatOperands {
    const uint64_t *a0, *a1;
    size_t a_row, a_col, a_poly;
    const uint64_t *b0, *b1;
    size_t b_row, b_col, b_poly;
    int m, n, k;
};

// Pointers, shape and strides of the operands (lw = level * N); in[0 .. 4) = the ranges they span.
static int ctmat_check_operands(const std::string& w, const CtmatOperands& o, size_t npoly, size_t lw,
                                KsRange in[4]) {
    if (!o.a0 || !o.a1 || !o.b0 || !o.b1) return set_error(MFHE_EINVAL, w + ": null pointer");
    if (o.m < 1 || o.n < 1) return set_error(MFHE_EINVAL, w + ": m or n < 1");
    if (o.k < 1 || o.k > kCtmulMaxTerms) return set_error(MFHE_EINVAL, w + ": k outside [1, 64]");
    if (o.a_poly < lw || o.b_poly < lw) return set_error(MFHE_EINVAL, w + ": poly stride smaller than level * N");
    size_t asp = 0, bsp = 0;
    if (!ctmat_span({(size_t)o.m, (size_t)o.k, o.a_row, o.a_col, o.a_poly}, npoly, lw, &asp))
        return set_error(MFHE_EINVAL, w + ": entries of A overlap at these strides");
    if (!ctmat_span({(size_t)o.k, (size_t)o.n, o.b_row, o.b_col, o.b_poly}, npoly, lw, &bsp))
        return set_error(MFHE_EINVAL, w + ": entries of B overlap at these strides");
    in[0] = {o.a0, asp};
    in[1] = {o.a1, asp};
    in[2] = {o.b0, bsp};
    in[3] = {o.b1, bsp};
    return MFHE_OK;
}

static CtmatArgs ctmat_args(const CtmatOperands& o, uint64_t* d0, uint64_t* d1, const CtmatMatrix& d01, uint64_t* d2,
                            const CtmatMatrix& d2s, size_t npoly, int level, size_t N) {
    CtmatArgs a{};
    a.a0 = o.a0; a.a1 = o.a1; a.b0 = o.b0; a.b1 = o.b1;
    a.d0 = d0; a.d1 = d1; a.d2 = d2;
    a.a_row = o.a_row; a.a_col = o.a_col; a.a_poly = o.a_poly;
    a.b_row = o.b_row; a.b_col = o.b_col; a.b_poly = o.b_poly;
    a.d01_row = d01.row; a.d01_col = d01.col; a.d01_poly = d01.poly;
    a.d2_row = d2s.row; a.d2_col = d2s.col; a.d2_poly = d2s.poly;
    a.ncoeff = N; a.npoly = npoly; a.m = o.m; a.n = o.n; a.k = o.k; a.level = level;
    return a;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ctmat_tensor(mfhe_ctx* c, const uint64_t* d_a0, const uint64_t* d_a1, size_t a_row_stride,
                                 size_t a_col_stride, size_t a_poly_stride, const uint64_t* d_b0, const uint64_t* d_b1,
                                 size_t b_row_stride, size_t b_col_stride, size_t b_poly_stride, int m, int n, int k,
                                 uint64_t* d_d0, uint64_t* d_d1, size_t d01_row_stride, size_t d01_col_stride,
                                 size_t d01_poly_stride, uint64_t* d_d2, size_t d2_row_stride, size_t d2_col_stride,
                                 size_t d2_poly_stride, size_t npoly, int level, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_d0 || !d_d1 || !d_d2) return set_error(MFHE_EINVAL, "ctmat_tensor: null pointer");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ctmat_tensor: level outside the context");
    const size_t N = c->N, lw = (size_t)level * N;
    const CtmatOperands o{d_a0, d_a1, a_row_stride, a_col_stride, a_poly_stride, d_b0, d_b1, b_row_stride,
                          b_col_stride, b_poly_stride, m, n, k};
    KsRange in[4];
    RC(ctmat_check_operands("ctmat_tensor", o, npoly, lw, in));
    if (d01_poly_stride < lw || d2_poly_stride < lw)
        return set_error(MFHE_EINVAL, "ctmat_tensor: output poly stride smaller than level * N");
    const CtmatMatrix d01{(size_t)m, (size_t)n, d01_row_stride, d01_col_stride, d01_poly_stride};
    const CtmatMatrix d2s{(size_t)m, (size_t)n, d2_row_stride, d2_col_stride, d2_poly_stride};
    size_t osp = 0, o2sp = 0;
    if (!ctmat_span(d01, npoly, lw, &osp) || !ctmat_span(d2s, npoly, lw, &o2sp))
        return set_error(MFHE_EINVAL, "ctmat_tensor: entries of an output overlap at these strides");
    const KsRange out[3] = {{d_d0, osp}, {d_d1, osp}, {d_d2, o2sp}};
    RC(ks_check_overlap("ctmat_tensor", in, 4, out, 3));
    if (npoly == 0) return MFHE_OK;
    return launch_ctmat_tensor(c, ctmat_args(o, d_d0, d_d1, d01, d_d2, d2s, npoly, level, N), (hipStream_t)s);
}


extern "C" int mfhe_ctmat_reserve(mfhe_ctx* c, int m, int n, size_t npoly, int level, int key_level, int alpha,
                                  int special_start, int nspecial, int flags) {
    RC(ks_check_ctx(c));
    if (m < 1 || n < 1) return set_error(MFHE_EINVAL, "ctmat_reserve: m or n < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "ctmat_reserve"));
    RC(ctmul_check_flags("ctmat_reserve", flags, level));
    size_t batch = 0;
    if (!ctmat_batch(m, n, npoly, &batch)) return set_error(MFHE_EINVAL, "ctmat_reserve: m n npoly overflows");
    KsTables t;
    return ctmul_prepare(c, batch, g, alpha, flags, t);
}

extern "C" int mfhe_ctmat_apply(mfhe_ctx* c, const uint64_t* d_a0, const uint64_t* d_a1, size_t a_row_stride,
                                size_t a_col_stride, size_t a_poly_stride, const uint64_t* d_b0, const uint64_t* d_b1,
                                size_t b_row_stride, size_t b_col_stride, size_t b_poly_stride, int m, int n, int k,
                                const uint64_t* d_rlk, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride,
                                size_t npoly, int level, int key_level, int alpha, int special_start, int nspecial,
                                int flags, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_rlk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "ctmat_apply: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "ctmat_apply"));
    RC(ctmul_check_flags("ctmat_apply", flags, level));
    const size_t N = c->N, lw = (size_t)level * N;
    const CtmatOperands o{d_a0, d_a1, a_row_stride, a_col_stride, a_poly_stride, d_b0, d_b1, b_row_stride,
                          b_col_stride, b_poly_stride, m, n, k};
    KsRange in[5];
    RC(ctmat_check_operands("ctmat_apply", o, npoly, lw, in));
    if (out_poly_stride < lw) return set_error(MFHE_EINVAL, "ctmat_apply: output poly stride smaller than level * N");
    size_t batch = 0;
    if (!ctmat_batch(m, n, npoly, &batch)) return set_error(MFHE_EINVAL, "ctmat_apply: m n npoly overflows");
    in[4] = {d_rlk, (size_t)ks_beta(level, alpha) * 2 * g.key_rows() * N};   // the key's digits read here
    const size_t osp = ks_span(batch, out_poly_stride, lw);
    const KsRange out[2] = {{d_out0, osp}, {d_out1, osp}};
    RC(ks_check_overlap("ctmat_apply", in, 5, out, 2));
    if (npoly == 0) return MFHE_OK;
    // every table and the workspace before the first launch (nothing to do after mfhe_ctmat_reserve)
    KsTables t;
    RC(ctmul_prepare(c, batch, g, alpha, flags, t));
    hipStream_t st = (hipStream_t)s;
    uint64_t* d2 = ctmul_d2(c, batch, t.beta, g);   // [m][n][npoly][level][N]

    // entry (i, j) of the outputs and of d2 is polynomials (i n + j) npoly .. of the batch
    const CtmatMatrix d01{(size_t)m, (size_t)n, (size_t)n * npoly * out_poly_stride, npoly * out_poly_stride,
                          out_poly_stride};
    const CtmatMatrix d2s{(size_t)m, (size_t)n, (size_t)n * npoly * lw, npoly * lw, lw};
    RC(launch_ctmat_tensor(c, ctmat_args(o, d_out0, d_out1, d01, d2, d2s, npoly, level, N), st));
    return ctmul_relin_rescale(c, d_rlk, d_out0, d_out1, out_poly_stride, batch, g, alpha, t, flags, st);
}

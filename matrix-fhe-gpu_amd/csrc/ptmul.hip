// ptmul.hip -- plaintext x ciphertext products for gfx950 on the layout of the key switch: the plaintext-weighted sum
// of ciphertexts, the tiled product of a matrix of plaintexts with a matrix of ciphertexts, and the driver that chains
// the latter with one rescale over the whole product (include/mfhe.h mfhe_ptmul_sum, mfhe_ptmat_tensor,
// mfhe_ptmat_reserve, mfhe_ptmat_apply).
//
// Domain and conventions are ctmul.hip's: everything is in the evaluation domain (phantom NTT) and canonical, a
// ciphertext is a pair of [level][N] polynomials, limb r is row r.  A plaintext is one [>= level rows][N] polynomial
// (mfhe_slot_encode with nspecial = 0 writes one); no special limbs, no key.
//
//   sum    : out_c[p] = sum_t pt[term_pt[t]][p'] x_c[term_x[t]][p] + [c == 0] pt[addend_pt][p']   mod q_r
//   tensor : out0[i][j] = sum_t w[i][t] x0[t][j] + bias[i][j], out1[i][j] = sum_t w[i][t] x1[t][j]  mod q_r, one launch;
//            bit-identical to m n sums
//   apply  : tensor into [m][n][npoly][level][N], then with MFHE_PTMUL_RESCALE one ModDown by limb level - 1 over all
//            m n npoly polynomials of both components
//
// Design.  Both kernels are row kernels of ctmat.hip's family: one thread owns one (row, coefficient) -- two adjacent
// coefficients with 16-byte accesses when the layout allows -- the row is the grid's y index, so the modulus constants
// are scalar loads, and the work items fold over blockIdx.z.  A thread of the sum owns both components of one output
// polynomial, so a plaintext is loaded once for the two products it enters; its term indices are kernel arguments.  A
// thread of the tensor owns a TM x TN tile of outputs, TM on the plaintext side: per term it loads the TM entries of W
// and the TN entries of X (two components) once and forms all 2 TM TN products, (TM + 2 TN) / (TM TN) loads per term
// per output where separate sums take 3.  The sums are unreduced u128 and fold every kPtmulFold terms (ptmul.hpp has
// the bound) with the reduced residues carried in; the bias and, with MFHE_PTMUL_ADD, the outputs' present contents
// are what the first fold carries.  A tile at the edge of the product runs the instantiation of its own shape, chosen
// on a condition uniform over the block: nothing outside the operands is read and no lane is predicated inside the
// product loop.
#include "ptmul.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "mod128.hpp"

namespace mfhe {

// The tile, rows of W by columns of X, and the build knobs behind the trials of DESIGN.md §3.17 (make EXTRA=-D...; the
// product library is built at these defaults, the fastest tile measured there): MFHE_PTMAT_WIDE 0 keeps the scalar
// form on every layout, MFHE_PTMAT_WAVES is the waves per SIMD the register allocator must leave room for (0: no
// bound; unbounded, the 4 x 2 16-byte form takes 256 registers and 12 AGPRs for one wave, and above 2 it spills).
// mfhe_ptmat_tile reports the tile a library was built with.
#ifndef MFHE_PTMAT_TM
#define MFHE_PTMAT_TM 4
#endif
#ifndef MFHE_PTMAT_TN
#define MFHE_PTMAT_TN 2
#endif
#ifndef MFHE_PTMAT_WIDE
#define MFHE_PTMAT_WIDE 1
#endif
#ifndef MFHE_PTMAT_WAVES
#define MFHE_PTMAT_WAVES 2
#endif
#if MFHE_PTMAT_WAVES
#define MFHE_PTMAT_BOUNDS __launch_bounds__(256, MFHE_PTMAT_WAVES)
#else
#define MFHE_PTMAT_BOUNDS __launch_bounds__(256)
#endif
constexpr int kPtmatTM = MFHE_PTMAT_TM, kPtmatTN = MFHE_PTMAT_TN;
static_assert(kPtmatTM >= 1 && kPtmatTN >= 1, "the tile holds an output");

// ---- the plaintext-weighted sum ----
// V: coefficients per thread.  Work item: one polynomial, both components.  dmod is indexed by the block's row and the
// term indices are kernel arguments: scalar loads.
template <int V>
__global__ __launch_bounds__(256) void ptmul_sum_kernel(PtmulArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t q = dmod[3 * r], r0 = dmod[3 * r + 1], r1 = dmod[3 * r + 2];
    const uint64_t ro = (uint64_t)r * a.ncoeff + c;

    for (uint64_t p = blockIdx.z; p < a.npoly; p += gridDim.z) {
        const T* x0 = (const T*)a.x0 + ro + p * a.x_poly;
        const T* x1 = (const T*)a.x1 + ro + p * a.x_poly;
        const T* pt = (const T*)a.pt + ro + p * a.pt_poly;
        uint64_t o0[V], o1[V];
#pragma unroll
        for (int v = 0; v < V; ++v) o0[v] = o1[v] = 0;
        if (a.addend_pt >= 0) Lane<V>::load(pt + (uint64_t)a.addend_pt * a.pt_stride, o0);
        for (int t0 = 0; t0 < a.nterms; t0 += kPtmulFold) {   // kPtmulFold products and a residue fit a u128
            u128 s0[V], s1[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                s0[v] = o0[v];
                s1[v] = o1[v];
            }
            const int t1 = t0 + kPtmulFold < a.nterms ? t0 + kPtmulFold : a.nterms;
            for (int t = t0; t < t1; ++t) {
                uint64_t w[V], y0[V], y1[V];
                const uint64_t xo = (uint64_t)a.term_x[t] * a.src_stride;
                Lane<V>::load(pt + (uint64_t)a.term_pt[t] * a.pt_stride, w);
                Lane<V>::load(x0 + xo, y0);
                Lane<V>::load(x1 + xo, y1);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    s0[v] += (u128)w[v] * y0[v];
                    s1[v] += (u128)w[v] * y1[v];
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                o0[v] = barrett128(s0[v], q, r0, r1);
                o1[v] = barrett128(s1[v], q, r0, r1);
            }
        }
        Lane<V>::store((T*)a.o0 + ro + p * a.o_poly, o0);
        Lane<V>::store((T*)a.o1 + ro + p * a.o_poly, o1);
    }
}

int launch_ptmul_sum(mfhe_ctx* c, PtmulArgs a, hipStream_t st) {
    if (a.npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    const bool wide = ks_wide({&a.ncoeff, &a.src_stride, &a.x_poly, &a.pt_stride, &a.pt_poly, &a.o_poly},
                              {a.x0, a.x1, a.pt, a.o0, a.o1});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull || a.level > 65535) return set_error(MFHE_EINVAL, "ptmul_sum: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)a.level, (uint32_t)(a.npoly < 65535 ? a.npoly : 65535));
    if (wide)
        hipLaunchKernelGGL(ptmul_sum_kernel<2>, grid, dim3(rg.block), 0, st, a, (const uint64_t*)c->d_dmod);
    else
        hipLaunchKernelGGL(ptmul_sum_kernel<1>, grid, dim3(rg.block), 0, st, a, (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ptmul_sum_kernel");
    return MFHE_OK;
}

// ---- the tiled product ----
// A block's view of a tile of one polynomial on its row: W at (i0, 0), X at (0, j0), the bias and the outputs at
// (i0, j0).  Everything here is uniform over the block and computed in scalar registers; a lane adds its 32-bit offset
// in bytes.
template <int V>
struct PtmatTile {
    using T = typename Lane<V>::T;
    const T *w, *x0, *x1, *b;
    T *o0, *o1;
    uint64_t q, r0, r1;
    static __device__ __forceinline__ const T* at(const T* p, uint32_t off) {
        return (const T*)((const char*)p + off);
    }
    static __device__ __forceinline__ T* at(T* p, uint32_t off) { return (T*)((char*)p + off); }
};

// RM x RN outputs of one (row, coefficient): every entry of W and X is loaded once per term
template <int V, int RM, int RN>
static __device__ __forceinline__ void ptmat_tile(const PtmatArgs& a, const PtmatTile<V>& x, uint32_t off) {
    using X = PtmatTile<V>;
    uint64_t o0[RM][RN][V], o1[RM][RN][V];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) o0[i][j][v] = o1[i][j][v] = 0;
    // what the first fold carries: the bias and the outputs' contents, two residues at most (both conditions uniform)
    if (a.bias) {
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j) Lane<V>::load(X::at(x.b + i * a.b_row + j * a.b_col, off), o0[i][j]);
    }
    if (a.add) {
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                uint64_t c0[V];
                Lane<V>::load(X::at(x.o0 + i * a.o_row + j * a.o_col, off), c0);
                Lane<V>::load(X::at(x.o1 + i * a.o_row + j * a.o_col, off), o1[i][j]);
#pragma unroll
                for (int v = 0; v < V; ++v) o0[i][j][v] += c0[v];
            }
    }
    for (int t0 = 0; t0 < a.k; t0 += kPtmulFold) {
        u128 s0[RM][RN][V], s1[RM][RN][V];
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    s0[i][j][v] = o0[i][j][v];
                    s1[i][j][v] = o1[i][j][v];
                }
        const int t1 = t0 + kPtmulFold < a.k ? t0 + kPtmulFold : a.k;
        for (int t = t0; t < t1; ++t) {
            uint64_t w[RM][V], y0[RN][V], y1[RN][V];
#pragma unroll
            for (int i = 0; i < RM; ++i) Lane<V>::load(X::at(x.w + i * a.w_row + t * a.w_col, off), w[i]);
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                Lane<V>::load(X::at(x.x0 + t * a.x_row + j * a.x_col, off), y0[j]);
                Lane<V>::load(X::at(x.x1 + t * a.x_row + j * a.x_col, off), y1[j]);
            }
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        s0[i][j][v] += (u128)w[i][v] * y0[j][v];
                        s1[i][j][v] += (u128)w[i][v] * y1[j][v];
                    }
        }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    o0[i][j][v] = barrett128(s0[i][j][v], x.q, x.r0, x.r1);
                    o1[i][j][v] = barrett128(s1[i][j][v], x.q, x.r0, x.r1);
                }
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            Lane<V>::store(X::at(x.o0 + i * a.o_row + j * a.o_col, off), o0[i][j]);
            Lane<V>::store(X::at(x.o1 + i * a.o_row + j * a.o_col, off), o1[i][j]);
        }
}

// the instantiation of a tile's own shape, rm <= RM rows and rn <= RN columns (both uniform over the block)
template <int V, int RM, int RN>
static __device__ __forceinline__ void ptmat_cols(const PtmatArgs& a, const PtmatTile<V>& x, uint32_t off, int rn) {
    if (rn == RN)
        ptmat_tile<V, RM, RN>(a, x, off);
    else if constexpr (RN > 1)
        ptmat_cols<V, RM, RN - 1>(a, x, off, rn);
}
template <int V, int RM, int TN>
static __device__ __forceinline__ void ptmat_rows(const PtmatArgs& a, const PtmatTile<V>& x, uint32_t off, int rm,
                                                  int rn) {
    if (rm == RM)
        ptmat_cols<V, RM, TN>(a, x, off, rn);
    else if constexpr (RM > 1)
        ptmat_rows<V, RM - 1, TN>(a, x, off, rm, rn);
}

// V: coefficients per thread; TM x TN: the tile.  Work item w = tile * npoly + polynomial, tiles row-major over
// ceil(m / TM) x ceil(n / TN).  dmod is indexed by the block's row: scalar loads.
template <int V, int TM, int TN>
__global__ MFHE_PTMAT_BOUNDS void ptmat_tensor_kernel(PtmatArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t ro = (uint64_t)r * a.ncoeff;                  // the row: uniform
    const uint32_t off = (uint32_t)c * (uint32_t)sizeof(T);      // the lane: below 2^32 bytes, the launcher checks
    const uint32_t tn = ((uint32_t)a.n + TN - 1) / TN;
    PtmatTile<V> x;
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
        const uint64_t xo = ro + j0 * a.x_col + (uint64_t)p * a.x_poly;
        const uint64_t oo = ro + i0 * a.o_row + j0 * a.o_col + (uint64_t)p * a.o_poly;
        x.w = (const T*)a.w + ro + i0 * a.w_row + (uint64_t)p * a.w_poly;
        x.x0 = (const T*)a.x0 + xo;
        x.x1 = (const T*)a.x1 + xo;
        x.b = a.bias ? (const T*)a.bias + ro + i0 * a.b_row + j0 * a.b_col + (uint64_t)p * a.b_poly : nullptr;
        x.o0 = (T*)a.o0 + oo;
        x.o1 = (T*)a.o1 + oo;
        ptmat_rows<V, TM, TN>(a, x, off, rm, rn);
    }
}

int launch_ptmat_tensor(mfhe_ctx* c, PtmatArgs a, hipStream_t st) {
    if (a.npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    if (!a.bias) a.b_row = a.b_col = a.b_poly = 0;
    const bool wide = MFHE_PTMAT_WIDE &&
                      ks_wide({&a.ncoeff, &a.w_row, &a.w_col, &a.w_poly, &a.x_row, &a.x_col, &a.x_poly, &a.b_row,
                               &a.b_col, &a.b_poly, &a.o_row, &a.o_col, &a.o_poly},
                              {a.w, a.x0, a.x1, a.bias, a.o0, a.o1});
    const uint64_t tiles = (((uint64_t)a.m + kPtmatTM - 1) / kPtmatTM) * (((uint64_t)a.n + kPtmatTN - 1) / kPtmatTN);
    a.nwork = tiles * a.npoly;
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull || a.level > 65535 || a.ncoeff > (1ull << 28) || a.nwork / tiles != a.npoly ||
        a.nwork > 0xffffffffull)
        return set_error(MFHE_EINVAL, "ptmat_tensor: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)a.level, (uint32_t)(a.nwork < 65535 ? a.nwork : 65535));
    if (wide)
        hipLaunchKernelGGL((ptmat_tensor_kernel<2, kPtmatTM, kPtmatTN>), grid, dim3(rg.block), 0, st, a,
                           (const uint64_t*)c->d_dmod);
    else
        hipLaunchKernelGGL((ptmat_tensor_kernel<1, kPtmatTM, kPtmatTN>), grid, dim3(rg.block), 0, st, a,
                           (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ptmat_tensor_kernel");
    return MFHE_OK;
}

// The operands of a product as the entry points take them.
struct PtmatOperands {
    const uint64_t* w;
    size_t w_row, w_col, w_poly;
    const uint64_t *x0, *x1;
    size_t x_row, x_col, x_poly;
    const uint64_t* bias;
    size_t b_row, b_col, b_poly;
    int m, n, k;
};

// Pointers, shape and strides of the operands (lw = level * N); in[0 .. 4) = the ranges they span (the bias' empty
// without one).  A stride of 0 repeats: W's and the bias' poly stride over the batch, the bias' row or column stride
// over the rows or columns; what is repeated spans one block.
static int ptmat_check_operands(const std::string& w, const PtmatOperands& o, size_t npoly, size_t lw, KsRange in[4]) {
    if (!o.w || !o.x0 || !o.x1) return set_error(MFHE_EINVAL, w + ": null pointer");
    if (o.m < 1 || o.n < 1) return set_error(MFHE_EINVAL, w + ": m or n < 1");
    if (o.k < 1 || o.k > kPtmulMaxTerms) return set_error(MFHE_EINVAL, w + ": k outside [1, 64]");
    if ((o.w_poly && o.w_poly < lw) || o.x_poly < lw || (o.bias && o.b_poly && o.b_poly < lw))
        return set_error(MFHE_EINVAL, w + ": poly stride smaller than level * N");
    size_t wsp = 0, xsp = 0, bsp = 0;
    if (!ctmat_span({(size_t)o.m, (size_t)o.k, o.w_row, o.w_col, o.w_poly}, o.w_poly ? npoly : (size_t)(npoly > 0), lw, &wsp))
        return set_error(MFHE_EINVAL, w + ": entries of W overlap at these strides");
    if (!ctmat_span({(size_t)o.k, (size_t)o.n, o.x_row, o.x_col, o.x_poly}, npoly, lw, &xsp))
        return set_error(MFHE_EINVAL, w + ": entries of X overlap at these strides");
    if (o.bias && !ctmat_span({o.b_row ? (size_t)o.m : 1, o.b_col ? (size_t)o.n : 1, o.b_row, o.b_col, o.b_poly},
                              o.b_poly ? npoly : (size_t)(npoly > 0), lw, &bsp))
        return set_error(MFHE_EINVAL, w + ": entries of the bias overlap at these strides");
    in[0] = {o.w, wsp};
    in[1] = {o.x0, xsp};
    in[2] = {o.x1, xsp};
    in[3] = {o.bias, bsp};
    return MFHE_OK;
}

static PtmatArgs ptmat_args(const PtmatOperands& o, uint64_t* o0, uint64_t* o1, const CtmatMatrix& out, size_t npoly,
                            int level, size_t N, int flags) {
    PtmatArgs a{};
    a.w = o.w; a.x0 = o.x0; a.x1 = o.x1; a.bias = o.bias;
    a.o0 = o0; a.o1 = o1;
    a.w_row = o.w_row; a.w_col = o.w_col; a.w_poly = o.w_poly;
    a.x_row = o.x_row; a.x_col = o.x_col; a.x_poly = o.x_poly;
    a.b_row = o.b_row; a.b_col = o.b_col; a.b_poly = o.b_poly;
    a.o_row = out.row; a.o_col = out.col; a.o_poly = out.poly;
    a.ncoeff = N; a.npoly = npoly; a.m = o.m; a.n = o.n; a.k = o.k; a.level = level;
    a.add = (flags & MFHE_PTMUL_ADD) != 0;
    return a;
}

// the flags of the driver: unknown ones, and MFHE_PTMUL_RESCALE at level 1
static int ptmat_check_flags(const char* what, int flags, int level) {
    const std::string w(what);
    if (flags & ~(MFHE_PTMUL_RESCALE | MFHE_PTMUL_ADD)) return set_error(MFHE_EINVAL, w + ": unknown flag");
    if ((flags & MFHE_PTMUL_RESCALE) && level == 1)
        return set_error(MFHE_EINVAL, w + ": MFHE_PTMUL_RESCALE at level 1 leaves no limb");
    return MFHE_OK;
}

// Everything the driver needs before its first launch, the same from mfhe_ptmat_reserve and from the call itself.
// The product needs nothing; the rescale its table (limb level - 1 -> [0, level - 1)) and the scratch of one ModDown
// of both components, 2 batch level N words of the context workspace.  No key geometry enters: ctmul_rescale reads
// the level of its KsGeom alone.
static int ptmat_prepare(mfhe_ctx* c, size_t batch, int level, int flags, KsTables& t) {
    if (!(flags & MFHE_PTMUL_RESCALE)) return MFHE_OK;
    RC(bconv_table(c, level - 1, 1, 0, level - 1, &t.rescale));
    return grow_ws(c, 2 * batch * (size_t)level * c->N * 8);
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ptmul_sum(mfhe_ctx* c, const uint64_t* d_x0, const uint64_t* d_x1, size_t src_stride,
                              size_t x_poly_stride, int nsrc, const uint64_t* d_pt, size_t pt_stride,
                              size_t pt_poly_stride, int npt, const int* term_x, const int* term_pt, int nterms,
                              int addend_pt, uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride, size_t npoly,
                              int level, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_x0 || !d_x1 || !d_pt || !d_out0 || !d_out1 || !term_x || !term_pt)
        return set_error(MFHE_EINVAL, "ptmul_sum: null pointer");
    if (nterms < 1 || nterms > kPtmulMaxTerms) return set_error(MFHE_EINVAL, "ptmul_sum: nterms outside [1, 64]");
    if (nsrc < 1 || npt < 1) return set_error(MFHE_EINVAL, "ptmul_sum: nsrc or npt < 1");
    for (int t = 0; t < nterms; ++t)
        if (term_x[t] < 0 || term_x[t] >= nsrc || term_pt[t] < 0 || term_pt[t] >= npt)
            return set_error(MFHE_EINVAL, "ptmul_sum: a term index is out of range");
    if (addend_pt < -1 || addend_pt >= npt) return set_error(MFHE_EINVAL, "ptmul_sum: addend_pt outside [-1, npt)");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ptmul_sum: level outside the context");
    const size_t N = c->N, lw = (size_t)level * N;
    if (x_poly_stride < lw || out_poly_stride < lw || (pt_poly_stride && pt_poly_stride < lw))
        return set_error(MFHE_EINVAL, "ptmul_sum: poly stride smaller than level * N");
    const size_t xsp = ks_span(npoly, x_poly_stride, lw);
    const size_t psp = ks_span(pt_poly_stride ? npoly : (size_t)(npoly > 0), pt_poly_stride, lw);
    if (src_stride < xsp) return set_error(MFHE_EINVAL, "ptmul_sum: source stride smaller than the polynomials of a source");
    if (pt_stride < psp)
        return set_error(MFHE_EINVAL, "ptmul_sum: plaintext stride smaller than the polynomials of a plaintext");
    const size_t ssp = ks_span(nsrc, src_stride, xsp), osp = ks_span(npoly, out_poly_stride, lw);
    RC(ks_check_overlap("ptmul_sum", {{d_x0, ssp}, {d_x1, ssp}, {d_pt, ks_span(npt, pt_stride, psp)}},
                        {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    PtmulArgs a{};
    a.x0 = d_x0; a.x1 = d_x1; a.pt = d_pt; a.o0 = d_out0; a.o1 = d_out1;
    a.src_stride = src_stride; a.x_poly = x_poly_stride; a.pt_stride = pt_stride; a.pt_poly = pt_poly_stride;
    a.o_poly = out_poly_stride;
    a.ncoeff = N; a.npoly = npoly; a.nterms = nterms; a.level = level; a.addend_pt = addend_pt;
    for (int t = 0; t < nterms; ++t) {
        a.term_x[t] = term_x[t];
        a.term_pt[t] = term_pt[t];
    }
    return launch_ptmul_sum(c, a, (hipStream_t)s);
}

extern "C" int mfhe_ptmat_tile(int* tm, int* tn) {
    if (!tm || !tn) return set_error(MFHE_EINVAL, "ptmat_tile: null pointer");
    *tm = kPtmatTM;
    *tn = kPtmatTN;
    return MFHE_OK;
}

extern "C" int mfhe_ptmat_tensor(mfhe_ctx* c, const uint64_t* d_w, size_t w_row_stride, size_t w_col_stride,
                                 size_t w_poly_stride, const uint64_t* d_x0, const uint64_t* d_x1, size_t x_row_stride,
                                 size_t x_col_stride, size_t x_poly_stride, int m, int n, int k, const uint64_t* d_bias,
                                 size_t bias_row_stride, size_t bias_col_stride, size_t bias_poly_stride,
                                 uint64_t* d_out0, uint64_t* d_out1, size_t out_row_stride, size_t out_col_stride,
                                 size_t out_poly_stride, size_t npoly, int level, int flags, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_out0 || !d_out1) return set_error(MFHE_EINVAL, "ptmat_tensor: null pointer");
    if (flags & ~MFHE_PTMUL_ADD) return set_error(MFHE_EINVAL, "ptmat_tensor: unknown flag");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ptmat_tensor: level outside the context");
    const size_t N = c->N, lw = (size_t)level * N;
    const PtmatOperands o{d_w, w_row_stride, w_col_stride, w_poly_stride, d_x0, d_x1, x_row_stride, x_col_stride,
                          x_poly_stride, d_bias, bias_row_stride, bias_col_stride, bias_poly_stride, m, n, k};
    KsRange in[4];
    RC(ptmat_check_operands("ptmat_tensor", o, npoly, lw, in));
    if (out_poly_stride < lw) return set_error(MFHE_EINVAL, "ptmat_tensor: output poly stride smaller than level * N");
    const CtmatMatrix out{(size_t)m, (size_t)n, out_row_stride, out_col_stride, out_poly_stride};
    size_t osp = 0;
    if (!ctmat_span(out, npoly, lw, &osp))
        return set_error(MFHE_EINVAL, "ptmat_tensor: entries of the outputs overlap at these strides");
    const KsRange outs[2] = {{d_out0, osp}, {d_out1, osp}};
    RC(ks_check_overlap("ptmat_tensor", in, 4, outs, 2));
    if (npoly == 0) return MFHE_OK;
    return launch_ptmat_tensor(c, ptmat_args(o, d_out0, d_out1, out, npoly, level, N, flags), (hipStream_t)s);
}

extern "C" int mfhe_ptmat_reserve(mfhe_ctx* c, int m, int n, size_t npoly, int level, int flags) {
    RC(ks_check_ctx(c));
    if (m < 1 || n < 1) return set_error(MFHE_EINVAL, "ptmat_reserve: m or n < 1");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ptmat_reserve: level outside the context");
    RC(ptmat_check_flags("ptmat_reserve", flags, level));
    size_t batch = 0;
    if (!ctmat_batch(m, n, npoly, &batch)) return set_error(MFHE_EINVAL, "ptmat_reserve: m n npoly overflows");
    KsTables t;
    return ptmat_prepare(c, batch, level, flags, t);
}

extern "C" int mfhe_ptmat_apply(mfhe_ctx* c, const uint64_t* d_w, size_t w_row_stride, size_t w_col_stride,
                                size_t w_poly_stride, const uint64_t* d_x0, const uint64_t* d_x1, size_t x_row_stride,
                                size_t x_col_stride, size_t x_poly_stride, int m, int n, int k, const uint64_t* d_bias,
                                size_t bias_row_stride, size_t bias_col_stride, size_t bias_poly_stride,
                                uint64_t* d_out0, uint64_t* d_out1, size_t out_poly_stride, size_t npoly, int level,
                                int flags, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_out0 || !d_out1) return set_error(MFHE_EINVAL, "ptmat_apply: null pointer");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "ptmat_apply: level outside the context");
    RC(ptmat_check_flags("ptmat_apply", flags, level));
    const size_t N = c->N, lw = (size_t)level * N;
    const PtmatOperands o{d_w, w_row_stride, w_col_stride, w_poly_stride, d_x0, d_x1, x_row_stride, x_col_stride,
                          x_poly_stride, d_bias, bias_row_stride, bias_col_stride, bias_poly_stride, m, n, k};
    KsRange in[4];
    RC(ptmat_check_operands("ptmat_apply", o, npoly, lw, in));
    if (out_poly_stride < lw) return set_error(MFHE_EINVAL, "ptmat_apply: output poly stride smaller than level * N");
    size_t batch = 0;
    if (!ctmat_batch(m, n, npoly, &batch)) return set_error(MFHE_EINVAL, "ptmat_apply: m n npoly overflows");
    const size_t osp = ks_span(batch, out_poly_stride, lw);
    const KsRange outs[2] = {{d_out0, osp}, {d_out1, osp}};
    RC(ks_check_overlap("ptmat_apply", in, 4, outs, 2));
    if (npoly == 0) return MFHE_OK;
    // the table and the workspace before the first launch (nothing to do after mfhe_ptmat_reserve)
    KsTables t;
    RC(ptmat_prepare(c, batch, level, flags, t));
    hipStream_t st = (hipStream_t)s;
    // entry (i, j) of the outputs is polynomials (i n + j) npoly .. of the batch
    const CtmatMatrix out{(size_t)m, (size_t)n, (size_t)n * npoly * out_poly_stride, npoly * out_poly_stride,
                          out_poly_stride};
    RC(launch_ptmat_tensor(c, ptmat_args(o, d_out0, d_out1, out, npoly, level, N, flags), st));
    if (!(flags & MFHE_PTMUL_RESCALE)) return MFHE_OK;
    return ctmul_rescale(c, d_out0, d_out1, out_poly_stride, batch, KsGeom{level, level, level, 0}, t, st);
}

// ptmul.hpp -- plaintext x ciphertext products on the key switch's layout (ptmul.hip): the kernel arguments and the
// launchers of the plaintext-weighted sum and of the tiled product of a plaintext matrix with a ciphertext matrix, and
// the bound behind the fold of their sums.
#pragma once
#include "ctmat.hpp"
#include "mod128.hpp"

namespace mfhe {

// most terms of one sum: the index arrays travel in the kernel arguments
constexpr int kPtmulMaxTerms = 64;
// Terms between two reductions of a running sum.  Every sum takes one product per term (ct_term's d1 takes two, hence
// kCtmulFold = 8).  Residues are canonical and q < 2^62, so a product is at most (2^62 - 2)^2 = 2^124 - 2^64 + 4 and 16
// of them at most 2^128 - 2^68 + 64.  Beside them a sum carries either the residue of the terms before, or at its start
// the bias (the addend) and with MFHE_PTMUL_ADD the output's present content: at most two residues, below 2^63.
constexpr int kPtmulFold = 16;
constexpr u128 kPtmulMaxProduct = ((u128)1 << 124) - ((u128)1 << 64) + 4;   // (2^62 - 2)^2
constexpr u128 kPtmulMaxCarry = (u128)1 << 63;                               // two residues below 2^62
static_assert(kPtmulMaxProduct <= (~(u128)0 - kPtmulMaxCarry) / kPtmulFold, "a fold's products and its carry fit a u128");
static_assert(kPtmulMaxProduct > (~(u128)0 - kPtmulMaxCarry) / (kPtmulFold + 1), "kPtmulFold is the longest such fold");

// Kernel arguments of the plaintext-weighted sum.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2 the
// 16-byte form).  x0, x1 [nsrc][npoly][>= level rows][ncoeff] with a source stride and a poly stride, pt
// [npt][npoly or 1][>= level rows][ncoeff] with a pt stride and a poly stride (0: one plaintext for the whole batch),
// o0, o1 [npoly][level][ncoeff] with one poly stride.
struct PtmulArgs {
    const void *x0, *x1, *pt;
    void *o0, *o1;
    uint64_t src_stride, x_poly, pt_stride, pt_poly, o_poly;
    uint64_t ncoeff;   // elements per row
    uint64_t npoly;
    int nterms, level, addend_pt;   // addend_pt < 0: no addend
    int term_x[kPtmulMaxTerms], term_pt[kPtmulMaxTerms];   // source and plaintext of term t, by value: nothing is copied
};

// One launch: o_c[p][r] = sum_t pt[term_pt[t]][p'][r] x_c[term_x[t]][p][r] + [c == 0, addend_pt >= 0] pt[addend_pt][p'][r]
// mod q_r on rows r < level (limb r is row r), p' = p or 0.  Strides and ncoeff given in words; the 16-byte form is
// chosen here when ncoeff and every stride are even and the five buffers 16-byte aligned.  Arguments already checked.
int launch_ptmul_sum(mfhe_ctx* c, PtmulArgs a, hipStream_t st);

// Kernel arguments of the tiled product Y = W X + B, W m x k plaintexts and X k x n ciphertexts of npoly polynomials
// per component.  Strides and ncoeff in units of V words.  Entry (i, t) of W starts at i w_row + t w_col, its
// polynomial p a further p w_poly (0: shared); entry (t, j) of X at t x_row + j x_col in x0 and x1 with x_poly; entry
// (i, j) of the bias (null: none) at i b_row + j b_col with b_poly, any of the three 0 to broadcast; entry (i, j) of o0
// and o1 at i o_row + j o_col with o_poly.
struct PtmatArgs {
    const void *w, *x0, *x1, *bias;
    void *o0, *o1;
    uint64_t w_row, w_col, w_poly, x_row, x_col, x_poly, b_row, b_col, b_poly, o_row, o_col, o_poly;
    uint64_t ncoeff;   // elements per row
    uint64_t npoly;
    uint64_t nwork;    // tiles x polynomials, set by the launcher
    int m, n, k, level;
    int add;           // the outputs' present contents are carried into the sums
};

// One launch: o0[i][j] = sum_t w[i][t] x0[t][j] + bias[i][j], o1[i][j] = sum_t w[i][t] x1[t][j] mod q_r on rows
// r < level, each added to what the output holds when a.add.  Strides and ncoeff given in words; the 16-byte form is
// chosen here when ncoeff and every stride are even and every buffer 16-byte aligned.  Arguments already checked.
int launch_ptmat_tensor(mfhe_ctx* c, PtmatArgs a, hipStream_t st);

}  // namespace mfhe

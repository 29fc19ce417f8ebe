// ctmat.hpp -- products of matrices of ciphertexts on the key switch's layout (ctmat.hip): the kernel arguments and
// the launcher of the tiled tensor sum.
#pragma once
#include "ctmul.hpp"

namespace mfhe {

// Kernel arguments of the tiled tensor sum C = A B, A m x k and B k x n ciphertexts of npoly polynomials per
// component.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2 the 16-byte form).  Entry (i, t) of A starts
// at i a_row + t a_col in a0 and a1, its polynomial p a_poly further; entry (t, j) of B at t b_row + j b_col with
// b_poly; entry (i, j) of d0 and d1 at i d01_row + j d01_col with d01_poly, of d2 at its own three strides.
struct CtmatArgs {
    const void *a0, *a1, *b0, *b1;
    void *d0, *d1, *d2;
    uint64_t a_row, a_col, a_poly, b_row, b_col, b_poly;
    uint64_t d01_row, d01_col, d01_poly, d2_row, d2_col, d2_poly;
    uint64_t ncoeff;   // elements per row
    uint64_t npoly;
    uint64_t nwork;    // tiles x polynomials, set by the launcher
    int m, n, k, level;
};

// One launch: d0[i][j] = sum_t a0[i][t] b0[t][j], d1[i][j] = sum_t (a0[i][t] b1[t][j] + a1[i][t] b0[t][j]),
// d2[i][j] = sum_t a1[i][t] b1[t][j] mod q_r on rows r < level.  Strides and ncoeff given in words; the 16-byte form is
// chosen here when ncoeff and every stride are even and every buffer 16-byte aligned.  Arguments already checked.
int launch_ctmat_tensor(mfhe_ctx* c, CtmatArgs a, hipStream_t st);

// ---- shared with ptmul.hip ----
// One matrix of entries as an entry point takes it.
struct CtmatMatrix {
    size_t rows, cols, row, col, poly;
};

// Words spanned by the matrix when no two of its entries overlap, each entry npoly polynomials of lw words: the
// smaller of the two strides holds an entry and the larger the line of entries at the smaller (ks_span both times),
// whichever of the two is the row stride; a stride that is never stepped (one row, one column) is free.  False when
// entries overlap.
inline bool ctmat_span(const CtmatMatrix& x, size_t npoly, size_t lw, size_t* span) {
    const size_t e = ks_span(npoly, x.poly, lw);
    const size_t cols_in = ks_span(x.cols, x.col, e), rows_in = ks_span(x.rows, x.row, e);
    if ((x.cols == 1 || x.col >= e) && (x.rows == 1 || x.row >= cols_in)) {
        *span = ks_span(x.rows, x.row, cols_in);
        return true;
    }
    if ((x.rows == 1 || x.row >= e) && (x.cols == 1 || x.col >= rows_in)) {
        *span = ks_span(x.cols, x.col, rows_in);
        return true;
    }
    return false;
}

// m n npoly, the polynomials of the driver's one batch; false when it does not fit a size_t
inline bool ctmat_batch(int m, int n, size_t npoly, size_t* batch) {
    const size_t mn = (size_t)m * (size_t)n;
    *batch = mn * npoly;
    return npoly == 0 || *batch / npoly == mn;
}

}  // namespace mfhe

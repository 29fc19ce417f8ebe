// slot.hpp -- CKKS slot encoding and decoding (slot.hip): the geometry of the batched FP64 embedding FFT, as plain
// integer code with no HIP dependency, and the kernel arguments.
//
// n = N / 2 slots, zeta = e^(i pi / N), g_j = 5^j mod 2N, t_j = (g_j - 1) / 4 (a permutation of [0, n)), u_k = m_k +
// i m_(k+n), w = e^(2 pi i / n):  m(zeta^(g_j)) = sum_k (u_k zeta^k) w^(k t_j).  Decode = twist, n-point DFT, gather
// by t_j; encode = scatter by t_j, the DFT with w^-1, times zeta^-k / n, real and imaginary parts to the two halves.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mfhe {

constexpr int kSlotThreads = 512;      // one workgroup: eight waves
constexpr int kSlotTileLog = 12;       // a workgroup's LDS tile: 2^12 double2 = 64 KiB (two workgroups per CU)
constexpr int kSlotWholeMaxLog = 12;   // n <= 2^12: the whole transform in one workgroup; above: n = n1 n2, two launches

// The launches of one transform of n = 2^ln points.  whole: one launch, `lc_whole` = log2 of the polynomials a
// workgroup holds.  Else pass A runs n1 / 2^lcA tiles per polynomial of 2^lcA columns k1 x n2 points, pass B n2 / 2^lcB
// tiles of 2^lcB rows t2 x n1 points.
struct SlotGeom {
    int ln;        // log2 n
    bool whole;
    int l1, l2;    // log2 n1, log2 n2 (two-pass)
    int lcA, lcB;  // log2 of the columns of a tile in pass A and B
    int lcW;       // whole: log2 of the polynomials per workgroup
};

inline SlotGeom slot_geom(int log_n, size_t npoly) {
    SlotGeom g{};
    g.ln = log_n - 1;
    g.whole = g.ln <= kSlotWholeMaxLog;
    if (g.whole) {
        // as many polynomials per workgroup as keep about two workgroups per CU busy; the bits of a transform do not
        // depend on its neighbours in the tile
        int lc = kSlotTileLog - g.ln;
        while (lc > 0 && ((npoly + ((size_t)1 << lc) - 1) >> lc) < 512) --lc;
        g.lcW = lc;
        return g;
    }
    g.l1 = g.ln / 2;
    g.l2 = g.ln - g.l1;
    g.lcA = kSlotTileLog - g.l2;
    g.lcB = kSlotTileLog - g.l1;
    return g;
}

// words of the context workspace a call needs: the two-pass intermediate [npoly][n] double2 and the dense blocks the
// NTTs run on (encode: level + nspecial rows; decode: d rows)
inline size_t slot_ws_words(int log_n, size_t npoly, size_t dense_rows) {
    const size_t N = (size_t)1 << log_n;
    const SlotGeom g = slot_geom(log_n, npoly);
    return npoly * N * ((g.whole ? 0 : 1) + dense_rows);
}

// jinv[t] = j with (5^j mod 2N - 1) / 4 == t, for t < n = N / 2
inline void slot_jinv_table(int log_n, uint32_t* jinv) {
    const uint64_t N = (uint64_t)1 << log_n, n = N / 2;
    uint64_t g = 1;
    for (uint64_t j = 0; j < n; ++j) {
        jinv[(g - 1) >> 2] = (uint32_t)j;
        g = (g * 5) & (2 * N - 1);
    }
}

#if defined(__HIPCC__)
}  // namespace mfhe
#include <hip/hip_runtime.h>
namespace mfhe {
// Kernel arguments.  Residue rows r < level of polynomial p at res0 + p stride0 + r N, rows r >= level at res1 + p
// stride1 + (r - level) N (one block in the caller's layout, or the two dense blocks the NTTs run on).
struct SlotArgs {
    const double* slots_in;
    double* slots_out;
    uint64_t slot_stride;    // doubles
    const uint64_t* res_in;  // decode
    uint64_t* res0;          // encode
    uint64_t* res1;
    uint64_t stride0, stride1;   // words
    double2* ws;             // [npoly][n], two-pass
    const uint32_t* jinv;    // [n]
    const uint64_t* dmod;    // [L][3]
    double mul;              // encode: scale / n; decode: 1 / scale
    uint64_t npoly;
    uint64_t q0, q1, q0inv1; // decode: q_0, q_1, q_0^-1 mod q_1
    int logN;
    int lm, lc;              // log2 of this launch's transform length and of its tile's columns
    int l1;                  // log2 n1 (two-pass)
    int level, special_start, nspecial;   // encode's rows
    int d;                   // decode's limbs: 1 or 2
    int real;                // MFHE_SLOT_REAL
};
#endif

}  // namespace mfhe

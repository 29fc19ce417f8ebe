// rlwe.hpp -- kernel arguments and workspace sizes of the RLWE client side (rlwe.hip; include/mfhe.h mfhe_rlwe_*).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mfhe {

// the caller's 256-bit seed, by value in the kernel arguments (scalar registers)
struct RlweSeed {
    uint32_t w[8];
};

// The sampler of small polynomials: one thread owns eight neighbouring coefficients (one ChaCha block, or eight int32
// of the caller's) of one polynomial and writes their residues on every row.  nsets > 1: polynomial pp = set npoly + p
// draws from stream[set] with id first_id + p (the public-key encryption's u, e0, e1 in one launch); its block is pp
// strides in, so the sets are contiguous.  Rows r < level of polynomial pp at res0 + pp stride0 + r N, rows r >= level
// at res1 + pp stride1 + (r - level) N (one block in the caller's layout, or the two dense blocks the NTTs run on).
struct RlweSmallArgs {
    RlweSeed seed;
    uint64_t first_id;
    const int32_t* coeffs;   // lift: [npoly][N] int32, coeff_stride int32 apart
    uint64_t coeff_stride;
    uint64_t* res0;
    uint64_t* res1;
    uint64_t stride0, stride1;   // words
    const uint64_t* dmod;        // [L][3]
    uint64_t npoly;
    int nsets, stream0, stream1, stream2;
    int logN, level, special_start, nspecial;
};

// what rlwe_mask_kernel computes beside a
enum {
    kRlweMaskOnly = 0,   // out1 = a
    kRlweEncZero = 1,    // out0 = e - a s
    kRlweEncMsg = 2,     // out0 = m + e - a s
    kRlweKeySwitch = 3,  // out0 = e - a s + F s_from, s_from from memory
    kRlweKeyRelin = 4,   // s_from = s s
    kRlweKeyGalois = 5,  // s_from[i] = s[pi_g(i)]
};

// One thread owns one ChaCha block: four neighbouring mask coefficients of one row (grid y) of a run of polynomials
// (grid z).  out1[p][r] = a, out0[p][r] = e + x - a s; e from the dense blocks (rows < level at e0 + p e_stride0 + r N,
// special rows at e1 + p e_stride1 + (r - level) N).  For a key, p is the digit and F = pmod[r] on its rows.
struct RlweMaskArgs {
    RlweSeed seed;
    uint64_t first_id;
    uint64_t* out0;
    uint64_t* out1;
    uint64_t out_stride;
    const uint64_t* e0;
    const uint64_t* e1;
    uint64_t e_stride0, e_stride1;
    const uint64_t* s;     // [level + K][N]
    const uint64_t* add;   // m [npoly][level + K][N] at add_stride, or s_from [level + K][N]
    uint64_t add_stride;
    const uint64_t* pmod;  // [level] P mod q_r
    const uint64_t* dmod;
    uint64_t npoly, prun;
    int kind, alpha;
    uint32_t galois_elt;
    int logN, level, special_start, nspecial;
};

// The row kernels of public-key encryption and decryption: one thread owns V neighbouring coefficients of one row and
// walks a run of polynomials.  Strides and ncoeff in units of V words.
//   pk      : c0 = pk0 u + e0 + m, c1 = pk1 u + e1; u, e0, e1 dense [npoly][level][N] blocks, set_stride apart
//   decrypt : out = c0 + c1 s
struct RlwePkArgs {
    const void *pk0, *pk1, *ws, *m;
    void *c0, *c1;
    uint64_t set_stride, dense_stride, m_stride, out_stride;
    uint64_t ncoeff, npoly, prun;
    const uint64_t* dmod;
};
struct RlweDecArgs {
    const void *c0, *c1, *s;
    void* out;
    uint64_t in_stride, out_stride;
    uint64_t ncoeff, npoly, prun;
    const uint64_t* dmod;
};

// words of the context workspace: the dense blocks of the small polynomials (npoly polynomials of `rows` rows; three
// sets of `level` rows for the public-key encryption)
inline size_t rlwe_ws_words(size_t npoly, size_t level, size_t nspecial, size_t N) {
    const size_t rows = level + nspecial;
    return npoly * N * (rows > 3 * level ? rows : 3 * level);
}

}  // namespace mfhe

// wcrt_gemm.hpp -- the exact modular GEMM of the W-CRT.
//
//   C[m][p] = sum_k A[m][k] B[k][p] mod q   (HE.cu:716-781, 1245-1270)
//
//  * VALU kernel: u64 operands (< 2^59), exact u128 accumulation over K = 512, one reduction per output (the
//    reference does an __int128 % per term, HE.cu:742); tiled and addressed as gemm_tile.hpp describes
//  * i8 MFMA path (M = K = 512): balanced base-256 digit planes (wcrt_digitize.hpp) and exact i32 accumulation
//    (wcrt_mfma.hpp), dense or factored over 771 = 3 x 257
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhe {

struct ModGemmArgs {
    const uint64_t* A;     // [L][M][K] row-major, limb stride aL
    const uint64_t* B;     // limb l at B + l*bL
    uint64_t* C;           // limb l at C + l*cL
    uint64_t* C2 = nullptr;   // factored forward only: a second copy of C, same layout (he.hip: the encrypt's shared a
                              // written into both ciphertexts by the GEMM instead of by the ring kernel)
    uint64_t aL, bL, cL;
    uint64_t sbK, sbY, scM, scY;
    int M, K, log_n;
    uint32_t P;
    const uint64_t* qmu;   // [L][2] (q, floor(2^64/q))
    const uint64_t* r64;   // [L] 2^64 mod q
    // i8 MFMA path (M = K = 512): A pre-split into D balanced base-256 digit planes [L][D][M][K] (limb
    // stride adL bytes), rtab [L][2D-1][2] = (256^s mod q, Shoup), Bdig workspace >= L*D*Ppad*K bytes.
    // Adig == nullptr selects the VALU u128 kernel.
    const int8_t* Adig = nullptr;
    uint64_t adL = 0;
    int D = 0;                   // digit-plane stride (max over limbs)
    const uint64_t* rtab = nullptr;
    int8_t* Bdig = nullptr;
    const int* limbD = nullptr;  // host: digits limb l needs (<= D); null = D for every limb
    const double* epi = nullptr; // [L][8] FP64 epilogue (q, 1/q, centred 2^32k mod q); null = integer epilogue
    bool lds_stage = true;       // LDS-staged MFMA kernel (false: fragments straight from global memory)
    int pipe = 0;                // LDS-staged K pipeline (MFHE_OPT_WCRT_PIPE): 0 auto (factored: ring, dense: two
                                 // 64-k stages), 1 two 64-k stages, 2 4-slot 32-k ring, 3 ring + one-ahead A reads
    // factored forward W-CRT (wcrt_digitize.hpp, 771 = 3 x 257): Adig holds the [L][D][256][256] planes of
    // Z[i][k] = zeta^((i+1)(k+1)) and fold [L][16] its FP64 fold constants; null = dense GEMM
    const double* fold = nullptr;
    uint64_t* d0 = nullptr;      // set by the launcher (workspace after the digit planes)
    // factored inverse W-CRT (wcrt_digitize.hpp): Adig holds the planes of Zi[i][k] = zeta^-((i+1)(k+1)), ifold [L][16]
    // (q, 1/q, lam1[2][3], lam2[2][3]), iz [L][48] the dot-product points and chunk powers, phi the packed Phi_771
    // rows; null = dense
    const double* ifold = nullptr;
    const double* iz = nullptr;
    const uint8_t* phi = nullptr;
    double* cc = nullptr;        // set by the launcher: [L][Ppad][2] (c0, c1) per column (the d0 workspace)
    // factored forward only: where the digitize kernel takes B from (wcrt_digitize.hpp mfma_digitize_fold_kernel<D, SRC>)
    //  qsrc 0: B (residues); 1: the doubles v[r][p] at qf[r * qf_row + p * qf_step], residue round(v delta) mod q
    //  (the encode's RNS decompose fused away); 2: the encrypt's uniform sampler (he.hip uniform_kernel) evaluated
    //  in place, limb lbase + l of Ltot; 3: one centred integer per (r, p) at qf[r * qf_row + p] (the Gaussian
    //  noise, drawn once per coefficient, he.hip gaussian_compact_kernel), the same integer in every limb
    int qsrc = 0;
    const double* qf = nullptr;
    uint64_t qf_row = 0, qf_step = 0;
    double delta = 0.0;
    int lbase = 0, Ltot = 0;
    // factored inverse only (n = 64): B is not read; the digitize kernel forms it as the decrypt of the ciphertext
    // dct (wcrt_digitize.hpp mfma_digitize_ifold_dec_kernel): B[w][l][y][.] = ct.b + INTT(NTT(ct.a) * s) mod q over each
    // X row (ring_row.hpp, he.hip dec_ring_kernel), ct matrix-major, b at dct and a at dct + dtotal
    const uint64_t* dct = nullptr;
    uint64_t dtotal = 0;
    const uint64_t* dsk = nullptr;    // s [w][L][n], NTT form
    const void* dlf = nullptr;        // LimbConst [L]
    const double* dtw = nullptr;      // X-NTT tables [L][n] (ph_f)
    const double* ditw = nullptr;
    const double* dninv = nullptr;    // [L]
    double* dpart = nullptr;          // set by the launcher: [G][L][Ppad][6] column partials of a split launch
};

// bytes of B digit workspace the MFMA path needs for P columns and L limbs at D digits
size_t mod_gemm_mfma_ws(uint32_t P, int L, int D);
// host: balanced base-256 digits of x (< 2^(8D-1)), D in [1, 8]
void balanced_digits(uint64_t x, int D, int8_t* out);

int launch_mod_gemm(const ModGemmArgs& a, int L, hipStream_t s);
// the dense W-CRT forward of one small signed int8 operand shared by every limb (the encrypt's Gaussian noise, |e| <=
// 27): b8 is its one digit plane [K/32][Ppad][32]; a as launch_mod_gemm's dense MFMA arguments (wcrt_gemm.hip)
int launch_mod_gemm_smallb(const ModGemmArgs& a, const int8_t* b8, int L, hipStream_t s);
// two independent W-CRT transforms of the same shape as one launch per step (wcrt_gemm.hip; he.hip encode / decode)
int launch_mod_gemm_pair(const ModGemmArgs& a, const ModGemmArgs& b, int L, hipStream_t s);

}  // namespace mfhe

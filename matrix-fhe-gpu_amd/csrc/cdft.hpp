// cdft.hpp -- FP64 complex transforms on the W and XY axes.
//
//  * complex GEMM  C = A B  in FP64   (W-DFT HE.cu:1147-1172, w_idft batched_encoder.cu:104-123, XY DFT
//    mat_mul_kernel_complex encoder.cu:318-326): a VALU kernel in the oracle's term order and an f64 MFMA kernel,
//    tiled and addressed as gemm_tile.hpp describes
//  * the factored W-DFT / W-IDFT (771 = 3 x 257, as the W-CRT of wcrt_gemm.hpp) as a 256 x 256 GEMM or by Rader's
//    algorithm, and the n = 64 XY products as one fused launch or by 64-point FFTs
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhe {

struct CGemmArgs {
    const double2* A;      // batch b at A + b*aB, row-major [M][K] (lda = K)
    const double2* B;      // batch b at B + b*bB, element (k,p) at k*sbK + (p>>log_n)*sbY + (p&(n-1))
    double2* C;            // batch b at C + b*cB, element (m,p) at m*scM + (p>>log_n)*scY + (p&(n-1))
    uint64_t aB, bB, cB;
    uint64_t sbK, sbY, scM, scY;
    int M, K, log_n;
    uint32_t P;
    bool mfma = true;      // f64 MFMA kernel; false = VALU mul-then-add kernel (oracle term order)
    // factored W-DFT (cdft.hip, 771 = 3 x 257, as the W-CRT): 0 dense; 1 forward: A = Z [256][256], B read as
    // F_a[k + 1] folded from in[k + 1], in[k + 258] on load, columns 2 p + a', rows of C a' 256 + m, plus F_a[0];
    // 2 inverse: A = Z^-1, B = in[a' 256 + k][p] in interleaved columns 2 p + a', epilogue lam / Phi_771 as the
    // integer inverse (rows 0 and 257 and (c0, c1) come from cwdft_inv_dots_kernel).  in / out row-major [512][Pf].
    int fac = 0;
    uint32_t Pf = 0;
    const double2* cc = nullptr;    // fac 2: [Pf][2] (c0, c1)
    const double2* lam = nullptr;   // fac 2: [2: lam1, lam2][2: a'][3: t]
    const int8_t* phi = nullptr;    // fac 2: [513] Phi_771 coefficients
    double* Cim = nullptr;          // fac 2 only: planar output -- the real parts at (double*)C, the imaginary at Cim,
                                    // element (row, p) at row * scM + p in each (he.hip encode: the fold then reads
                                    // 8-byte lanes, not every other double of 16-byte pairs)
};

int launch_cgemm(const CGemmArgs& a, int batch, hipStream_t s);
// the forward factored W-DFT (cgemm_mfma_kernel<1>'s outputs, to rounding) by Rader's algorithm: in / out [512][Pf]
// complex, rb = FFT_256(zeta^(g^-k)) / 256, gp = [g^n, g^-m] (mfhe_ctx d_wdrad / d_wdgp; cdft.hip)
int launch_wdft_rader(const double2* in, double2* out, uint32_t Pf, const double2* rb, const int16_t* gp, hipStream_t s);
// the inverse (cgemm_mfma_kernel<2> + cwdft_inv_dots_kernel, to rounding): rb = the inverse table (d_wdrad + 256),
// lam / phi as CGemmArgs; out_im: planar output (real parts at (double*)out), else interleaved (cdft.hip)
int launch_wdft_rader_inv(const double2* in, double2* out, double* out_im, uint32_t Pf, const double2* rb,
                          const int16_t* gp, const double2* lam, const int8_t* phi, hipStream_t s);
// out = A M B per lane for 64 x 64 complex blocks (A, B shared; M, out [lanes][64][64]) in one launch: the two
// launch_cgemm products of wtrans.hip xy3 without the intermediate's HBM round trip, the same doubles (cdft.hip)
int launch_xy_fused(const double2* A, const double2* M, const double2* B, double2* out, int lanes, hipStream_t s);
// the same products at n = 64 by 64-point FFTs (V = ensure_xy's encoder matrix; inv: V^-1 M V^-T), equal to
// rounding; in and out must not overlap (cdft.hip xy_fft_kernel takes both as __restrict__)
int launch_xy_fft(const double2* in, double2* out, bool inv, int lanes, hipStream_t s);
// factored inverse W-DFT, first step: per column the rows r2 = 0, 255, 256 of E_a by dot products (xpow [2][256]:
// zeta^(-255 b), zeta^(-256 b)), then f_0, f_257 into out and (c0, c1) into a.cc (cdft.hip)
int launch_cwdft_inv_dots(const CGemmArgs& a, const double2* in, const double2* xpow, hipStream_t s);

}  // namespace mfhe

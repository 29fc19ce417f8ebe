// wtrans.hpp -- the W-axis and XY transform layer (wtrans.hip) as the pipelines of he.hip call it: the context
// workspace, the W-CRT request and its launcher, the complex W-DFT, the per-lane XY products and the layout change.
#pragma once
#include <hip/hip_runtime.h>

#include "mfhe_ctx.hpp"
#include "wcrt_gemm.hpp"

namespace mfhe {

inline dim3 g1(uint64_t total, uint32_t th = 256) { return dim3((uint32_t)((total + th - 1) / th)); }

int need_wcrt(const mfhe_ctx* c);

struct Geo2 {
    int L, logn;
    uint64_t n, n2, words, cnt;   // words = phi*L*n2 ; cnt = phi*n2
};
Geo2 geo(const mfhe_ctx* c);

// the context workspace (c->ws) at the size the transforms and pipelines carve their buffers from (Bump)
int ensure_ws(mfhe_ctx* c);

struct Bump {
    char* p;
    template <class T>
    T* get(size_t n) {
        T* r = (T*)p;
        p += ((n * sizeof(T) + 255) / 256) * 256;
        return r;
    }
};

// the X-row ring kernels' constants (he.hip enc_ring_kernel / dec_ring_kernel; the decrypt-fused W-CRT request)
struct RingArgs {
    const LimbConst* lf;     // [L]
    const double* tw;        // ph_f tables [L][n]
    const double* itw;
    const double* ninv;      // [L]
    const uint64_t* sk;      // [w][L][n], NTT form
    int L;
    uint64_t rows;           // 512 n L
};

// One W-CRT transform C = A B mod q over the 512 polynomials.
enum class WOut { Poly, Matrix, Vector };
// where the factored forward's digitize takes B from instead of memory (ModGemmArgs::qsrc, wcrt_gemm.hpp)
enum class WSrc { None = 0, Quant = 1, Uniform = 2, Noise = 3 };
struct WcrtReq {   // filled by designated initialisers: C++20, taken by hipcc under the build's -std=c++17
    const uint64_t* A = nullptr;   // c->d_wV or c->d_wVinv
    const uint64_t* B = nullptr;   // matrix-major [r][L][pos], poly-major with b_poly, or the vector [r][L][x]
    bool b_poly = false;
    uint64_t* C = nullptr;
    WOut out = WOut::Poly;
    bool vector = false;
    // only where quant_fused_ok(c).  Quant: the doubles qf[r n2 step + p step], quantised with the context's delta;
    // Uniform: the encrypt's sampler; Noise: one centred integer per (r, p) at qf[r n2 + p]
    WSrc src = WSrc::None;
    const double* qf = nullptr;
    uint64_t step = 1;
    const RingArgs* dec = nullptr;   // B is a ciphertext, decrypted inside the inverse's digitize (dec_fused_ok only)
    int slot = 0;                    // 1: the second set of digit planes (the side stream's, or a pair's second half)
    uint64_t* C2 = nullptr;          // factored forward only: a second copy of C
};
// the GEMM arguments of one request (wcrt_gemm launches them; or two as a pair, wcrt_gemm.hip launch_mod_gemm_pair)
int wcrt_args(mfhe_ctx* c, ModGemmArgs& a, const WcrtReq& r);
int wcrt_gemm(mfhe_ctx* c, const WcrtReq& r, hipStream_t s);
// i8 MFMA operands for A = V or V^-1 and the digit-plane workspace of `slot`, grown to a.P columns
int use_mfma(mfhe_ctx* c, ModGemmArgs& a, const uint64_t* A, int L, int slot = 0);
// the factored forward W-CRT runs: its digitize kernel (wcrt_digitize.hpp mfma_digitize_fold_kernel<D, SRC>) can take
// a WSrc (the encode's quantise + RNS split, the encrypt's samplers)
bool quant_fused_ok(const mfhe_ctx* c);

// complex W-DFT / W-IDFT over [phi][n2], A = c->d_wdV / c->d_wdVinv.  planar (only where wdft_planar_ok(c), W-IDFT):
// out as two [phi][n2] double planes, real then imaginary
bool wdft_planar_ok(const mfhe_ctx* c);
int wdft(mfhe_ctx* c, const double2* A, const double2* in, double2* out, hipStream_t s, bool planar = false);

// per-lane XY: out = A * M * B over `lanes` n x n matrices (tmp: lanes*n2 complex)
int xy3(const mfhe_ctx* c, const double2* A, const double2* in, const double2* B, double2* tmp, double2* out,
        size_t lanes, hipStream_t s);

int layout(const mfhe_ctx* c, const uint64_t* in, uint64_t* out, bool to_poly, hipStream_t s);

}  // namespace mfhe

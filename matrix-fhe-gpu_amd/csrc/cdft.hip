// cdft.hip -- see cdft.hpp.
#include "cdft.hpp"
#include "gemm_tile.hpp"
#include "mfhe_ctx.hpp"

namespace mfhe {

__global__ __launch_bounds__(NTH) void cgemm_kernel(CGemmArgs a) {
    __shared__ double2 As[TM][TK + 1];
    __shared__ double2 Bs[TK][TP];
    const int bt = blockIdx.z;
    const int m0 = blockIdx.y * TM;
    const uint32_t p0 = blockIdx.x * TP;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const double2* A = a.A + (uint64_t)bt * a.aB;
    const double2* B = a.B + (uint64_t)bt * a.bB;
    double accr[4][4], acci[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) accr[i][j] = acci[i][j] = 0.0;
    for (int k0 = 0; k0 < a.K; k0 += TK) {
#pragma unroll
        for (int e = 0; e < (TM * TK) / NTH; ++e) {
            const int idx = t + e * NTH, r = idx / TK, c = idx % TK;
            const int m = m0 + r, k = k0 + c;
            As[r][c] = (m < a.M && k < a.K) ? A[(uint64_t)m * a.K + k] : make_double2(0, 0);
        }
#pragma unroll
        for (int e = 0; e < (TK * TP) / NTH; ++e) {
            const int idx = t + e * NTH, r = idx / TP, c = idx % TP;
            const int k = k0 + r;
            const uint32_t p = p0 + c;
            Bs[r][c] = (k < a.K && p < a.P) ? B[b_off(k, p, a.sbK, a.sbY, a.log_n)] : make_double2(0, 0);
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < TK; ++k) {
            double2 av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[ty + 16 * i][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[k][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // acc += a*b, same term order as cuCmul + add (encoder.cu:323, HE.cu:1168-1169)
                    accr[i][j] += av[i].x * bv[j].x - av[i].y * bv[j].y;
                    acci[i][j] += av[i].x * bv[j].y + av[i].y * bv[j].x;
                }
        }
        __syncthreads();
    }
    double2* C = a.C + (uint64_t)bt * a.cB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty + 16 * i;
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p = p0 + tx + 16 * j;
            if (p >= a.P) continue;
            C[b_off(m, p, a.scM, a.scY, a.log_n)] = make_double2(accr[i][j], acci[i][j]);
        }
    }
}

// ---------------- FP64 MFMA complex GEMM (W-DFT, XY transforms) ----------------
//
// C = A B over complex doubles as four real products on v_mfma_f64_16x16x4_f64:
//   Cr += Ar Br + (-Ai) Bi,  Ci += Ar Bi + Ai Br.
// A workgroup computes a 64 x 64 tile of C (four 32 x 32 wave tiles of 2 x 2 MFMA blocks); each
// 16-deep K stage of A and B goes global -> registers -> LDS (split into re / im planes) one stage
// ahead of the MFMAs that read it.  Products are exact-rounded f64 FMAs, so the sum differs from the
// oracle's mul-then-add order by ~1e-16 relative per term -- the FP_TOL parity of the VALU kernel
// above, which stays selectable (MFHE_OPT_CGEMM_MFMA = 0).
// Fragment maps (f64 16x16x4): A lane l = A[l&15][k=l>>4], B lane l = B[k=l>>4][l&15],
// C/D reg j of lane l = C[(l>>4) + 4j][l&15].
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int CKT = 16;          // K per LDS stage
constexpr int CAP = CKT + 1;     // A plane row pitch (doubles): spreads a fragment's 16 rows over the banks

// omega^e, omega = e^(2 pi i / 3) (the order-3 root of the factored W-DFT)
__device__ __forceinline__ double2 omega3(int e) {
    constexpr double h = 0.86602540378443864676;   // sqrt(3) / 2
    return e == 0 ? make_double2(1.0, 0.0) : make_double2(-0.5, e == 1 ? h : -h);
}
__device__ __forceinline__ double2 cmul(double2 x, double2 y) {
    return make_double2(__fma_rn(x.x, y.x, -x.y * y.y), __fma_rn(x.x, y.y, x.y * y.x));
}
// lanes l <-> l ^ 1 (DPP quad_perm [1, 0, 3, 2])
__device__ __forceinline__ double dpp_swap1(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true),
                            __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true));
}

// one output of the factored inverse W-DFT: interleaved complex, or planar (CGemmArgs::Cim)
__device__ __forceinline__ void cstore(const CGemmArgs& a, uint64_t idx, double re, double im) {
    if (a.Cim) {
        ((double*)a.C)[idx] = re;
        a.Cim[idx] = im;
    } else {
        a.C[idx] = make_double2(re, im);
    }
}

// FAC (a.fac): 0 dense; 1 / 2 the factored forward / inverse W-DFT (cdft.hpp CGemmArgs::fac)
template <int FAC>
__global__ __launch_bounds__(NTH, 2) void cgemm_mfma_kernel(CGemmArgs a) {
    __shared__ double Ar[2][TM * CAP], Ai[2][TM * CAP];   // [row][k]
    __shared__ double Br[2][CKT * TP], Bi[2][CKT * TP];   // [k][col]
    const int bt = blockIdx.z;
    const int m0 = blockIdx.y * TM;
    const uint32_t p0 = blockIdx.x * TP;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 32, wp = (w & 1) * 32, r = lane & 15, kq = lane >> 4;
    const double2* A = a.A + (uint64_t)bt * a.aB;
    const double2* B = a.B + (uint64_t)bt * a.bB;
    double2 ra[(TM * CKT) / NTH], rb[(CKT * TP) / NTH];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < (TM * CKT) / NTH; ++e) {   // A stage 64 x 16, 16 consecutive k per row
            const int idx = t + e * NTH, m = m0 + (idx >> 4), k = k0 + (idx & 15);
            ra[e] = (m < a.M && k < a.K) ? A[(uint64_t)m * a.K + k] : make_double2(0, 0);
        }
#pragma unroll
        for (int e = 0; e < (CKT * TP) / NTH; ++e) {   // B stage 16 x 64, coalesced along p
            const int idx = t + e * NTH, k = k0 + (idx >> 6);
            const uint32_t p = p0 + (idx & 63);
            if constexpr (FAC == 0) {
                rb[e] = (k < a.K && p < a.P) ? B[b_off(k, p, a.sbK, a.sbY, a.log_n)] : make_double2(0, 0);
            } else if constexpr (FAC == 1) {
                // F_a[r2] = omega^(a t) in[r2] + omega^(a ((t + 2) mod 3)) in[r2 + 257], r2 = k + 1, t = r2 mod 3
                // interleaved columns 2 p + a': lanes 2p, 2p + 1 load the same two inputs (one fetch per pair)
                const bool live = p < a.P;
                const int ap = p & 1;
                const uint32_t pc = live ? p >> 1 : 0;
                const int r2 = k + 1, t3 = r2 % 3, r3 = r2 + 257 < 512 ? r2 + 257 : 511;
                const double2 x1 = B[(uint64_t)r2 * a.Pf + pc], x2 = B[(uint64_t)r3 * a.Pf + pc];
                const double2 f1 = cmul(omega3(((ap + 1) * t3) % 3), x1);
                const double2 f2 = r2 + 257 < 512 ? cmul(omega3(((ap + 1) * ((t3 + 2) % 3)) % 3), x2) : make_double2(0, 0);
                rb[e] = live ? make_double2(f1.x + f2.x, f1.y + f2.y) : make_double2(0, 0);
            } else {
                // y[a'][b] = in[a' 256 + k][p] in interleaved columns 2 p + a'
                const bool live = p < a.P;
                const uint32_t pc = live ? p >> 1 : 0;
                const double2 y = B[(uint64_t)((p & 1) * 256 + k) * a.Pf + pc];
                rb[e] = live ? y : make_double2(0, 0);
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int e = 0; e < (TM * CKT) / NTH; ++e) {
            const int idx = t + e * NTH, o = (idx >> 4) * CAP + (idx & 15);
            Ar[buf][o] = ra[e].x;
            Ai[buf][o] = ra[e].y;
        }
#pragma unroll
        for (int e = 0; e < (CKT * TP) / NTH; ++e) {
            const int idx = t + e * NTH;
            Br[buf][idx] = rb[e].x;
            Bi[buf][idx] = rb[e].y;
        }
    };
    v4d cr[2][2], ci[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) cr[i][j] = ci[i][j] = v4d{0, 0, 0, 0};
    const int nk = (a.K + CKT - 1) / CKT;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * CKT);
#pragma unroll
        for (int ks = 0; ks < CKT / 4; ++ks) {
            const int k = ks * 4 + kq;
            double ar[2], ai[2], nai[2], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ar[i] = Ar[buf][(wm + 16 * i + r) * CAP + k];
                ai[i] = Ai[buf][(wm + 16 * i + r) * CAP + k];
                nai[i] = -ai[i];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                br[j] = Br[buf][k * TP + wp + 16 * j + r];
                bi[j] = Bi[buf][k * TP + wp + 16 * j + r];
            }
            // first terms of all eight accumulators, then the second terms: no back-to-back dependence
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    cr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], cr[i][j], 0, 0, 0);
                    ci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], ci[i][j], 0, 0, 0);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    cr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai[i], bi[j], cr[i][j], 0, 0, 0);
                    ci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], br[j], ci[i][j], 0, 0, 0);
                }
        }
        if (kt + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }
    double2* C = a.C + (uint64_t)bt * a.cB;
    if constexpr (FAC == 1) {
        // out[a' 256 + m][p] = GEMM + F_a[0], F_a[0] = in[0] + omega^(2 a) in[257]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t c = p0 + wp + 16 * j + r;
            if (c >= a.P) continue;
            const int ap = c & 1;
            const uint32_t p = c >> 1;
            const double2 f = cmul(omega3((2 * (ap + 1)) % 3), B[257ull * a.Pf + p]), x0 = B[p];
            const double2 add = make_double2(x0.x + f.x, x0.y + f.y);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int m = m0 + wm + 16 * i + kq + 4 * g;
                    C[(uint64_t)(ap * 256 + m) * a.scM + p] = make_double2(cr[i][j][g] + add.x, ci[i][j][g] + add.y);
                }
        }
        return;
    } else if constexpr (FAC == 2) {
        // E_a'[r2] (r2 = m + 1) in lanes 2p + a'; h_r2 = sum_a lam1[a][t] E_a, h_(r2+257) = sum_a lam2[a][t] E_a
        // (t = r2 mod 3), f_j = h_j - c0 phi_j - c1 phi_(j-1): lane a' = 0 writes row r2, a' = 1 row r2 + 257
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t c = p0 + wp + 16 * j + r;
            const int ap = c & 1;
            const uint32_t p = c >> 1;
            const bool live = c < a.P;   // the same for both lanes of a pair (P even)
            const uint32_t pc = live ? p : 0;
            const double2 c0 = a.cc[2ull * pc], c1 = a.cc[2ull * pc + 1];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r2 = m0 + wm + 16 * i + kq + 4 * g + 1;
                    const int t3 = r2 % 3;
                    const double2 own = a.lam[(ap * 2 + ap) * 3 + t3], oth = a.lam[((1 - ap) * 2 + ap) * 3 + t3];
                    const double2 e = make_double2(cr[i][j][g], ci[i][j][g]);
                    const double2 po = cmul(own, e), ps = cmul(oth, e);
                    const double hx = po.x + dpp_swap1(ps.x), hy = po.y + dpp_swap1(ps.y);
                    const int jr = ap ? r2 + 257 : r2;
                    if (live && jr < 512) {
                        const double f0 = (double)a.phi[jr], f1 = (double)a.phi[jr - 1];
                        cstore(a, (uint64_t)jr * a.scM + p, hx - c0.x * f0 - c1.x * f1, hy - c0.y * f0 - c1.y * f1);
                    }
                }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t p = p0 + wp + 16 * j + r;
            if (p >= a.P) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m = m0 + wm + 16 * i + kq + 4 * g;
                if (m < a.M) C[b_off(m, p, a.scM, a.scY, a.log_n)] = make_double2(cr[i][j][g], ci[i][j][g]);
            }
        }
}

// factored inverse W-DFT, rows r2 = 0, 255, 256 of E_a by dot products.  One thread per (column p, a', 32-row
// chunk q): lane = 2 p_local + a' (16 columns per block), q = thread / 32.  S0 = sum y, S1 = sum x1^b y,
// S2 = sum x2^b y over b = 32 q + 1 .. 32 q + 32; the chunks reduce through LDS, a' by a lane exchange; then
// f_0, f_257 and (c0, c1) as in wcrt_digitize.hpp mfma_digitize_ifold_kernel (complex, no reduction mod q).
__global__ __launch_bounds__(256) void cwdft_inv_dots_kernel(CGemmArgs a, const double2* __restrict__ in,
                                                             const double2* __restrict__ xpow) {
    __shared__ double2 red[3][8][32];
    const int lane = threadIdx.x & 31, q = threadIdx.x >> 5;   // 32 threads = 16 columns x 2 a'; 8 chunks
    const uint32_t p = blockIdx.x * 16 + (lane >> 1);
    const int ap = lane & 1;
    const bool live = p < a.Pf;
    const uint32_t pc = live ? p : 0;
    double2 s0 = make_double2(0, 0), s1 = s0, s2 = s0;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
        const int k = q * 32 + i;   // b = k + 1
        const double2 y = in[(uint64_t)(ap * 256 + k) * a.Pf + pc];
        const double2 z1 = xpow[k], z2 = xpow[256 + k];
        s0.x += y.x;
        s0.y += y.y;
        s1.x = __fma_rn(z1.x, y.x, __fma_rn(-z1.y, y.y, s1.x));
        s1.y = __fma_rn(z1.x, y.y, __fma_rn(z1.y, y.x, s1.y));
        s2.x = __fma_rn(z2.x, y.x, __fma_rn(-z2.y, y.y, s2.x));
        s2.y = __fma_rn(z2.x, y.y, __fma_rn(z2.y, y.x, s2.y));
    }
    red[0][q][lane] = s0;
    red[1][q][lane] = s1;
    red[2][q][lane] = s2;
    __syncthreads();
    if (q != 0) return;
    double2 e[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        double2 acc = red[v][0][lane];
#pragma unroll
        for (int c = 1; c < 8; ++c) acc = make_double2(acc.x + red[v][c][lane].x, acc.y + red[v][c][lane].y);
        e[v] = acc;
    }
    double2 o[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) o[v] = make_double2(__shfl_xor(e[v].x, 1), __shfl_xor(e[v].y, 1));
    const double2* e1 = ap ? o : e;   // a = 1
    const double2* e2 = ap ? e : o;   // a = 2
    auto lam = [&](int kind, int aa, int t3) { return a.lam[(kind * 2 + aa) * 3 + t3]; };
    auto add2 = [](double2 x, double2 y) { return make_double2(x.x + y.x, x.y + y.y); };
    const double2 h0 = add2(cmul(lam(0, 0, 0), e1[0]), cmul(lam(0, 1, 0), e2[0]));       // r2 = 0
    const double2 h257 = add2(cmul(lam(1, 0, 0), e1[0]), cmul(lam(1, 1, 0), e2[0]));
    const double2 h512 = add2(cmul(lam(1, 0, 0), e1[1]), cmul(lam(1, 1, 0), e2[1]));     // r2 = 255, t = 0
    const double2 h513 = add2(cmul(lam(1, 0, 1), e1[2]), cmul(lam(1, 1, 1), e2[2]));     // r2 = 256, t = 1
    const double p511 = a.phi[511], p0 = a.phi[0], p256 = a.phi[256], p257 = a.phi[257];
    const double2 c1 = h513;
    const double2 c0 = make_double2(h512.x - c1.x * p511, h512.y - c1.y * p511);
    if (!live) return;
    if (ap == 0) {
        cstore(a, p, h0.x - c0.x * p0, h0.y - c0.y * p0);
        ((double2*)a.cc)[2ull * p] = c0;
        ((double2*)a.cc)[2ull * p + 1] = c1;
    } else {
        cstore(a, 257ull * a.scM + p, h257.x - c0.x * p257 - c1.x * p256, h257.y - c0.y * p257 - c1.y * p256);
    }
}

int launch_cwdft_inv_dots(const CGemmArgs& a, const double2* in, const double2* xpow, hipStream_t s) {
    hipLaunchKernelGGL(cwdft_inv_dots_kernel, dim3((a.Pf + 15) / 16), dim3(256), 0, s, a, in, xpow);
    MFHE_CHECK_LAUNCH("cwdft_inv_dots_kernel");
    return MFHE_OK;
}

// ---- the per-lane XY product out = A M B in one launch (r06, n = 64) ----
// wtrans.hip xy3 at n = 64: A and B the shared 64 x 64 encoder matrices, M one lane's 64 x 64 block; one workgroup per
// lane, eight waves of 16 x 32 outputs.  Phase 1 is cgemm_mfma_kernel<0>'s T = A M (v_mfma_f64_16x16x4_f64 blocks,
// each output accumulated in the same order, k-step by k-step: first the Ar Br / Ar Bi terms, then -Ai Bi / Ai Br),
// with all of K in LDS at once; T then goes to LDS instead of HBM and phase 2 is out = T B the same way.  So the
// doubles are those of the two launches, without T's round trip and the second launch's fill.  LDS: A / T planes
// [64][65] (the row pitch spreads a fragment's 16 rows over the banks), M / B planes [64][64]: 130.5 KiB, one
// workgroup per CU, two waves per SIMD (four waves: 61.8 us per call; eight: 51.3 us; the two launches ~54 us).
constexpr int XYN = 64, XYP = 65, XYT = 512;   // eight waves: two per SIMD at one workgroup per CU
__global__ __launch_bounds__(XYT, 1) void xy_fused_kernel(const double2* __restrict__ A, const double2* __restrict__ M,
                                                          const double2* __restrict__ Bm, double2* __restrict__ out) {
    __shared__ double Lr[XYN * XYP], Li[XYN * XYP];   // left operand: A, then T   ([row][k])
    __shared__ double Rr[XYN * XYN], Ri[XYN * XYN];   // right operand: M, then B  ([k][col])
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 16, wp = (w & 1) * 32, r = lane & 15, kq = lane >> 4;   // each wave 16 x 32
    const uint64_t lb = (uint64_t)blockIdx.x * XYN * XYN;
    auto load_left = [&](const double2* src) {
#pragma unroll 4
        for (int e = 0; e < XYN * XYN / XYT; ++e) {
            const int idx = t + e * XYT;
            const double2 v = src[idx];
            Lr[(idx >> 6) * XYP + (idx & 63)] = v.x;
            Li[(idx >> 6) * XYP + (idx & 63)] = v.y;
        }
    };
    auto load_right = [&](const double2* src) {
#pragma unroll 4
        for (int e = 0; e < XYN * XYN / XYT; ++e) {
            const int idx = t + e * XYT;
            const double2 v = src[idx];
            Rr[idx] = v.x;
            Ri[idx] = v.y;
        }
    };
    v4d cr[1][2], ci[1][2];
    auto product = [&]() {
#pragma unroll
        for (int i = 0; i < 1; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) cr[i][j] = ci[i][j] = v4d{0, 0, 0, 0};
#pragma unroll 4
        for (int ks = 0; ks < XYN / 4; ++ks) {
            const int k = ks * 4 + kq;
            double ar[1], ai[1], nai[1], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 1; ++i) {
                ar[i] = Lr[(wm + 16 * i + r) * XYP + k];
                ai[i] = Li[(wm + 16 * i + r) * XYP + k];
                nai[i] = -ai[i];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                br[j] = Rr[k * XYN + wp + 16 * j + r];
                bi[j] = Ri[k * XYN + wp + 16 * j + r];
            }
#pragma unroll
            for (int i = 0; i < 1; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    cr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], cr[i][j], 0, 0, 0);
                    ci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], ci[i][j], 0, 0, 0);
                }
#pragma unroll
            for (int i = 0; i < 1; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    cr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai[i], bi[j], cr[i][j], 0, 0, 0);
                    ci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], br[j], ci[i][j], 0, 0, 0);
                }
        }
    };
    load_left(A);
    load_right(M + lb);
    __syncthreads();
    product();   // T = A M
    __syncthreads();   // every wave is done reading A and M
#pragma unroll
    for (int i = 0; i < 1; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m = wm + 16 * i + kq + 4 * g, p = wp + 16 * j + r;
                Lr[m * XYP + p] = cr[i][j][g];
                Li[m * XYP + p] = ci[i][j][g];
            }
    load_right(Bm);
    __syncthreads();
    product();   // out = T B
    double2* o = out + lb;
#pragma unroll
    for (int i = 0; i < 1; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                o[(wm + 16 * i + kq + 4 * g) * XYN + wp + 16 * j + r] = make_double2(cr[i][j][g], ci[i][j][g]);
}

int launch_xy_fused(const double2* A, const double2* M, const double2* B, double2* out, int lanes, hipStream_t s) {
    if (!A || !M || !B || !out || lanes <= 0) return set_error(MFHE_EINVAL, "xy_fused: bad arguments");
    hipLaunchKernelGGL(xy_fused_kernel, dim3((uint32_t)lanes), dim3(XYT), 0, s, A, M, B, out);
    MFHE_CHECK_LAUNCH("xy_fused_kernel");
    return MFHE_OK;
}

// ---- the forward factored W-DFT by Rader's algorithm (r06) ----
// cgemm_mfma_kernel<1> computes, per column p and a = a' + 1, X_a[b] = F_a[0] + sum_{j=1..256} zeta^(b j) F_a[j]
// (b = 1..256, zeta = e^(2 pi i / 257); F_a folded from in[j] and in[j + 257] with omega = e^(2 pi i / 3)) as a
// 256 x 256 complex GEMM.  That is a 257-point DFT: with g = 3 (a primitive root of 257), j = g^n and b = g^-m,
// X_a[g^-m] - F_a[0] = sum_n F_a[g^n] zeta^(g^(n - m)) is the cyclic convolution of a[n] = F_a[g^n] with
// bk[k] = zeta^(g^-k), taken as IFFT_256(FFT_256(a) . FFT_256(bk)) -- 2 x 1024 butterflies per column instead of
// 65536 complex MACs, so the transform becomes bound by its 64 MB of HBM traffic.  Same outputs to rounding
// (~1e-15 relative; the GEMM's are already not the reference's own rounding, HE.cu:1147-1172).
// One workgroup: 8 columns x both a; 16 threads per column, each holding 16 points of each a's FFT: 256 = 16 x 16
// (a 16-point radix-2 FFT in registers over s, the twiddle W256^(t k1), a transpose through LDS, the 16-point FFT
// over t), the product with FFT(bk) / 256, and the inverse the same way.
__device__ __forceinline__ double2 cadd(double2 x, double2 y) { return make_double2(x.x + y.x, x.y + y.y); }
__device__ __forceinline__ double2 csub(double2 x, double2 y) { return make_double2(x.x - y.x, x.y - y.y); }
__device__ __forceinline__ double2 cconj(double2 x) { return make_double2(x.x, -x.y); }
// e^(SIGN 2 pi i k / 16), k = 0..7
template <int SIGN>
__device__ __forceinline__ double2 w16(int k) {
    constexpr double C[8] = {1.0, 0.92387953251128675613, 0.70710678118654752440, 0.38268343236508977173,
                             0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613};
    constexpr double S[8] = {0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128675613,
                             1.0, 0.92387953251128675613, 0.70710678118654752440, 0.38268343236508977173};
    return make_double2(C[k], SIGN * S[k]);
}
// in-register 16-point DFT, natural order in and out: X[k] = sum_s x[s] e^(SIGN 2 pi i s k / 16)
template <int SIGN>
__device__ __forceinline__ void fft16(double2 (&x)[16]) {
    auto sw = [&](int i, int j) {
        const double2 t = x[i];
        x[i] = x[j];
        x[j] = t;
    };
    sw(1, 8); sw(2, 4); sw(3, 12); sw(5, 10); sw(7, 14); sw(11, 13);   // 4-bit reversal
#pragma unroll
    for (int len = 2; len <= 16; len <<= 1)
#pragma unroll
        for (int i = 0; i < 16; i += len)
#pragma unroll
            for (int j = 0; j < len / 2; ++j) {
                const int k = j * (16 / len);
                const double2 u = x[i + j], v = k == 0 ? x[i + j + len / 2] : cmul(x[i + j + len / 2], w16<SIGN>(k));
                x[i + j] = cadd(u, v);
                x[i + j + len / 2] = csub(u, v);
            }
}
constexpr int RDC = 8;   // columns per workgroup
__global__ __launch_bounds__(RDC * 16) void wdft_rader_kernel(const double2* __restrict__ in, double2* __restrict__ out,
                                                              uint32_t Pf, const double2* __restrict__ rb,
                                                              const int16_t* __restrict__ gp) {
    __shared__ double2 tw[256];                  // e^(-2 pi i k / 256)
    __shared__ double2 fb[256];                  // FFT(bk) / 256
    __shared__ int16_t sg[512];                  // g^n, g^-m
    __shared__ double2 xs[RDC][2][16][17];       // transposes: [column][a'][row][col], padded
    const int t = threadIdx.x & 15, pc = threadIdx.x >> 4;
    for (int i = threadIdx.x; i < 256; i += RDC * 16) {
        double sn, cs;
        sincospi(-(double)i / 128.0, &sn, &cs);
        tw[i] = make_double2(cs, sn);
        fb[i] = rb[i];
        sg[i] = gp[i];
        sg[256 + i] = gp[256 + i];
    }
    __syncthreads();
    const uint32_t p = blockIdx.x * RDC + pc;
    const bool live = p < Pf;
    const uint32_t pr = live ? p : 0;
    // F_a[j] for a' = 0, 1: omega^(a (j mod 3)) in[j] + omega^(a ((j + 2) mod 3)) in[j + 257] (second term if j <= 254)
    auto fold = [&](int j, double2& f0, double2& f1) {
        const double2 x1 = in[(uint64_t)j * Pf + pr];
        const double2 x2 = j <= 254 ? in[(uint64_t)(j + 257) * Pf + pr] : make_double2(0.0, 0.0);
        const int t3 = j % 3, t3b = (t3 + 2) % 3;
        f0 = cadd(cmul(omega3(t3), x1), cmul(omega3(t3b), x2));
        f1 = cadd(cmul(omega3((2 * t3) % 3), x1), cmul(omega3((2 * t3b) % 3), x2));
    };
    double2 x[2][16];
#pragma unroll
    for (int s = 0; s < 16; ++s) fold(sg[t + 16 * s], x[0][s], x[1][s]);
    double2 F0[2];
    fold(0, F0[0], F0[1]);
    // forward FFT_256 of a[n] = F[g^n], n = t + 16 s: over s, twiddle W256^(t k1), transpose, over t
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
        fft16<-1>(x[ap]);
#pragma unroll
        for (int k1 = 1; k1 < 16; ++k1) x[ap][k1] = cmul(x[ap][k1], tw[(t * k1) & 255]);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) xs[pc][ap][k1][t] = x[ap][k1];
    }
    __syncthreads();
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
#pragma unroll
        for (int tt = 0; tt < 16; ++tt) x[ap][tt] = xs[pc][ap][t][tt];   // this thread is now k1 = t
        fft16<-1>(x[ap]);                                                 // A[t + 16 k2] in x[ap][k2]
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) x[ap][k2] = cmul(x[ap][k2], fb[t + 16 * k2]);
        // inverse: over k2 (this thread k1 = t) gives C[t][u]; twiddle e^(+2 pi i u t / 256); transpose; over k1
        fft16<1>(x[ap]);
#pragma unroll
        for (int u = 1; u < 16; ++u) x[ap][u] = cmul(x[ap][u], cconj(tw[(u * t) & 255]));
    }
    __syncthreads();   // every thread has read its transposed row
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int u = 0; u < 16; ++u) xs[pc][ap][u][t] = x[ap][u];
    __syncthreads();
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) x[ap][k1] = xs[pc][ap][t][k1];   // this thread is now u = t
        fft16<1>(x[ap]);                                                  // y[t + 16 v] in x[ap][v]
        if (live) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int b = sg[256 + t + 16 * v];   // output b = g^-m, m = t + 16 v
                out[(uint64_t)(ap * 256 + b - 1) * Pf + p] = cadd(F0[ap], x[ap][v]);
            }
        }
    }
}

// ---- the inverse factored W-DFT by Rader's algorithm (r06) ----
// cgemm_mfma_kernel<2> + cwdft_inv_dots_kernel: E_a'[r2] = sum_{b=1..256} zeta^(-b r2) y_a'[b], y_a'[b] =
// in[a' 256 + b - 1][p] (r2 = 0..256), then h_j = sum_a' lam1[a'][r2 mod 3] E_a'[r2] (j = r2) and
// h_(r2+257) with lam2, c1 = h_513, c0 = h_512 - c1 phi_511, f_j = h_j - c0 phi_j - c1 phi_(j-1) (j < 512).  For
// r2 != 0 the sum is the cyclic convolution of a[n] = y[g^n] with conj(bk) (E[g^-m] = conv[m]); E[0] = sum_b y[b]
// is FFT(a)[0].  E at r2 = 0, 255, 256 (the c's and f_0, f_257) reach every thread of the column through LDS.
__global__ __launch_bounds__(RDC * 16) void wdft_rader_inv_kernel(const double2* __restrict__ in, double2* __restrict__ out,
                                                                  double* __restrict__ out_im, uint32_t Pf,
                                                                  const double2* __restrict__ rb,
                                                                  const int16_t* __restrict__ gp,
                                                                  const double2* __restrict__ lam,
                                                                  const int8_t* __restrict__ phi) {
    __shared__ double2 tw[256];
    __shared__ double2 fb[256];
    __shared__ int16_t sg[512];
    __shared__ double2 xs[RDC][2][16][17];
    __shared__ double2 ex[RDC][2][3];            // E_a'[0], E_a'[255], E_a'[256] per column
    const int t = threadIdx.x & 15, pc = threadIdx.x >> 4;
    for (int i = threadIdx.x; i < 256; i += RDC * 16) {
        double sn, cs;
        sincospi(-(double)i / 128.0, &sn, &cs);
        tw[i] = make_double2(cs, sn);
        fb[i] = rb[i];
        sg[i] = gp[i];
        sg[256 + i] = gp[256 + i];
    }
    __syncthreads();
    const uint32_t p = blockIdx.x * RDC + pc;
    const bool live = p < Pf;
    const uint32_t pr = live ? p : 0;
    double2 x[2][16];
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int s = 0; s < 16; ++s) x[ap][s] = in[(uint64_t)(ap * 256 + sg[t + 16 * s] - 1) * Pf + pr];
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
        fft16<-1>(x[ap]);
#pragma unroll
        for (int k1 = 1; k1 < 16; ++k1) x[ap][k1] = cmul(x[ap][k1], tw[(t * k1) & 255]);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) xs[pc][ap][k1][t] = x[ap][k1];
    }
    __syncthreads();
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
#pragma unroll
        for (int tt = 0; tt < 16; ++tt) x[ap][tt] = xs[pc][ap][t][tt];
        fft16<-1>(x[ap]);
        if (t == 0) ex[pc][ap][0] = x[ap][0];   // E[0] = sum_b y[b] = FFT(a)[0]
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) x[ap][k2] = cmul(x[ap][k2], fb[t + 16 * k2]);
        fft16<1>(x[ap]);
#pragma unroll
        for (int u = 1; u < 16; ++u) x[ap][u] = cmul(x[ap][u], cconj(tw[(u * t) & 255]));
    }
    __syncthreads();
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int u = 0; u < 16; ++u) xs[pc][ap][u][t] = x[ap][u];
    __syncthreads();
#pragma unroll
    for (int ap = 0; ap < 2; ++ap) {
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) x[ap][k1] = xs[pc][ap][t][k1];
        fft16<1>(x[ap]);   // E[g^-m] for m = t + 16 v in x[ap][v]
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r2 = sg[256 + t + 16 * v];
            if (r2 == 255) ex[pc][ap][1] = x[ap][v];
            if (r2 == 256) ex[pc][ap][2] = x[ap][v];
        }
    }
    __syncthreads();
    auto L = [&](int kind, int aa, int t3) { return lam[(kind * 2 + aa) * 3 + t3]; };
    auto comb = [&](int kind, int t3, double2 e0, double2 e1) { return cadd(cmul(L(kind, 0, t3), e0), cmul(L(kind, 1, t3), e1)); };
    const double2 E00 = ex[pc][0][0], E10 = ex[pc][1][0];
    const double2 c1 = comb(1, 1, ex[pc][0][2], ex[pc][1][2]);                         // h_513 (r2 = 256, t = 1)
    const double2 h512 = comb(1, 0, ex[pc][0][1], ex[pc][1][1]);                       // r2 = 255, t = 0
    const double p511 = (double)phi[511];
    const double2 c0 = make_double2(h512.x - c1.x * p511, h512.y - c1.y * p511);
    if (!live) return;
    auto put = [&](int j, double2 h) {   // f_j = h_j - c0 phi_j - c1 phi_(j-1)
        const double f0 = (double)phi[j], f1 = j > 0 ? (double)phi[j - 1] : 0.0;
        const double re = h.x - c0.x * f0 - c1.x * f1, im = h.y - c0.y * f0 - c1.y * f1;
        const uint64_t idx = (uint64_t)j * Pf + p;
        if (out_im) {
            ((double*)out)[idx] = re;
            out_im[idx] = im;
        } else {
            out[idx] = make_double2(re, im);
        }
    };
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r2 = sg[256 + t + 16 * v], t3 = r2 % 3;
        put(r2, comb(0, t3, x[0][v], x[1][v]));
        if (r2 <= 254) put(r2 + 257, comb(1, t3, x[0][v], x[1][v]));
    }
    if (t == 0) {
        put(0, comb(0, 0, E00, E10));
        put(257, comb(1, 0, E00, E10));
    }
}

int launch_wdft_rader_inv(const double2* in, double2* out, double* out_im, uint32_t Pf, const double2* rb,
                          const int16_t* gp, const double2* lam, const int8_t* phi, hipStream_t s) {
    if (!in || !out || !rb || !gp || !lam || !phi || Pf == 0 || in == out)
        return set_error(MFHE_EINVAL, "wdft_rader_inv: bad arguments");
    hipLaunchKernelGGL(wdft_rader_inv_kernel, dim3((Pf + RDC - 1) / RDC), dim3(RDC * 16), 0, s, in, out, out_im, Pf, rb,
                       gp, lam, phi);
    MFHE_CHECK_LAUNCH("wdft_rader_inv_kernel");
    return MFHE_OK;
}

int launch_wdft_rader(const double2* in, double2* out, uint32_t Pf, const double2* rb, const int16_t* gp, hipStream_t s) {
    if (!in || !out || !rb || !gp || Pf == 0 || in == out) return set_error(MFHE_EINVAL, "wdft_rader: bad arguments");
    hipLaunchKernelGGL(wdft_rader_kernel, dim3((Pf + RDC - 1) / RDC), dim3(RDC * 16), 0, s, in, out, Pf, rb, gp);
    MFHE_CHECK_LAUNCH("wdft_rader_kernel");
    return MFHE_OK;
}

// ---- the per-lane XY transforms by FFT (r06, n = 64) ----
// V[j][k] = zeta^(g_j k), zeta = e^(2 pi i / 256), g_j = 5^j mod 256 (ctx.cpp ensure_xy, encoder.cu:425-444).  Every
// g_j is 1 mod 4 and j -> (g_j - 1) / 4 is a permutation of 0..63, so (V x)[j] = sum_k (x[k] zeta^k) w^(k (g_j-1)/4)
// with w = e^(2 pi i / 64): a 64-point DFT of the twisted column, its output i' landing at j = jinv[i'].  V^-1 =
// V^H / 64 runs backwards: the input permuted to u[i'] = z[jinv[i']], the DFT with e^(-2 pi i / 64), the output
// times zeta^-k / 64.  xy3's out = V M V^T (decode) or V^-1 M V^-T (encode) is the transform of every column, a
// transpose, the transform of every row: 2 x 64 DFTs of 64 points per lane instead of two 64^3 complex GEMMs, so
// the launch is bound by its 64 KB in and out per lane.  The twiddles are single cos / sin values, the GEMMs' V a
// chain of products: equal to rounding (~1e-15 relative), not bit for bit.  One workgroup per lane, eight waves:
// in each pass thread (c, q) holds x[q + 8 s] (s = 0..7) of transform c, runs the 8-point DFT over s and the
// twiddle w^(q k1), and after an exchange through LDS the 8-point DFT over q for k1 = q; the results go back to
// LDS transposed, so the second pass reads rows the way the first read columns.  (Four waves with a 16 x 4
// split: 18.9 / 21.3 us per call.)
constexpr int XFP = 65;   // LDS row pitch (double2)
// in-register 8-point DFT, natural order in and out: X[k] = sum_s x[s] e^(SIGN 2 pi i s k / 8)
template <int SIGN>
__device__ __forceinline__ void fft8(double2 (&x)[8]) {
    auto sw = [&](int i, int j) {
        const double2 t = x[i];
        x[i] = x[j];
        x[j] = t;
    };
    sw(1, 4); sw(3, 6);   // 3-bit reversal
#pragma unroll
    for (int len = 2; len <= 8; len <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i += len)
#pragma unroll
            for (int j = 0; j < len / 2; ++j) {
                const int k = j * (8 / len);
                const double2 u = x[i + j], v = k == 0 ? x[i + j + len / 2] : cmul(x[i + j + len / 2], w16<SIGN>(2 * k));
                x[i + j] = cadd(u, v);
                x[i + j + len / 2] = csub(u, v);
            }
}
template <bool INV>
__global__ __launch_bounds__(512) void xy_fft_kernel(const double2* __restrict__ in, double2* __restrict__ out) {
    __shared__ double2 S[64 * XFP];
    __shared__ double2 tz[256];   // e^(2 pi i m / 256)
    __shared__ int jinv[64];
    constexpr int SG = INV ? -1 : 1;
    const int t = threadIdx.x, c = t & 63, q = t >> 6;
    if (t < 256) {
        double sn, cs;
        sincospi((double)t / 128.0, &sn, &cs);
        tz[t] = make_double2(cs, sn);
    } else if (t < 320) {
        int g = 1;
        for (int i = 0; i < t - 256; ++i) g = (g * 5) & 255;
        jinv[(g - 1) >> 2] = t - 256;
    }
    const uint64_t lb = (uint64_t)blockIdx.x * 4096;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int idx = t + 512 * e;
        S[(idx >> 6) * XFP + (idx & 63)] = in[lb + idx];
    }
    __syncthreads();
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        double2 x[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int n = q + 8 * s;
            x[s] = INV ? S[jinv[n] * XFP + c] : cmul(S[n * XFP + c], tz[n]);
        }
        fft8<SG>(x);
#pragma unroll
        for (int k1 = 1; k1 < 8; ++k1) {
            const double2 w = tz[(4 * q * k1) & 255];
            x[k1] = cmul(x[k1], INV ? cconj(w) : w);
        }
        __syncthreads();   // every thread has read its inputs
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) S[(8 * q + k1) * XFP + c] = x[k1];
        __syncthreads();
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) x[qq] = S[(8 * qq + q) * XFP + c];   // k1 = q
        fft8<SG>(x);                                                          // X[q + 8 k2] in x[k2]
        __syncthreads();   // every thread has read the exchange
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            const int i = q + 8 * k2;
            if (INV) {
                const double2 v = cmul(x[k2], cconj(tz[i]));
                S[c * XFP + i] = make_double2(v.x * 0.015625, v.y * 0.015625);
            } else {
                S[c * XFP + jinv[i]] = x[k2];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int idx = t + 512 * e;
        out[lb + idx] = S[(idx >> 6) * XFP + (idx & 63)];
    }
}

int launch_xy_fft(const double2* in, double2* out, bool inv, int lanes, hipStream_t s) {
    if (!in || !out || lanes <= 0) return set_error(MFHE_EINVAL, "xy_fft: bad arguments");
    if (inv) hipLaunchKernelGGL(xy_fft_kernel<true>, dim3((uint32_t)lanes), dim3(512), 0, s, in, out);
    else hipLaunchKernelGGL(xy_fft_kernel<false>, dim3((uint32_t)lanes), dim3(512), 0, s, in, out);
    MFHE_CHECK_LAUNCH("xy_fft_kernel");
    return MFHE_OK;
}

int launch_cgemm(const CGemmArgs& a, int batch, hipStream_t s) {
    dim3 grid((a.P + TP - 1) / TP, (a.M + TM - 1) / TM, batch);
    if (a.mfma) {
        if (a.fac == 1) hipLaunchKernelGGL(cgemm_mfma_kernel<1>, grid, dim3(NTH), 0, s, a);
        else if (a.fac == 2) hipLaunchKernelGGL(cgemm_mfma_kernel<2>, grid, dim3(NTH), 0, s, a);
        else hipLaunchKernelGGL(cgemm_mfma_kernel<0>, grid, dim3(NTH), 0, s, a);
        MFHE_CHECK_LAUNCH("cgemm_mfma_kernel");
    } else {
        hipLaunchKernelGGL(cgemm_kernel, grid, dim3(NTH), 0, s, a);
        MFHE_CHECK_LAUNCH("cgemm_kernel");
    }
    return MFHE_OK;
}

}  // namespace mfhe

// wcrt_digitize.hpp -- the digit-plane layout of the i8 MFMA W-CRT GEMM and the kernels that write B's planes:
// dense, factored forward (four sources, pair form), factored inverse, and the inverse with the decrypt fused in
// front (single and pair, with the column-sum kernels of a split launch).  Included by wcrt_gemm.hip only.
#pragma once
#include "he_sample.hpp"
#include "mfhe_ctx.hpp"
#include "ring_row.hpp"
#include "wcrt_gemm.hpp"

#ifndef MFHE_DEC_WG_CU
#define MFHE_DEC_WG_CU 1  // decrypt-fused digitize: minimum workgroups per CU for the register budget (A/B knob)
#endif
#ifndef MFHE_DEC_SUBS
#define MFHE_DEC_SUBS 4   // decrypt-fused digitize: 16-row substeps loaded together (1, 2 or 4)
#endif
#ifndef MFHE_DEC_NT
#define MFHE_DEC_NT 1   // decrypt-fused digitize: the ciphertext loads nontemporal (read once; 0 for A/B)
#endif
#ifndef MFHE_DEC_SPLIT
#define MFHE_DEC_SPLIT 4   // decrypt-fused digitize: workgroups per (row, limb), each 8 / MFHE_DEC_SPLIT panels
#endif

namespace mfhe {

// ---------------- i8 MFMA modular GEMM (W-CRT, M = K = 512) ----------------
//
// Exact integer product through v_mfma_i32_32x32x32_i8: every operand x < q < 2^(8D-1) is written in
// D balanced base-256 digits x = sum_i d_i 256^i, d_i in [-128, 127].  For each s = i + j the
// digit-pair products accumulate in one i32 tile acc_s = sum_{i+j=s} A_i B_j (|acc_s| <= D * 2^14 * 512
// < 2^26 for D <= 8, exact), and the epilogue folds C = sum_s acc_s * (256^s mod q) mod q.
// A's digit planes are built once per context; B is split by mfma_digitize_kernel into a
// [L][D][Ppad][K] workspace (K contiguous) so both fragments are single 16-byte loads per lane
// (probe: tools/microbench/mfma_i8_probe.hip; any k order shared by A and B is valid).
constexpr int MK = 512;   // K of the W-CRT GEMM

using v4i = int __attribute__((ext_vector_type(4)));
using v16i = int __attribute__((ext_vector_type(16)));

// Digit planes are "k-panel-major": [K/32][rows][32] bytes, so one 32-k panel of 64 consecutive rows (or
// columns) is 2 KiB of contiguous memory: every fragment load (16 B per lane, lanes over rows and k halves)
// and every digitize store below is a fully coalesced sweep.
//
// Balanced base-256 digits by offset: x = sum d_i 256^i with d_i in [-128, 127] iff
// y = x + 128 (256^D - 1) / 255 = x + 0x8080..80 has bytes d_i + 128, so d_i = byte_i(y) ^ 0x80 as an i8.
// Valid for -0x80..80 <= x <= 0x7F..7F (D bytes); the fold kernel's |x| <= q/2 + 1 is well inside.
template <int D>
__device__ __forceinline__ uint64_t balanced_bytes(double v) {   // v integral, |v| < 2^51
    constexpr double kMagic = 6755399441055744.0;                 // 1.5 * 2^52: bits(v + M) - bits(M) = v
    constexpr uint64_t kOff = 0x8080808080808080ull >> (64 - 8 * D);
    return (uint64_t)__double_as_longlong(v + kMagic) - ((uint64_t)__double_as_longlong(kMagic) - kOff);
}
// Byte transpose of digit words into digit-plane words (r06): rows 4c .. 4c + 3 of y (each row's D digit bytes in
// its low D bytes) give word c of every plane i = byte i of those four rows.  v_perm_b32 picks 4 of the 8 bytes of
// (S0:S1): rows (0, 1) and (2, 3) interleaved for two planes at once, then the halves joined -- three perms per two
// planes and four rows, instead of a shift, mask and or per byte.
template <int D, int R>
__device__ __forceinline__ void pack_planes(const uint64_t (&y)[R], uint32_t (&pk)[D][R / 4]) {
#pragma unroll
    for (int c = 0; c < R / 4; ++c)
#pragma unroll
        for (int pi = 0; pi < D; pi += 2) {
            const int sh = pi < 4 ? 0 : 32;
            const uint32_t i = (uint32_t)(pi & 3), j = i + 1;
            const uint32_t sel = i | ((4 + i) << 8) | (j << 16) | ((4 + j) << 24);
            const uint32_t t01 = __builtin_amdgcn_perm((uint32_t)(y[4 * c + 1] >> sh), (uint32_t)(y[4 * c] >> sh), sel);
            const uint32_t t23 = __builtin_amdgcn_perm((uint32_t)(y[4 * c + 3] >> sh), (uint32_t)(y[4 * c + 2] >> sh), sel);
            pk[pi][c] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
            if (pi + 1 < D) pk[pi + 1][c] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
        }
}

// digit planes the GEMM reads per limb (wcrt_gemm.hip limb_digits, <= D): planes past it are never read, so never
// written
struct PlaneCounts {
    uint8_t n[64];   // limbs >= 64: all D
};

// one thread: column p (of Ppad; zero past P), one 32-k panel; B (k, p) via the (sbK, sbY, log_n) map
template <int D>
__global__ __launch_bounds__(256) void mfma_digitize_kernel(const uint64_t* __restrict__ B, uint64_t bL,
                                                            uint64_t sbK, uint64_t sbY, int log_n, uint32_t P,
                                                            uint32_t Ppad, int8_t* __restrict__ out, PlaneCounts pc) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    const int kc = blockIdx.y;
    const int l = blockIdx.z;
    if (p >= Ppad) return;
    const uint64_t* Bl = B + (uint64_t)l * bL;
    const uint64_t col = (uint64_t)(p >> log_n) * sbY + (p & ((1u << log_n) - 1));
    // plane i, bytes 4c..4c+3 of the panel's 32 k.  Balanced digits by the offset rule: the bytes of x + 0x80..80
    // (D bytes; x < 2^(8D - 1)) are the digits + 128, so byte ^ 0x80 is the digit mod 256 (r05: a shift-and-carry
    // loop per digit; the same bytes)
    constexpr uint64_t kOff = 0x8080808080808080ull >> (64 - 8 * D);
    uint64_t y[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        const uint64_t x = Bl[(uint64_t)(kc * 32 + kk) * sbK + (p < P ? col : 0)];
        y[kk] = (p < P ? x : 0) + kOff;
    }
    uint32_t pk[D][8];
    pack_planes<D, 32>(y, pk);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) pk[i][c] ^= 0x80808080u;
    const int nd = l < 64 ? pc.n[l] : D;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (i >= nd) break;
        int8_t* o = out + (((uint64_t)l * D + i) * (MK / 32) + kc) * Ppad * 32 + (uint64_t)p * 32;
        *(v4i*)o = v4i{(int)pk[i][0], (int)pk[i][1], (int)pk[i][2], (int)pk[i][3]};
        *(v4i*)(o + 16) = v4i{(int)pk[i][4], (int)pk[i][5], (int)pk[i][6], (int)pk[i][7]};
    }
}

// ---- factored forward W-CRT (every q < 2^50) ----
// The 512 evaluation points are eta^e for the units e of Z_771 in the order e = 257 a + 3 b (a = 1, 2;
// b = 1..256; HE.cu:72-105, k_wntt_exp).  With omega = eta^257 (order 3) and zeta = eta^3 (order 257),
// x_w^r = omega^(a (r mod 3)) zeta^(b (r mod 257)), and since r < 512 < 771 each r2 = r mod 257 takes at
// most two r (r2 and r2 + 257):
//   out[a][b] = F_a[0] + sum_{k < 256} zeta^(b (k + 1)) F_a[k + 1],
//   F_a[r2]   = omega^(a (r2 mod 3)) in[r2] + omega^(a ((r2 + 2) mod 3)) in[r2 + 257]   (second term if < 512).
// That is a 256 x 256 GEMM over 2 P columns (a, p) instead of 512 x 512 over P: half the MACs, and the
// same linear map mod q, so bit-exact.  This kernel forms F_a (two FP64 modmuls per term), writes the
// digit planes of F_a[1..256] as the B operand ([L][D][8 panels][2 Ppad][32], column a' Ppad + p for
// a = a' + 1) and F_a[0] to d0[L][2][Ppad] for the GEMM epilogue.
// fold[l][16] = q, 1/q, omega^(a r1) [a'][r1], omega^(a ((r1 + 2) mod 3)) [a'][r1], all centred.
constexpr int FK = 256;   // K (and M) of the factored GEMM

// One thread: column p, one half (16 k) of a 32-k panel, both a; lane pairs share a column, so each
// 16-byte store completes a 1 KiB contiguous run per wave.  The digits need any representative of F_a mod q
// within the limb's digit range, so F_a is only reduced to the centred (-q/2, q/2] and split by the offset
// rule (balanced_bytes).
// SRC 1 (encode): B is not a residue matrix but the W-IDFT's doubles v[r][p] (row stride qf_row, element stride
// qf_step): each limb's residue is formed on the fly as round(v delta) mod q -- the RNS decompose
// (rns_decompose_kernel: llround, then the residue of the int64) fused away, exact for |v delta| < 2^63 (the
// centred FP64 reduction of the rounded double is exact while |x / q| < 2^51).  With any SRC the grid runs the
// limbs fastest (blockIdx.x), so the L blocks of one column range read the same doubles out of the L2.
// SRC 2 / 3 (encrypt): the uniform sampler's residue computed in place (seed from (w, limb, position) exactly as
// he.hip uniform_kernel, so no a[] in HBM), or the Gaussian noise read as one centred integer per coefficient.
struct FoldSrc {
    const double* qf = nullptr;
    uint64_t qf_row = 0, qf_step = 0;
    double delta = 0.0;
    const uint64_t* qmu = nullptr;   // SRC 2: [L][2] (q, floor(2^64 / q))
    int lbase = 0, Ltot = 0;
};
// PAIR (fused sources only): two components in one grid, blockIdx.x in [0, 2 L); the upper half writes fp's planes
// from fp's source (he.hip encode: re and im)
struct FoldPair {
    int L = 0;
    int8_t* out2 = nullptr;
    uint64_t* d02 = nullptr;
    const double* qf2 = nullptr;
};
template <int D, int SRC = 0, bool PAIR = false>
__global__ __launch_bounds__(256, 4) void mfma_digitize_fold_kernel(const uint64_t* __restrict__ B, uint64_t bL,
                                                                 uint64_t sbK, uint64_t sbY, int log_n, uint32_t P,
                                                                 uint32_t Ppad, const double* __restrict__ fold,
                                                                 int8_t* __restrict__ out, uint64_t* __restrict__ d0,
                                                                 PlaneCounts pc, FoldSrc fs = FoldSrc{},
                                                                 FoldPair fp = FoldPair{}) {
    constexpr bool QF = SRC != 0;
    static_assert(!PAIR || QF, "pair launches: fused sources only");
    const double* __restrict__ qf = fs.qf;
    const uint64_t qf_row = fs.qf_row, qf_step = fs.qf_step;
    const double delta = fs.delta;
    const uint32_t p = (QF ? blockIdx.y : blockIdx.x) * 128 + (threadIdx.x >> 1);
    const int hf = threadIdx.x & 1;
    const int kc = QF ? blockIdx.z : blockIdx.y;   // panel: r2 = 32 kc + 16 hf + 1 .. 32 kc + 16 hf + 16
    int lx = QF ? blockIdx.x : blockIdx.z;
    if constexpr (PAIR) {
        if (lx >= fp.L) {
            lx -= fp.L;
            out = fp.out2;
            d0 = fp.d02;
            qf = fp.qf2;
        }
    }
    const int l = lx;
    if (p >= Ppad) return;
    const double* fo = fold + (uint64_t)l * 16;
    LimbConst lc;
    lc.qf = fo[0];
    lc.qinv = fo[1];
    const ArithF64 ar(lc);
    double c1[2][3], c2[2][3];
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int r1 = 0; r1 < 3; ++r1) {
            c1[ap][r1] = fo[2 + 3 * ap + r1];
            c2[ap][r1] = fo[8 + 3 * ap + r1];
        }
    const uint64_t* Bl = B + (uint64_t)l * bL;
    const uint64_t col = (uint64_t)(p >> log_n) * sbY + (p & ((1u << log_n) - 1));
    const bool live = p < P;
    // unconditional loads (column 0 stands in for the padding columns, then zeroed): a load under `live ? :` is
    // a branch per load, each followed by its own vmcnt(0) -- the 32 loads of a thread ran one at a time
    const uint64_t cl = live ? col : 0;
    uint64_t uq = 0, umu = 0;
    if constexpr (SRC == 2) {
        uq = fs.qmu[2 * l];
        umu = fs.qmu[2 * l + 1];
    }
    // SRC 2: the sampler's word for row r (he_sample.hpp uniform_seed, as he.hip uniform_kernel draws it).  It is affine
    // in r: with the per-row step K = (Ltot << 2 log n) A, row r + 1's word is row r's + K, and row r + 257's is row
    // r's + 257 K -- 64-bit adds in the row loop instead of a 64-bit multiply per value, the same words (in(r) keeps
    // the direct form for the d0 rows).
    uint64_t lcgK = 0, lcgK257 = 0;
    if constexpr (SRC == 2) {
        lcgK = ((uint64_t)fs.Ltot << (2 * log_n)) * kUniformLcgA;
        lcgK257 = lcgK * 257ull;
    }
    auto lcg_seed = [&](int r) {
        const uint32_t pp = live ? p : 0;
        return uniform_seed((uint64_t)r, (uint64_t)(fs.lbase + l), (uint64_t)fs.Ltot, log_n, pp);
    };
    auto sampled = [&](uint64_t seed) {
        const uint64_t v = uniform_reduce(seed, uq, umu);   // outside the select: dead lanes take no branch round it
        return live ? ArithF64::from_u64(v) : 0.0;
    };
    auto in = [&](int r) {
        double x;
        const uint32_t pp = live ? p : 0;
        if constexpr (SRC == 1) {
            x = ar.reduce(round(qf[(uint64_t)r * qf_row + (uint64_t)pp * qf_step] * delta));
        } else if constexpr (SRC == 2) {
            return sampled(lcg_seed(r));
        } else if constexpr (SRC == 3) {
            x = qf[(uint64_t)r * qf_row + pp];
        } else {
            x = ArithF64::from_u64(Bl[(uint64_t)r * sbK + cl]);
        }
        return live ? x : 0.0;
    };
    uint32_t pk[2][D][4];
    uint32_t ylo[2][4], yhi[2][4];   // the current group of four rows' digit words
    const int rb = kc * 32 + hf * 16 + 1;
    // r06: F_a = omega^(a r1) (x1 + omega^(2a) x2) and omega^2 = -1 - omega, so with m = omega x2
    //   F_1 = omega^r1 (x1 - x2 - m),  F_2 = omega^(2 r1) (x1 + m)
    // -- three modmuls per r2 instead of four (|x1 - x2 - m| <= 3q: inside mulmod's |v| <= 4q); the same residues,
    // other representatives, so other digits but the same GEMM result mod q.  The weights omega^(a r1) are rotated
    // once to this thread's first r2 mod 3, so the unrolled loop indexes them by kk % 3 (the per-row selects by a
    // runtime r1 were ~200 of the kernel's ~1830 VALU instructions).
    const double omega = c1[0][1];
    const int r10 = rb % 3;
    double wr[2][3];
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e0 = j, e1 = (j + 1) % 3, e2 = (j + 2) % 3;   // (r10 + j) mod 3 for r10 = 0, 1, 2
            wr[ap][j] = r10 == 0 ? c1[ap][e0] : (r10 == 1 ? c1[ap][e1] : c1[ap][e2]);
        }
    uint64_t seed1 = 0;
    if constexpr (SRC == 2) seed1 = lcg_seed(rb);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int r2 = rb + kk;
        double x1, x2r;
        if constexpr (SRC == 2) {
            x1 = sampled(seed1);
            x2r = sampled(seed1 + lcgK257);   // row r2 + 257 (unused past row 511)
            seed1 += lcgK;
        } else {
            x1 = in(r2);
            x2r = in(r2 + 257 < 512 ? r2 + 257 : 511);
        }
        const double x2 = r2 + 257 < 512 ? x2r : 0.0;
        const double m = ar.mulmod(x2, omega);
        const double fin[2] = {x1 - x2 - m, x1 + m};
#pragma unroll
        for (int ap = 0; ap < 2; ++ap) {
            const double v = ar.reduce(ar.mulmod(fin[ap], wr[ap][kk % 3]));   // |v| <= q/2 + eps
            const uint64_t y = balanced_bytes<D>(v);
            ylo[ap][kk & 3] = (uint32_t)y;
            yhi[ap][kk & 3] = (uint32_t)(y >> 32);
        }
        if ((kk & 3) == 3) {
            // byte transpose of four rows' digits into the planes' words: plane i's word = byte i of rows 0..3.
            // v_perm_b32 picks 4 of the 8 bytes of (S0:S1): first rows (0, 1) and (2, 3) interleaved for two planes
            // at once, then the two halves joined -- 3 perms per two planes instead of a shift, mask and or per byte
#pragma unroll
            for (int ap = 0; ap < 2; ++ap)
#pragma unroll
                for (int pi = 0; pi < D; pi += 2) {
                    const uint32_t* src = pi < 4 ? ylo[ap] : yhi[ap];
                    const uint32_t i = (uint32_t)(pi & 3), j = i + 1;
                    const uint32_t sel = i | ((4 + i) << 8) | (j << 16) | ((4 + j) << 24);
                    const uint32_t t01 = __builtin_amdgcn_perm(src[1], src[0], sel);
                    const uint32_t t23 = __builtin_amdgcn_perm(src[3], src[2], sel);
                    pk[ap][pi][kk >> 2] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
                    if (pi + 1 < D) pk[ap][pi + 1][kk >> 2] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
                }
        }
    }
    if (kc == 0 && hf == 0) {
        const double x1 = in(0), x2 = in(257);
#pragma unroll
        for (int ap = 0; ap < 2; ++ap)
            d0[((uint64_t)l * 2 + ap) * Ppad + p] = ar.canon(ar.mulmod(x1, c1[ap][0]) + ar.mulmod(x2, c2[ap][0]));
    }
    const int nd = l < 64 ? pc.n[l] : D;
#pragma unroll
    for (int ap = 0; ap < 2; ++ap)
#pragma unroll
        for (int i = 0; i < D; ++i) {
            if (i >= nd) break;
            int8_t* o = out + ((((uint64_t)l * D + i) * (FK / 32) + kc) * 2 * Ppad + (uint64_t)ap * Ppad + p) * 32 + hf * 16;
            const uint32_t* w = pk[ap][i];
            *(v4i*)o = v4i{(int)(w[0] ^ 0x80808080u), (int)(w[1] ^ 0x80808080u), (int)(w[2] ^ 0x80808080u),
                           (int)(w[3] ^ 0x80808080u)};
        }
}

// ---- factored inverse W-CRT (every q < 2^50; tools/wcrt_factor_check.py) ----
// V^-1 y is the 771-point inverse DFT of the 512 values (zeros at the 259 non-unit exponents), reduced mod
// Phi_771.  With the forward's e = 257 a + 3 b order, E_a[r2] = sum_{b=1..256} zeta^(-b r2) y[a][b] (r2 = 0..256) and
//   g_r = 771^-1 sum_a omega^(-a r) E_a[r mod 257]                       (r = 0..770)
//   h_j = g_j - g_(j+514) (j <= 256),  h_j = g_j - g_(j+257) (257 <= j <= 513)   (mod x^514 + x^257 + 1)
//   f_j = h_j - c0 phi_j - c1 phi_(j-1),  c1 = h_513, c0 = h_512 - c1 phi_511       (mod Phi_771, j < 512)
// j = r2, r2 + 257 and r2 + 514 share E_a[r2], so per GEMM row r2 = 1..256 (a 256 x 256 GEMM over 2 P columns
// interleaved as 2 p + a'): h_r2 = sum_a lam1[a][r2 mod 3] E_a[r2], h_(r2+257) = sum_a lam2[a][r2 mod 3] E_a[r2].
// The digitize kernel below also forms the rows r2 = 0 (-> f_0, f_257), 255 and 256 (-> c0, c1 per column) by
// dot products, so the GEMM epilogue writes the final f directly: half the MACs of the dense V^-1 product.

// One 16-k chunk v (b = k0 + 1 + i, reduced) into the column sums s0 = E[0], s1 = E[255], s2 = E[256]:
// sum_b x^b v_b as x^(k0+1) * Horner(v, x) for x = x1 = zeta^-255, x2 = zeta^-256 (zp: the chunk powers x1^(k0+1) at
// [k0 / 16], x2^(k0+1) at [16 + k0 / 16]): no per-element table, two independent chains (|h| <= q + 1 between steps:
// mulmod's range holds), and the plain sum for x = 1
__device__ __forceinline__ void ifold_chunk_sums(const ArithF64& ar, const double (&v)[16], double x1, double x2,
                                                 const double* zp, int k0, double& s0, double& s1, double& s2) {
    double h1 = v[15], h2 = v[15], t0 = 0.0;
#pragma unroll
    for (int kk = 14; kk >= 0; --kk) {
        h1 = ar.mulmod(h1, x1) + v[kk];
        h2 = ar.mulmod(h2, x2) + v[kk];
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) t0 += v[kk];   // |t0| <= 8 q < 2^53
    s0 = ar.reduce(s0 + t0);
    s1 = ar.reduce(s1 + ar.mulmod(h1, zp[(k0 >> 4)]));
    s2 = ar.reduce(s2 + ar.mulmod(h2, zp[16 + (k0 >> 4)]));
}

// One thread: column p = 16 blockIdx.x + lane / 4, a' = (lane >> 1) & 1, half panel hf = lane & 1 (16 k), k quarter
// = wave (two 32-k panels): lane l's 16-byte digit store lands at byte 16 l of a contiguous 1 KiB run.
template <int D>
__global__ __launch_bounds__(256) void mfma_digitize_ifold_kernel(ModGemmArgs a, uint32_t Ppad, PlaneCounts pc) {
    __shared__ double red[3][4][64];
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * 16 + (lane >> 2);
    const int ap = (lane >> 1) & 1, hf = lane & 1;
    const int l = blockIdx.y;
    typedef const __attribute__((address_space(4))) double* cdp_t;
    const cdp_t fo = (cdp_t)(a.ifold + (uint64_t)l * 16);
    LimbConst lc;
    lc.qf = fo[0];
    lc.qinv = fo[1];
    const ArithF64 ar(lc);
    // iz[l] = (x1, x2, pad[14], x1^(16 j + 1) for j < 16, x2^(16 j + 1) for j < 16), x1 = zeta^-255, x2 = zeta^-256
    const double* izl = a.iz + (uint64_t)l * 48;
    const double x1 = ((cdp_t)izl)[0], x2 = ((cdp_t)izl)[1];
    const double* zp = izl + 16;
    const uint64_t* Bl = a.B + (uint64_t)l * a.bL;
    const uint32_t nmask = (1u << a.log_n) - 1;
    const uint64_t col = (uint64_t)(p >> a.log_n) * a.sbY + (p & nmask);
    const bool live = p < a.P;
    const uint64_t cl = live ? col : 0;   // unconditional loads (see mfma_digitize_fold_kernel)
    const int nd = l < 64 ? pc.n[l] : D;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;   // E_a'[0], E_a'[255], E_a'[256] over this thread's 32 k
#pragma unroll 1
    for (int pn = 0; pn < 2; ++pn) {
        const int kc = 2 * kq + pn, k0 = kc * 32 + hf * 16;
        uint32_t pk[D][4];
        double v[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)   // b = k0 + kk + 1
            v[kk] = ArithF64::from_u64(Bl[(uint64_t)(ap * FK + k0 + kk) * a.sbK + cl]);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) v[kk] = live ? ar.reduce(v[kk]) : 0.0;
        ifold_chunk_sums(ar, v, x1, x2, zp, k0, s0, s1, s2);
        {
            uint64_t y[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) y[kk] = balanced_bytes<D>(v[kk]);
            pack_planes<D, 16>(y, pk);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            if (i >= nd) break;
            int8_t* o = a.Bdig + (((uint64_t)l * D + i) * (FK / 32) + kc) * 2 * Ppad * 32 + (uint64_t)blockIdx.x * 1024 +
                        lane * 16;
            const uint32_t* w = pk[i];
            *(v4i*)o = v4i{(int)(w[0] ^ 0x80808080u), (int)(w[1] ^ 0x80808080u), (int)(w[2] ^ 0x80808080u),
                           (int)(w[3] ^ 0x80808080u)};
        }
    }
    // halves of a panel -> lanes l, l ^ 1; quarters -> the four waves (LDS); a' -> lanes l, l ^ 2
    s0 += __shfl_xor(s0, 1);
    s1 += __shfl_xor(s1, 1);
    s2 += __shfl_xor(s2, 1);
    red[0][kq][lane] = s0;
    red[1][kq][lane] = s1;
    red[2][kq][lane] = s2;
    __syncthreads();
    if (kq != 0) return;   // wave 0 finishes (no barrier below)
    double e[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) e[t] = ar.reduce(red[t][0][lane] + red[t][1][lane] + red[t][2][lane] + red[t][3][lane]);
    double o[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) o[t] = __shfl_xor(e[t], 2);
    const double e1[3] = {ap ? o[0] : e[0], ap ? o[1] : e[1], ap ? o[2] : e[2]};   // a = 1
    const double e2[3] = {ap ? e[0] : o[0], ap ? e[1] : o[1], ap ? e[2] : o[2]};   // a = 2
    // fo[2 + 3 a' + t] = lam1[a'][t], fo[8 + 3 a' + t] = lam2[a'][t]
    const double h0 = ar.mulmod(e1[0], fo[2]) + ar.mulmod(e2[0], fo[5]);          // r2 = 0, t = 0
    const double h257 = ar.mulmod(e1[0], fo[8]) + ar.mulmod(e2[0], fo[11]);
    const double h512 = ar.mulmod(e1[1], fo[8]) + ar.mulmod(e2[1], fo[11]);       // r2 = 255, t = 0
    const double h513 = ar.mulmod(e1[2], fo[9]) + ar.mulmod(e2[2], fo[12]);       // r2 = 256, t = 1
    // packed Phi_771 rows (mfhe_ctx::d_wphi): byte r2 - 1 (r2 = 1..256; r2 = 0 at byte 256) holds phi_r2, phi_(r2-1),
    // phi_(r2+257), phi_(r2+256) as 2-bit fields (value + 1) at shifts 0, 2, 4, 6
    auto phi = [&](int byte, int sh) { return (double)((int)((a.phi[byte] >> sh) & 3) - 1); };
    const double c1 = ar.reduce(h513);
    const double c0 = ar.reduce(h512 - c1 * phi(254, 6));   // phi_511 = phi_(r2+256) at r2 = 255
    if (!live || hf) return;
    uint64_t* Cl = a.C + (uint64_t)l * a.cL + (uint64_t)(p >> a.log_n) * a.scY + (p & nmask);
    if (ap == 0) {
        Cl[0] = ar.canon(h0 - c0 * phi(256, 0));
        a.cc[((uint64_t)l * Ppad + p) * 2] = c0;
        a.cc[((uint64_t)l * Ppad + p) * 2 + 1] = c1;
    } else {
        Cl[257 * a.scM] = ar.canon(h257 - c0 * phi(256, 4) - c1 * phi(256, 6));
    }
}

// rows r2 = 0, 255, 256 of the factored inverse from the column sums E_a'[0], E_a'[255], E_a'[256] (a = 1: e1,
// a = 2: e2), as at the end of mfma_digitize_ifold_kernel: f_0 and f_257 into C, (c0, c1) into cc
template <class FO>
__device__ __forceinline__ void ifold_finish(const ModGemmArgs& a, const ArithF64& ar, FO fo, const double (&e1)[3],
                                             const double (&e2)[3], int l, uint32_t Ppad, uint32_t p) {
    const double h0 = ar.mulmod(e1[0], fo[2]) + ar.mulmod(e2[0], fo[5]);
    const double h257 = ar.mulmod(e1[0], fo[8]) + ar.mulmod(e2[0], fo[11]);
    const double h512 = ar.mulmod(e1[1], fo[8]) + ar.mulmod(e2[1], fo[11]);
    const double h513 = ar.mulmod(e1[2], fo[9]) + ar.mulmod(e2[2], fo[12]);
    auto phi = [&](int byte, int sh) { return (double)((int)((a.phi[byte] >> sh) & 3) - 1); };
    const double c1 = ar.reduce(h513);
    const double c0 = ar.reduce(h512 - c1 * phi(254, 6));
    const uint32_t nmask = (1u << a.log_n) - 1;
    uint64_t* Cl = a.C + (uint64_t)l * a.cL + (uint64_t)(p >> a.log_n) * a.scY + (p & nmask);
    Cl[0] = ar.canon(h0 - c0 * phi(256, 0));
    Cl[257 * a.scM] = ar.canon(h257 - c0 * phi(256, 4) - c1 * phi(256, 6));
    a.cc[((uint64_t)l * Ppad + p) * 2] = c0;
    a.cc[((uint64_t)l * Ppad + p) * 2 + 1] = c1;
}

// The same digitize with the decrypt fused in front of it (n = 64, he.hip mfhe_decrypt_and_decode): B is never
// written to HBM.  One workgroup owns limb l and row y: the 64 columns p = 64 y + x over all 512 k (= w), so the
// whole X row of every (w, l, y) -- what the ring product needs -- is inside the workgroup, and the column sums
// s0 / s1 / s2 stay in it.  Per 32-k panel kc (eight iterations):
//   ring: 64 rows w = a' 256 + 32 kc + (0..31) (a' = 0, 1), 16 lanes per row (ring_row.hpp), B = ct.b +
//         INTT(NTT(ct.a) s) mod q exactly as dec_ring_kernel, reduced as the digitize reduces it, into LDS [row][x];
//   digitize: wave c = 2 a' + hf takes the 16 k of (a', hf) at column x = lane, the four waves fill each column's
//         64-byte (a', hf) group of the kc plane: 4 KiB contiguous per plane and iteration.
// Reads: ct (16 B per element) + s (L2-resident); writes: the digit planes.  The B round trip of the unfused path
// (8 B written by dec_ring_kernel + 8 B read here per element) and one launch per component are gone.
template <int D>
__device__ __forceinline__ void ifold_dec_impl(const ModGemmArgs& a, uint32_t Ppad, const PlaneCounts& pc, const int l,
                                               const int L) {
    constexpr int LOGN = 6, N = 64, RS = N + 2;   // row stride 528 B: the ring's 16-B row writes spread over banks
    __shared__ __attribute__((aligned(16))) double bt[64 * RS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t y = blockIdx.x;
    typedef const __attribute__((address_space(4))) double* cdp_t;
    const cdp_t fo = (cdp_t)(a.ifold + (uint64_t)l * 16);
    LimbConst lc;
    lc.qf = fo[0];
    lc.qinv = fo[1];
    const ArithF64 ar(lc);
    const LimbConst rl = ((const LimbConst*)a.dlf)[l];
    const ArithF64 rar(rl);
    const double* izl = a.iz + (uint64_t)l * 48;
    const double x1 = ((cdp_t)izl)[0], x2 = ((cdp_t)izl)[1];
    const double* zp = izl + 16;
    const int nd = l < 64 ? pc.n[l] : D;
    // ring-stage lane: 4 coefficients 4 j .. 4 j + 3 of row 16 s + rs (s = 0..3)
    const int j = t & 15, rs = t >> 4;
    const double* tw = a.dtw + (uint64_t)l * N;
    const double* itw = a.ditw + (uint64_t)l * N;
    const double ninv = a.dninv[l];
    // digitize-stage lane: column x = lane, (a', hf) = wave
    const int ap = wv >> 1, hf = wv & 1;
    const uint32_t p = y * N + lane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    // all four substeps' loads are issued before the first ring product (measured: a one-substep-ahead rolling
    // prefetch needs 186 VGPRs, 2 workgroups per CU, or spills at 3: 2-5% slower, profiles/r04_dec_fused_ab.txt)
    const int kpg = FK / 32 / (int)gridDim.z, kc0 = blockIdx.z * kpg;   // this block's share of the panels
#pragma unroll 1
    for (int kc = kc0; kc < kc0 + kpg; ++kc) {
#pragma unroll
        for (int sb = 0; sb < 4; sb += MFHE_DEC_SUBS) {   // MFHE_DEC_SUBS substeps' loads in flight together
        uint64_t av[MFHE_DEC_SUBS][4], sk[MFHE_DEC_SUBS][4], bv[MFHE_DEC_SUBS][4];
#pragma unroll
        for (int si = 0; si < MFHE_DEC_SUBS; ++si) {
            const int st = sb + si;
            const int rr = st * 16 + rs;
            const uint64_t w = (uint64_t)(rr >> 5) * FK + kc * 32 + (rr & 31);
            const uint64_t wl = w * L + l, r0 = (wl * N + y) * N;
            ld4<MFHE_DEC_NT>(a.dct + a.dtotal + r0 + 4 * j, av[si]);
            ld4(a.dsk + wl * N + 4 * j, sk[si]);
            ld4<MFHE_DEC_NT>(a.dct + r0 + 4 * j, bv[si]);
        }
        // ring product per row (the shuffle ring_mul_row: ring_mul_row64_lds measured slower here, 198 vs 183 us)
#pragma unroll
        for (int si = 0; si < MFHE_DEC_SUBS; ++si) {
            const int st = sb + si;
            double x[4], sv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] = ArithF64::from_u64(av[si][e]);
                sv[e] = centred_f(sk[si][e], rl.qf);
            }
            ring_mul_row<LOGN>(x, sv, j, rar, tw, itw, ninv);
            double v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint64_t sum = bv[si][e] + rar.canon(x[e]);
                v[e] = ar.reduce(ArithF64::from_u64(sum >= rl.q ? sum - rl.q : sum));
            }
            double* row = bt + (st * 16 + rs) * RS + 4 * j;
            *(double2*)row = make_double2(v[0], v[1]);
            *(double2*)(row + 2) = make_double2(v[2], v[3]);
        }
        }
        __syncthreads();
        const int k0 = kc * 32 + hf * 16;
        double v[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) v[kk] = bt[(wv * 16 + kk) * RS + lane];   // b = k0 + kk + 1 of a = a' + 1
        ifold_chunk_sums(ar, v, x1, x2, zp, k0, s0, s1, s2);
        uint32_t pk[D][4];
        {
            uint64_t yb[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) yb[kk] = balanced_bytes<D>(v[kk]);
            pack_planes<D, 16>(yb, pk);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            if (i >= nd) break;
            int8_t* o = a.Bdig + (((uint64_t)l * D + i) * (FK / 32) + kc) * (uint64_t)Ppad * 64 + (uint64_t)p * 64 + wv * 16;
            const uint32_t* w = pk[i];
            *(v4i*)o = v4i{(int)(w[0] ^ 0x80808080u), (int)(w[1] ^ 0x80808080u), (int)(w[2] ^ 0x80808080u),
                           (int)(w[3] ^ 0x80808080u)};
        }
        __syncthreads();   // the next panel's ring stage rewrites bt
    }
    // column sums: (a', hf) are the four waves
    bt[(0 * 4 + wv) * 64 + lane] = s0;
    bt[(1 * 4 + wv) * 64 + lane] = s1;
    bt[(2 * 4 + wv) * 64 + lane] = s2;
    __syncthreads();
    if (gridDim.z > 1) {
        // a share of the panels: this block's sums per (column, a') to the partials, finished by dec_colsum_kernel
        if (wv >= 2) return;
        double* o = a.dpart + (((uint64_t)blockIdx.z * L + l) * Ppad + p) * 6 + wv * 3;
#pragma unroll
        for (int tt = 0; tt < 3; ++tt)
            o[tt] = ar.reduce(bt[(tt * 4 + 2 * wv) * 64 + lane] + bt[(tt * 4 + 2 * wv + 1) * 64 + lane]);
        return;
    }
    if (wv != 0) return;
    double e1[3], e2[3];   // a = 1 (a' = 0), a = 2 (a' = 1)
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
        e1[tt] = ar.reduce(bt[(tt * 4 + 0) * 64 + lane] + bt[(tt * 4 + 1) * 64 + lane]);
        e2[tt] = ar.reduce(bt[(tt * 4 + 2) * 64 + lane] + bt[(tt * 4 + 3) * 64 + lane]);
    }
    ifold_finish(a, ar, fo, e1, e2, l, Ppad, p);
}
template <int D>
__global__ __launch_bounds__(256, MFHE_DEC_WG_CU) void mfma_digitize_ifold_dec_kernel(ModGemmArgs a, uint32_t Ppad, PlaneCounts pc) {
    ifold_dec_impl<D>(a, Ppad, pc, (int)blockIdx.y, (int)gridDim.y);
}
// two components in one grid (he.hip decrypt_and_decode: re and im): blockIdx.y in [0, 2 L), the upper half is b
template <int D>
__global__ __launch_bounds__(256, MFHE_DEC_WG_CU) void mfma_digitize_ifold_dec_pair_kernel(ModGemmArgs a, ModGemmArgs b,
                                                                                         uint32_t Ppad, PlaneCounts pc) {
    const int L = (int)gridDim.y / 2, y = (int)blockIdx.y;
    const bool hi = y >= L;
    ifold_dec_impl<D>(hi ? b : a, Ppad, pc, hi ? y - L : y, L);
}

// the column sums of a split decrypt-fused digitize (gridDim.z = G shares of the panels): one thread per (column, limb)
__device__ __forceinline__ void dec_colsum_impl(const ModGemmArgs& a, uint32_t Ppad, int G, const int l, const int L) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Ppad) return;
    typedef const __attribute__((address_space(4))) double* cdp_t;
    const cdp_t fo = (cdp_t)(a.ifold + (uint64_t)l * 16);
    LimbConst lc;
    lc.qf = fo[0];
    lc.qinv = fo[1];
    const ArithF64 ar(lc);
    double e[6] = {0, 0, 0, 0, 0, 0};
    for (int g = 0; g < G; ++g) {   // |partial| <= q / 2: 8 terms stay exact, so reduce after every 8
        const double* o = a.dpart + (((uint64_t)g * L + l) * Ppad + p) * 6;
#pragma unroll
        for (int t = 0; t < 6; ++t) e[t] += o[t];
        if ((g & 7) == 7)
#pragma unroll
            for (int t = 0; t < 6; ++t) e[t] = ar.reduce(e[t]);
    }
    double e1[3], e2[3];
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
        e1[tt] = ar.reduce(e[tt]);
        e2[tt] = ar.reduce(e[3 + tt]);
    }
    ifold_finish(a, ar, fo, e1, e2, l, Ppad, p);
}
__global__ __launch_bounds__(256) void dec_colsum_kernel(ModGemmArgs a, uint32_t Ppad, int G) {
    dec_colsum_impl(a, Ppad, G, (int)blockIdx.y, (int)gridDim.y);
}
__global__ __launch_bounds__(256) void dec_colsum_pair_kernel(ModGemmArgs a, ModGemmArgs b, uint32_t Ppad, int G) {
    const int L = (int)gridDim.y / 2, y = (int)blockIdx.y;
    const bool hi = y >= L;
    dec_colsum_impl(hi ? b : a, Ppad, G, hi ? y - L : y, L);
}

}  // namespace mfhe

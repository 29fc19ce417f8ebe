// wcrt_mfma.hpp -- the i8 MFMA GEMM kernels of the W-CRT over the digit planes of wcrt_digitize.hpp (direct,
// LDS-staged, ring, ring56, pair, small-operand) and their epilogue.  Included by wcrt_gemm.hip only.
#pragma once
#include "wcrt_digitize.hpp"

namespace mfhe {

// C = sum_s acc_s * 256^s mod q for the 32 x 32 wave tile at (m0, p0) of limb l (lane = (r, h)).
// MODE 1 (factored forward): column p0 + r is (a', p) = divmod(., Ppad), output row a' * 256 + row, plus d0.
// MODE 2 (factored inverse): column p0 + r is 2 p + a', row r2 - 1; lanes r, r ^ 1 hold a' = 0, 1 of one column
// and trade their lam products, then write f_r2 (a' = 0) and f_(r2+257) (a' = 1, r2 <= 254).
// lanes l <-> l ^ 1 (DPP quad_perm [1, 0, 3, 2]: a VALU move, no LDS crossbar)
__device__ __forceinline__ double swap_pair(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true),
                            __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true));
}

// MODE 2: this lane's column's (c0, c1), loaded before the K loop so the epilogue does not wait for them
struct InvCC {
    double c0 = 0.0, c1 = 0.0;
};
template <int MODE>
__device__ __forceinline__ InvCC inv_cc(const ModGemmArgs& a, int l, uint32_t p0, int r, uint32_t Ppad) {
    InvCC c;
    if constexpr (MODE == 2) {
        const uint32_t p = (p0 + r) >> 1;
        const double* src = a.cc + ((uint64_t)l * Ppad + (p < a.P ? p : 0)) * 2;
        c.c0 = src[0];
        c.c1 = src[1];
    }
    return c;
}

template <int D, int MODE = 0>
__device__ __forceinline__ void mfma_epilogue(const ModGemmArgs& a, const v16i (&acc)[2 * D - 1], int l, int m0,
                                              uint32_t p0, int r, int h, uint32_t Ppad = 0, InvCC cc = InvCC{}) {
    constexpr int NS = 2 * D - 1;
    constexpr bool FAC = MODE != 0;
    uint64_t* Cl = a.C + (uint64_t)l * a.cL;
    if constexpr (MODE == 2) {
        typedef const __attribute__((address_space(4))) double* cdp_t;
        const cdp_t ep = (cdp_t)(a.epi + (uint64_t)l * 8);
        const cdp_t fo = (cdp_t)(a.ifold + (uint64_t)l * 16);
        LimbConst lc;
        lc.qf = ep[0];
        lc.qinv = ep[1];
        const ArithF64 ar(lc);
        const double c32[3] = {ep[2], ep[3], ep[4]};
        const uint32_t colf = p0 + r;
        const int ap = colf & 1;
        const uint32_t p = colf >> 1;
        const bool live = p < a.P;   // the same for both lanes of a pair
        // this lane's output takes lam_own (lam1 for a' = 0, lam2 for a' = 1) of its own E and the partner's share
        // lam_oth; both rotated once by r2 mod 3 of the lane's first row, so row reg uses index (reg's offset) mod 3
        const int r2b = m0 + 4 * h + 1;   // r2 of reg 0; reg adds (reg & 3) + 8 (reg >> 2)
        const int tb = r2b % 3;
        double own[3], oth[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = tb + k >= 3 ? tb + k - 3 : tb + k;
            const double l1 = t == 0 ? (ap ? fo[5] : fo[2]) : (t == 1 ? (ap ? fo[6] : fo[3]) : (ap ? fo[7] : fo[4]));
            const double l2 = t == 0 ? (ap ? fo[11] : fo[8]) : (t == 1 ? (ap ? fo[12] : fo[9]) : (ap ? fo[13] : fo[10]));
            own[k] = ap ? l2 : l1;
            oth[k] = ap ? l1 : l2;
        }
        const double c0 = cc.c0, c1 = cc.c1;
        uint64_t* Cp = Cl + (uint64_t)(p >> a.log_n) * a.scY + (p & ((1u << a.log_n) - 1));
        // the packed Phi rows of this wave tile's 32 rows r2 = m0 + 1 .. m0 + 32 (bytes m0 .. m0 + 31) by scalar loads
        typedef const __attribute__((address_space(4))) uint32_t* cu32_t;
        const cu32_t pw = (cu32_t)(a.phi + m0);
        uint32_t win[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) win[i] = pw[i];
        const int sh = ap ? 4 : 0;   // fields (phi_j, phi_(j-1)) of this lane's output row j
        constexpr int NZ = (NS + 1) / 2, NY = (NZ + 1) / 2;
        // every row computed first, the guarded stores after: a store under a branch inside the row loop splits it
        // into 16 serial blocks, each paying the full FP64 latency chain
        uint64_t outw[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int k = ((reg & 3) + 8 * (reg >> 2)) % 3;
            const uint32_t pb = ((h ? win[2 * (reg >> 2) + 1] : win[2 * (reg >> 2)]) >> (8 * (reg & 3) + sh)) & 15u;
            double zz[NZ];
#pragma unroll
            for (int t = 0; t < NZ; ++t)
                zz[t] = 2 * t + 1 < NS ? __fma_rn(256.0, (double)acc[2 * t + 1][reg], (double)acc[2 * t][reg])
                                       : (double)acc[2 * t][reg];
            double v = 0.0;
#pragma unroll
            for (int u = 0; u < NY; ++u) {
                const double y = 2 * u + 1 < NZ ? __fma_rn(65536.0, zz[2 * u + 1], zz[2 * u]) : zz[2 * u];
                v += u == 0 ? y : ar.mulmod(y, c32[u - 1]);
            }
            // |v| < 2^51 + 2 q, so v * lam / q < 2^51 with |lam| <= q / 2: mulmod needs no reduction of v first
            const double hv = ar.mulmod(v, own[k]) + swap_pair(ar.mulmod(v, oth[k]));
            // phi in {-1, 0, 1}: exact products, so one fma each
            const double fj = __fma_rn(-c0, (double)((int)(pb & 3u) - 1), __fma_rn(-c1, (double)((int)(pb >> 2) - 1), hv));
            outw[reg] = ar.canon(fj);
        }
        if (live) {
            const uint64_t jb = (uint64_t)(ap ? r2b + 257 : r2b);
            if (m0 + 32 <= 254) {   // wave-uniform: every row of this tile has an output in both halves
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) Cp[(jb + (reg & 3) + 8 * (reg >> 2)) * a.scM] = outw[reg];
            } else {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int r2 = r2b + (reg & 3) + 8 * (reg >> 2);
                    if (ap == 0 || r2 <= 254) Cp[(jb + (reg & 3) + 8 * (reg >> 2)) * a.scM] = outw[reg];
                }
            }
        }
        return;
    }
    if (FAC || a.epi) {
        // FP64 (every q < 2^50): |acc_s| < 2^26, so z_t = acc_2t + 256 acc_2t+1 (< 2^35) and
        // y_u = z_2u + 2^16 z_2u+1 (< 2^51) are exact doubles; C = y_0 + sum_u y_u (2^32u mod q), each
        // product an exact FP64 modmul with a centred constant (|y c / q| < 2^50), then one canonical
        // reduction -- about 25 FP64 ops per output instead of 2D-1 64-bit Shoup products.
        // per-limb constants by scalar loads (constant address space): no vmcnt wait, so the persistent ring's
        // DMAs in flight are not waited for here
        typedef const __attribute__((address_space(4))) double* cdp_t;
        const cdp_t ep = (cdp_t)(a.epi + (uint64_t)l * 8);
        LimbConst lc;
        lc.qf = ep[0];
        lc.qinv = ep[1];
        const ArithF64 ar(lc);
        const double c32[3] = {ep[2], ep[3], ep[4]};
        uint32_t colf = p0 + r;
        int rbase = 0;
        double add = 0.0;
        if (FAC) {
            const int ap = colf >= Ppad;
            colf -= ap * Ppad;
            if (colf >= a.P) return;
            rbase = ap * FK;
            add = ArithF64::from_u64(a.d0[((uint64_t)l * 2 + ap) * Ppad + colf]);
        }
        if (colf >= a.P) return;
        constexpr int NZ = (NS + 1) / 2, NY = (NZ + 1) / 2;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = rbase + m0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            double z[NZ];
#pragma unroll
            for (int t = 0; t < NZ; ++t)
                z[t] = 2 * t + 1 < NS ? __fma_rn(256.0, (double)acc[2 * t + 1][reg], (double)acc[2 * t][reg])
                                      : (double)acc[2 * t][reg];
            double v = add;
#pragma unroll
            for (int u = 0; u < NY; ++u) {
                const double y = 2 * u + 1 < NZ ? __fma_rn(65536.0, z[2 * u + 1], z[2 * u]) : z[2 * u];
                v += u == 0 ? y : ar.mulmod(y, c32[u - 1]);
            }
            const uint64_t o = (uint64_t)row * a.scM + (uint64_t)(colf >> a.log_n) * a.scY + (colf & ((1u << a.log_n) - 1));
            const uint64_t cv = ar.canon(v);
            Cl[o] = cv;
            if (a.C2) a.C2[(uint64_t)l * a.cL + o] = cv;
        }
        return;
    }
    if constexpr (FAC) return;   // factored mode always has the FP64 epilogue (launch_mod_gemm checks)
    typedef const __attribute__((address_space(4))) uint64_t* cup_t;
    const uint64_t q = ((cup_t)a.qmu)[2 * l], mu = ((cup_t)a.qmu)[2 * l + 1];
    // rtab rows are [L][2 a.D - 1][2] for the context's plane stride a.D: a limb run with fewer digits (NS < 2 a.D - 1)
    // must still step by the table's row length (r06: stepping by NS gave limbs >= 1 of a D = 7 run in a D = 8 context
    // another limb's constants, tests/test_wcrt_sizes_gpu.py at 55 bits)
    const cup_t rt = (cup_t)(a.rtab + (uint64_t)l * (2 * a.D - 1) * 2);
    uint64_t* C = Cl;
    const uint32_t col = p0 + r;
    if (col >= a.P) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = m0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        uint64_t sum = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int64_t v = acc[s][reg];
            const uint64_t x = v < 0 ? (uint64_t)(v + (int64_t)q) : (uint64_t)v;   // |v| < 2^26 < q
            uint64_t t = x * rt[2 * s] - __umul64hi(x, rt[2 * s + 1]) * q;        // Shoup: [0, 2q)
            sum += t;                                                              // < 2 NS q < 2^64
        }
        uint64_t red = sum - __umul64hi(sum, mu) * q;   // Barrett: [0, 2q)
        red = red >= q ? red - q : red;
        C[(uint64_t)row * a.scM + (uint64_t)(col >> a.log_n) * a.scY + (col & ((1u << a.log_n) - 1))] = red;
    }
}

template <int D>
__global__ __launch_bounds__(256, D <= 5 ? 2 : 1) void mod_gemm_mfma_kernel(ModGemmArgs a, uint32_t Ppad, int limb0) {
    constexpr int NS = 2 * D - 1;
    const int l = limb0 + blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 64 + (w & 1) * 32;
    const uint32_t p0 = blockIdx.x * 64 + (w >> 1) * 32;
    const int8_t* Al = a.Adig + (uint64_t)l * a.adL;
    const int8_t* Bl = a.Bdig + (uint64_t)l * a.D * Ppad * MK;   // planes beyond this limb's D are zero
    v16i acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = v16i{0};
    for (int kc = 0; kc < MK / 32; ++kc) {
        v4i av[D], bv[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            av[i] = *(const v4i*)(Al + (uint64_t)i * 512 * MK + ((uint64_t)kc * 512 + m0 + r) * 32 + 16 * h);
            bv[i] = *(const v4i*)(Bl + (uint64_t)i * Ppad * MK + ((uint64_t)kc * Ppad + p0 + r) * 32 + 16 * h);
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) acc[i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], acc[i + j], 0, 0, 0);
    }
    mfma_epilogue<D>(a, acc, l, m0, p0, r, h);
}

// LDS-staged variant (default).  Same digit planes, tile (64 x 64 outputs, four 32 x 32 wave tiles) and
// exact accumulation as mod_gemm_mfma_kernel, but each 64-deep K stage (two 32-k panels) of both operands
// goes global -> LDS once per workgroup by LDS-DMA (global_load_lds_dwordx4: no VGPR staging; the
// k-panel-major planes make each wave's 1 KiB destination lane-linear, as the DMA requires), double-
// buffered one stage ahead of the MFMAs that read it.  Waves 0-1 move A's planes, waves 2-3 B's.
// RAW order for the DMA'd bytes: issuing waves' s_waitcnt vmcnt(0), then the barrier, then the reads.
typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int D, int MODE>
__global__ __launch_bounds__(256, D <= 5 ? 2 : 1) void mod_gemm_mfma_lds_kernel(ModGemmArgs a, uint32_t Ppad, int limb0) {
    // MODE 1 / 2 (factored forward / inverse): M = K = 256 and 2 Ppad B columns; 0: M = K = 512 and Ppad columns
    constexpr bool FAC = MODE != 0;
    constexpr int KK = FAC ? FK : MK, AM = FAC ? FK : 512;
    const uint32_t Pcols = FAC ? 2 * Ppad : Ppad;
    constexpr int NS = 2 * D - 1;
    constexpr int KS = 64;                       // K per stage: two 32-k panels
    constexpr int PANEL = 64 * 32;               // 64 rows x 32 k of one digit plane (bytes)
    constexpr int PLANE = 2 * PANEL;             // one digit plane of one operand per stage
    constexpr int STAGE = 2 * D * PLANE;         // A planes then B planes
    __shared__ __attribute__((aligned(16))) int8_t lds[2 * STAGE];
    const int l = limb0 + blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int mb = blockIdx.y * 64, pb = blockIdx.x * 64;
    const int wm = (w & 1) * 32, wp = (w >> 1) * 32;
    // DMA slot li: bytes [16 li, 16 li + 16) of a 2 KiB panel image (row li / 2, k half li & 1)
    const bool ldA = t < 128;
    const int li = t & 127;
    const uint64_t rows = ldA ? AM : Pcols;                        // rows of the operand's planes
    const int8_t* src = (ldA ? a.Adig + (uint64_t)l * a.adL : a.Bdig + (uint64_t)l * a.D * Pcols * KK) +
                        (uint64_t)(ldA ? mb : pb) * 32 + li * 16;
    const uint64_t pstride = rows * KK, kstride = rows * 32;      // digit-plane / k-panel strides
    const int wbase = (ldA ? 0 : D * PLANE) + (li & ~63) * 16;     // this wave's LDS destination base
    auto issue = [&](int s, int buf) {
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
                __builtin_amdgcn_global_load_lds((const void*)(src + i * pstride + (uint64_t)(2 * s + pp) * kstride),
                                                 (lds_ptr_t)(lds + buf * STAGE + wbase + i * PLANE + pp * PANEL), 16,
                                                 0, 0);
    };
    const InvCC icc = inv_cc<MODE>(a, l, (uint32_t)(pb + wp), r, Ppad);
    v16i acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = v16i{0};
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < KK / KS; ++s) {
        const int buf = s & 1;
        if (s + 1 < KK / KS) issue(s + 1, buf ^ 1);   // buf ^ 1's last readers all passed the previous barrier
        const int8_t* st = lds + buf * STAGE;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            v4i bv[D];
#pragma unroll
            for (int j = 0; j < D; ++j)
                bv[j] = *(const v4i*)(st + (D + j) * PLANE + pp * PANEL + (wp + r) * 32 + 16 * h);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const v4i av = *(const v4i*)(st + i * PLANE + pp * PANEL + (wm + r) * 32 + 16 * h);
#pragma unroll
                for (int j = 0; j < D; ++j)
                    acc[i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv[j], acc[i + j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA into buf ^ 1 has landed
        __syncthreads();
    }
    mfma_epilogue<D, MODE>(a, acc, l, mb + wm, (uint32_t)(pb + wp), r, h, Ppad, icc);
}

// Ring variant (MFHE_OPT_WCRT_PIPE 2 / 3, and 0 = auto on the factored launch): the same tile, digit planes and
// epilogue, but the K loop runs over 32-k stages (one panel per digit plane per operand, 4 D KiB) held in an
// NSLOT-slot LDS ring: stage s + NSLOT - 1 is DMA'd while stage s is multiplied, so a stage's bytes have NSLOT - 1
// stage times to land instead of one, and the wait at the end of stage s is a counted vmcnt that leaves the later
// stages in flight (D DMA instructions per thread per stage; nothing else in the loop touches vector memory).  The
// barrier after it is a raw s_barrier (__syncthreads' fence would wait for the DMAs in flight).  Slot
// (s + NSLOT - 1) % NSLOT = (s - 1) % NSLOT was last read in stage s - 1, which every wave has left at that barrier.
// NSLOT = 4 at D = 5 (80 KiB, 2 workgroups per CU); 3 at D = 6 (72 KiB): with its registers held to 256 (launch
// bounds) the D = 6 limb (the reference's 44-bit q0) also runs 2 workgroups per CU -- r03 ran it at 96 KiB and 384
// VGPRs, one workgroup per CU and 0.22 MFMA busy (profiles/r03_gemm_sq_pmc.txt).
// AHEAD: the next A fragment's LDS read is issued before the current fragment's D MFMAs (sched_barrier-pinned),
// so its latency hides behind them instead of being waited for in front of them (D <= 5 only: at D >= 6 the
// extra fragment spills).
template <int D>
constexpr int ring_slots() { return D <= 5 ? 4 : 3; }
template <int D, int MODE>
constexpr int ring_lds_bytes() { return ring_slots<D>() * 2 * D * 64 * 32; }
template <int D, int MODE, bool AHEAD>
__device__ __forceinline__ void ring_tile(const ModGemmArgs& a, uint32_t Ppad, int l, int8_t* lds) {
    constexpr bool FAC = MODE != 0;
    constexpr int KK = FAC ? FK : MK, AM = FAC ? FK : 512;
    const uint32_t Pcols = FAC ? 2 * Ppad : Ppad;
    constexpr int NS = 2 * D - 1;
    constexpr int NST = KK / 32;                 // 32-k stages
    constexpr int PANEL = 64 * 32;               // 64 rows x 32 k of one digit plane (bytes)
    constexpr int STAGE = 2 * D * PANEL;         // A planes then B planes
    constexpr int NSLOT = ring_slots<D>(), LEAD = NSLOT - 1;
    static_assert(NST >= NSLOT, "ring prologue assumes at least NSLOT stages");
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int mb = blockIdx.y * 64, pb = blockIdx.x * 64;
    const int wm = (w & 1) * 32, wp = (w >> 1) * 32;
    const bool ldA = t < 128;
    const int li = t & 127;
    const uint64_t rows = ldA ? AM : Pcols;
    const int8_t* src = (ldA ? a.Adig + (uint64_t)l * a.adL : a.Bdig + (uint64_t)l * a.D * Pcols * KK) +
                        (uint64_t)(ldA ? mb : pb) * 32 + li * 16;
    const uint64_t pstride = rows * KK, kstride = rows * 32;
    const int wbase = (ldA ? 0 : D * PANEL) + (li & ~63) * 16;
    auto issue = [&](int s) {
        int8_t* dst = lds + (s % NSLOT) * STAGE + wbase;
#pragma unroll
        for (int i = 0; i < D; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(src + i * pstride + (uint64_t)s * kstride),
                                             (lds_ptr_t)(dst + i * PANEL), 16, 0, 0);
    };
    auto barrier = []() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    const InvCC icc = inv_cc<MODE>(a, l, (uint32_t)(pb + wp), r, Ppad);   // older than every DMA: the counted waits cover it
    v16i acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = v16i{0};
#pragma unroll
    for (int s = 0; s < LEAD; ++s) issue(s);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LEAD - 1) * D) : "memory");   // stage 0 landed (1 .. LEAD - 1 in flight)
    barrier();
#pragma unroll
    for (int s = 0; s < NST; ++s) {
        if (s + LEAD < NST) issue(s + LEAD);
        const int8_t* st = lds + (s % NSLOT) * STAGE;
        v4i bv[D];
#pragma unroll
        for (int j = 0; j < D; ++j) bv[j] = *(const v4i*)(st + (D + j) * PANEL + (wp + r) * 32 + 16 * h);
        if constexpr (AHEAD) {
            v4i an = *(const v4i*)(st + (wm + r) * 32 + 16 * h);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const v4i av = an;
                if (i + 1 < D) an = *(const v4i*)(st + (i + 1) * PANEL + (wm + r) * 32 + 16 * h);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < D; ++j)
                    acc[i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv[j], acc[i + j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const v4i av = *(const v4i*)(st + i * PANEL + (wm + r) * 32 + 16 * h);
#pragma unroll
                for (int j = 0; j < D; ++j)
                    acc[i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv[j], acc[i + j], 0, 0, 0);
            }
        }
        // stage s + 1 landed for this wave: newer are the DMAs of the stages after it that were issued
        if (s + 1 < NST) {
            const int newer = (s + LEAD < NST ? s + LEAD : NST - 1) - (s + 1);
            if (newer == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * D) : "memory");
            else if (newer == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            barrier();
        }
    }
    mfma_epilogue<D, MODE>(a, acc, l, mb + wm, (uint32_t)(pb + wp), r, h, Ppad, icc);
}

template <int D, int MODE, bool AHEAD>
__global__ __launch_bounds__(256, D <= 5 || (D == 6 && MODE != 0) ? 2 : 1)   // dense D = 6 spills at 256 VGPRs
void mod_gemm_mfma_ring_kernel(ModGemmArgs a, uint32_t Ppad, int limb0) {
    __shared__ __attribute__((aligned(16))) int8_t lds[ring_lds_bytes<D, MODE>()];
    ring_tile<D, MODE, AHEAD>(a, Ppad, limb0 + (int)blockIdx.z, lds);
}

// r04: the factored launches' limbs at D = 5 and D = 6 in one grid (the reference's 44-bit q0 needs six
// digits and ran as its own one-limb launch at 0.22 MFMA busy).  The digit count is per limb (bit l of d6, workgroup-
// uniform: blockIdx.z), the two bodies share one LDS ring (max of 80 KiB at D = 5 and 72 KiB at D = 6) and one
// register budget (<= 256: 2 workgroups per CU for both); limb 0's tiles dispatch first (z slowest), so the heavier
// tiles do not form the tail.
template <int MODE>
__global__ __launch_bounds__(256, 2) void mod_gemm_mfma_ring56_kernel(ModGemmArgs a, uint32_t Ppad, int limb0, uint64_t d6) {
    constexpr int B5 = ring_lds_bytes<5, MODE>(), B6 = ring_lds_bytes<6, MODE>();
    __shared__ __attribute__((aligned(16))) int8_t lds[B5 > B6 ? B5 : B6];
    const int l = limb0 + (int)blockIdx.z;
    if ((d6 >> blockIdx.z) & 1) ring_tile<6, MODE, false>(a, Ppad, l, lds);
    else ring_tile<5, MODE, false>(a, Ppad, l, lds);
}
// two components in one grid (blockIdx.z in [0, 2 L), the upper half is b): encode's / decode's re and im, whose
// tiles then share the GPU without a stream fork (he.hip MFHE_OPT_HE_STREAMS 2)
template <int MODE>
__global__ __launch_bounds__(256, 2) void mod_gemm_mfma_ring56_pair_kernel(ModGemmArgs a, ModGemmArgs b, uint32_t Ppad,
                                                                           uint64_t d6) {
    constexpr int B5 = ring_lds_bytes<5, MODE>(), B6 = ring_lds_bytes<6, MODE>();
    __shared__ __attribute__((aligned(16))) int8_t lds[B5 > B6 ? B5 : B6];
    const int L = (int)gridDim.z / 2, z = (int)blockIdx.z;
    const bool hi = z >= L;
    const int l = hi ? z - L : z;
    const ModGemmArgs& x = hi ? b : a;
    if ((d6 >> l) & 1) ring_tile<6, MODE, false>(x, Ppad, l, lds);
    else ring_tile<5, MODE, false>(x, Ppad, l, lds);
}

// ---- the W-CRT forward of a small signed operand (r06): the encrypt's Gaussian noise ----
// The noise e is one small integer per (w, pos), the same in every limb: the reference's Box-Muller draw
// (HE.cu:581-627) is 3.2 sqrt(-2 ln u1) cos(2 pi u2) with u1 >= 2^-53, so |e| <= 3.2 sqrt(106 ln 2) < 27.5 and e is its
// own balanced base-256 digit.  The dense product V_l e then needs D_l x 1 digit pairs per MAC (acc_i = sum_k v_i e,
// shift i only) against the factored forward's D_l x D_l at half the MACs: 2 D_l / D_l^2 = 0.4 of its MFMAs at
// D_l = 5, with no digitize kernel (gaussian_i8_kernel writes the one plane, shared by every limb, in the GEMM's
// k-panel-major layout) and no per-limb residue array.
// Tile 64 rows x 64 NC columns, four waves as 2 x 2 (each 32 rows x 32 NC columns, NC accumulator sets per digit);
// 64-k LDS-DMA stages, double-buffered, per stage every thread issues DA + NC DMAs (A's DA planes, then B's NC).
// A's DA planes are the bulk of a stage, so NC = 2 halves the A bytes per MAC (r06 counters at NC = 1: MFMA busy
// 0.21, waits 0.54 of wave cycles; a third stage buffer was slower).  FP64 epilogue (every q < 2^50):
// |acc_i| <= 512 * 128 * 28 < 2^21, z / y as in mfma_epilogue.
template <int DA, int NC>
__device__ __forceinline__ void smallb_mma(const ModGemmArgs& a, const int8_t* __restrict__ b8, uint32_t Ppad, int l,
                                           int mb, int pb, int8_t* lds, v16i (&acc)[NC][DA]) {
    constexpr int KS = 64, PANEL = 64 * 32, PLANE = 2 * PANEL;   // one stage: two 32-k panels per 64-row plane
    constexpr int STAGE = (DA + NC) * PLANE;                        // A's DA planes, then B's NC (64 columns each)
    constexpr int NS = MK / KS;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = (w & 1) * 32, wp = (w >> 1) * 32 * NC;          // this wave's rows / first column in the tile
    const int pp = t >> 7, li = t & 127;                            // this thread's k-panel of a stage and 16-B chunk
    const int8_t* srcA = a.Adig + (uint64_t)l * a.adL + (uint64_t)mb * 32 + li * 16;
    const int8_t* srcB = b8 + (uint64_t)pb * 32 + li * 16;
    constexpr uint64_t kstrA = 512ull * 32, plA = 512ull * MK;      // A: k-panel / digit-plane strides
    const uint64_t kstrB = (uint64_t)Ppad * 32;
    const int wdst = pp * PANEL + ((li & ~63) * 16);                // this wave's LDS destination inside a plane
    auto issue = [&](int s, int buf) {
        int8_t* st = lds + buf * STAGE + wdst;
        const uint64_t kp = (uint64_t)(2 * s + pp);
#pragma unroll
        for (int i = 0; i < DA; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(srcA + i * plA + kp * kstrA), (lds_ptr_t)(st + i * PLANE), 16,
                                             0, 0);
#pragma unroll
        for (int c = 0; c < NC; ++c)
            __builtin_amdgcn_global_load_lds((const void*)(srcB + c * 64 * 32 + kp * kstrB),
                                             (lds_ptr_t)(st + (DA + c) * PLANE), 16, 0, 0);
    };
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < DA; ++i) acc[c][i] = v16i{0};
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
        const int buf = s & 1;
        if (s + 1 < NS) issue(s + 1, buf ^ 1);   // buf ^ 1's last readers all passed the previous barrier
        const int8_t* st = lds + buf * STAGE;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            v4i bv[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int tc = wp + 32 * c;   // tile column of this 32-column block: 64-column plane tc / 64
                bv[c] = *(const v4i*)(st + (DA + tc / 64) * PLANE + q * PANEL + (tc % 64 + r) * 32 + 16 * h);
            }
#pragma unroll
            for (int i = 0; i < DA; ++i) {
                const v4i av = *(const v4i*)(st + i * PLANE + q * PANEL + (wm + r) * 32 + 16 * h);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c][i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv[c], acc[c][i], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMAs into buf ^ 1 have landed
        __syncthreads();
    }
}

// C = sum_i acc_i 256^i mod q, canonical, for accumulator register `reg` (FP64: z / y as in mfma_epilogue)
template <int DA>
__device__ __forceinline__ uint64_t smallb_value(const ArithF64& ar, const double (&c32)[3], const v16i (&acc)[DA],
                                                 int reg) {
    constexpr int NZ = (DA + 1) / 2, NY = (NZ + 1) / 2;
    double z[NZ];
#pragma unroll
    for (int u = 0; u < NZ; ++u)
        z[u] = 2 * u + 1 < DA ? __fma_rn(256.0, (double)acc[2 * u + 1][reg], (double)acc[2 * u][reg])
                              : (double)acc[2 * u][reg];
    double v = 0.0;
#pragma unroll
    for (int u = 0; u < NY; ++u) {
        const double y = 2 * u + 1 < NZ ? __fma_rn(65536.0, z[2 * u + 1], z[2 * u]) : z[2 * u];
        v += u == 0 ? y : ar.mulmod(y, c32[u - 1]);
    }
    return ar.canon(v);
}

template <int DA, int NC>
__global__ __launch_bounds__(256, 2) void mod_gemm_mfma_smallb_kernel(ModGemmArgs a, const int8_t* __restrict__ b8,
                                                                      uint32_t Ppad, int limb0) {
    __shared__ __attribute__((aligned(16))) int8_t lds[2 * (DA + NC) * 64 * 64];
    const int l = limb0 + blockIdx.z;
    const int mb = blockIdx.y * 64, pb = blockIdx.x * 64 * NC;
    v16i acc[NC][DA];
    smallb_mma<DA, NC>(a, b8, Ppad, l, mb, pb, lds, acc);
    typedef const __attribute__((address_space(4))) double* cdp_t;
    const cdp_t ep = (cdp_t)(a.epi + (uint64_t)l * 8);
    LimbConst lc;
    lc.qf = ep[0];
    lc.qinv = ep[1];
    const ArithF64 ar(lc);
    const double c32[3] = {ep[2], ep[3], ep[4]};
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int wm = (w & 1) * 32, wp = (w >> 1) * 32 * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t col = pb + wp + 32 * c + r;
        if (col >= a.P) continue;
        uint64_t* Cl = a.C + (uint64_t)l * a.cL + (uint64_t)(col >> a.log_n) * a.scY + (col & ((1u << a.log_n) - 1));
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            Cl[(uint64_t)(mb + wm + (reg & 3) + 8 * (reg >> 2) + 4 * h) * a.scM] = smallb_value<DA>(ar, c32, acc[c], reg);
    }
}

}  // namespace mfhe

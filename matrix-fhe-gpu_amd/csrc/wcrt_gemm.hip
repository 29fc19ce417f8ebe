// wcrt_gemm.hip -- see wcrt_gemm.hpp: the VALU kernel and the host launchers; the i8 MFMA kernels are in
// wcrt_digitize.hpp and wcrt_mfma.hpp.
#include "wcrt_gemm.hpp"

#include <algorithm>
#include <type_traits>

#include "gemm_tile.hpp"
#include "mfhe_ctx.hpp"
#include "mod128.hpp"
#include "wcrt_digitize.hpp"
#include "wcrt_mfma.hpp"

namespace mfhe {

__global__ __launch_bounds__(NTH) void mod_gemm_kernel(ModGemmArgs a) {
    __shared__ uint64_t As[TM][TK + 1];
    __shared__ uint64_t Bs[TK][TP];
    const int l = blockIdx.z;
    const int m0 = blockIdx.y * TM;
    const uint32_t p0 = blockIdx.x * TP;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint64_t* A = a.A + (uint64_t)l * a.aL;
    const uint64_t* B = a.B + (uint64_t)l * a.bL;
    uint64_t acc_lo[4][4], acc_hi[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_lo[i][j] = acc_hi[i][j] = 0;

    for (int k0 = 0; k0 < a.K; k0 += TK) {
#pragma unroll
        for (int e = 0; e < (TM * TK) / NTH; ++e) {   // A tile 64 x 16
            const int idx = t + e * NTH, r = idx / TK, c = idx % TK;
            const int m = m0 + r, k = k0 + c;
            As[r][c] = (m < a.M && k < a.K) ? A[(uint64_t)m * a.K + k] : 0;
        }
#pragma unroll
        for (int e = 0; e < (TK * TP) / NTH; ++e) {   // B tile 16 x 64 (coalesced along p)
            const int idx = t + e * NTH, r = idx / TP, c = idx % TP;
            const int k = k0 + r;
            const uint32_t p = p0 + c;
            Bs[r][c] = (k < a.K && p < a.P) ? B[b_off(k, p, a.sbK, a.sbY, a.log_n)] : 0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < TK; ++k) {
            uint64_t av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[ty + 16 * i][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[k][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u128 pr = (u128)av[i] * bv[j];
                    const uint64_t lo = (uint64_t)pr, hi = (uint64_t)(pr >> 64);
                    acc_lo[i][j] += lo;
                    acc_hi[i][j] += hi + (acc_lo[i][j] < lo);
                }
        }
        __syncthreads();
    }
    const uint64_t q = a.qmu[2 * l], mu = a.qmu[2 * l + 1], r64 = a.r64[l];
    uint64_t* C = a.C + (uint64_t)l * a.cL;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty + 16 * i;
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p = p0 + tx + 16 * j;
            if (p >= a.P) continue;
            C[b_off(m, p, a.scM, a.scY, a.log_n)] = mod_u128_fold(acc_hi[i][j], acc_lo[i][j], q, mu, r64);
        }
    }
}

// ---------------- host dispatch of the i8 MFMA path ----------------

static uint32_t pad64(uint32_t P) { return (P + 63) / 64 * 64; }

// digits the GEMM takes for limb l: its own count but at least 5 (the smallest instantiated D); a.D for every limb
// without a per-limb table
static int limb_digits(const ModGemmArgs& a, int l) { return a.limbD ? std::max(a.limbD[l], 5) : a.D; }

static PlaneCounts plane_counts(const ModGemmArgs& a, int L) {
    PlaneCounts pc;
    for (int l = 0; l < 64; ++l) pc.n[l] = (uint8_t)(l < L ? limb_digits(a, l) : a.D);
    return pc;
}

// f(D) with D = std::integral_constant<int, d> for the run-time digit count d in [LO, HI] (the kernels' D is a
// template parameter: D() names it), then the launch check under `what`.  The factored and small-operand kernels are
// instantiated for 5..6 digits, the dense ones for 5..8.
template <int LO, int HI, class F>
static int dispatch_digits(int d, const char* what, F&& f) {
    if constexpr (LO > HI) {
        return set_error(MFHE_EINVAL, "mod_gemm: MFMA digit count must be 5..8");
    } else {
        if (d != LO) return dispatch_digits<LO + 1, HI>(d, what, f);
        f(std::integral_constant<int, LO>{});
        MFHE_CHECK_LAUNCH(what);
        return MFHE_OK;
    }
}

// f(D, l0, l1) (D as dispatch_digits') for every run [l0, l1) of consecutive limbs that need the same number of
// digits: one GEMM launch per run, each checked under `what`
template <int LO, int HI, class F>
static int for_digit_runs(const ModGemmArgs& a, int L, const char* what, F&& f) {
    for (int l0 = 0, l1; l0 < L; l0 = l1) {
        const int d = limb_digits(a, l0);
        for (l1 = l0 + 1; l1 < L && limb_digits(a, l1) == d;) ++l1;
        if (int rc = dispatch_digits<LO, HI>(d, what, [&](auto D) { f(D, l0, l1); })) return rc;
    }
    return MFHE_OK;
}

// The Bdig workspace of L limbs at plane stride D over Ppad columns:
//   the digit planes                                              L D Ppad 512 bytes
//   the factored forward's d0 [L][2][Ppad] u64, which are also
//   the factored inverse's cc [L][Ppad][2] (c0, c1) doubles       L 2 Ppad 8 bytes
//   the split decrypt-fused digitize's column partials dpart
//   [MFHE_DEC_SPLIT][L][Ppad][6] doubles                           MFHE_DEC_SPLIT L Ppad 6 8 bytes
struct BdigLayout {
    int8_t* base;
    size_t planes, cols, parts;   // bytes of the three regions
    BdigLayout(int8_t* Bdig, int L, int D, uint64_t Ppad)
        : base(Bdig), planes((size_t)L * D * Ppad * MK), cols((size_t)L * 2 * Ppad * 8),
          parts((size_t)MFHE_DEC_SPLIT * L * Ppad * 6 * 8) {}
    uint64_t* d0() const { return (uint64_t*)(base + planes); }
    double* cc() const { return (double*)(base + planes); }
    double* dpart() const { return (double*)(base + planes + cols); }
    size_t bytes() const { return planes + cols + parts; }
};

size_t mod_gemm_mfma_ws(uint32_t P, int L, int D) {
    return BdigLayout(nullptr, L, D, ((uint64_t)P + 63) / 64 * 64).bytes();
}

void balanced_digits(uint64_t x, int D, int8_t* out) {
    for (int i = 0; i < D; ++i) {
        int v = (int)(x & 255);
        x >>= 8;
        if (v >= 128) {
            v -= 256;
            ++x;
        }
        out[i] = (int8_t)v;
    }
}

// The ring kernel's waits are counted (vmcnt(D) / vmcnt(2D): the DMAs of the stages still in flight).  A build in
// which it spills would add scratch traffic to the counted ops; checked once per instantiation from the code
// object's metadata, and such a build runs the two-stage LDS kernel (vmcnt(0) waits) instead.  AHEAD is D <= 5
// only: at D = 6 its extra A fragment spills (tests/test_isa.py pins the shipped instantiations' instruction mix).
static bool spill_free(const void* kernel) {
    hipFuncAttributes fa{};
    return hipFuncGetAttributes(&fa, kernel) == hipSuccess && fa.localSizeBytes == 0;
}
template <int D, int MODE, bool AHEAD>
static bool ring_usable() {
    static const bool ok = spill_free(reinterpret_cast<const void*>(mod_gemm_mfma_ring_kernel<D, MODE, AHEAD>));
    return ok;
}
template <int MODE>
static bool ring56_usable() {
    static const bool ok = spill_free(reinterpret_cast<const void*>(mod_gemm_mfma_ring56_kernel<MODE>));
    return ok;
}
template <int MODE>
static bool ring56_pair_usable() {
    static const bool ok = spill_free(reinterpret_cast<const void*>(mod_gemm_mfma_ring56_pair_kernel<MODE>));
    return ok;
}

// what the ring56 kernels need: pipe 0 (auto), every limb at D = 5 or 6 (bit l of d6), at most 64 limbs
static bool ring56_all(const ModGemmArgs& f, int L, uint64_t& d6) {
    d6 = 0;
    if (f.pipe != 0 || L > 64) return false;
    for (int l = 0; l < L; ++l) {
        const int d = limb_digits(f, l);
        if (d != 5 && d != 6) return false;
        if (d == 6) d6 |= 1ull << l;
    }
    return true;
}

// pipe: 1 = two-stage LDS kernel; 3 = ring + one-ahead A read (D <= 5); anything else = ring
template <int D, int MODE>
static void launch_staged(int pipe, dim3 grid, hipStream_t s, const ModGemmArgs& f, uint32_t Ppad, int l0) {
    if constexpr (D <= 5) {
        if (pipe == 3 && ring_usable<D, MODE, true>()) {
            hipLaunchKernelGGL((mod_gemm_mfma_ring_kernel<D, MODE, true>), grid, dim3(256), 0, s, f, Ppad, l0);
            return;
        }
    }
    if (pipe != 1 && ring_usable<D, MODE, false>()) {
        hipLaunchKernelGGL((mod_gemm_mfma_ring_kernel<D, MODE, false>), grid, dim3(256), 0, s, f, Ppad, l0);
        return;
    }
    hipLaunchKernelGGL((mod_gemm_mfma_lds_kernel<D, MODE>), grid, dim3(256), 0, s, f, Ppad, l0);
}

// the factored 256 x 256 GEMM over 2 Ppad columns (MODE 1 forward, 2 inverse).  Pipe 0 (auto): every limb at D = 5
// or 6 in one ring56 grid; otherwise (another pipe, other digit counts, more than 64 limbs, a spilling build) one
// launch per run of equal digit counts -- pipe 0 and 2 the ring (K = 256: four 64-k stages leave the fill exposed)
template <int MODE>
static int launch_factored_gemm(const ModGemmArgs& f, int L, uint32_t Ppad, hipStream_t s) {
    uint64_t d6 = 0;
    if (ring56_all(f, L, d6) && ring56_usable<MODE>()) {
        hipLaunchKernelGGL((mod_gemm_mfma_ring56_kernel<MODE>), dim3(2 * Ppad / 64, FK / 64, L), dim3(256), 0, s, f, Ppad,
                           0, d6);
        MFHE_CHECK_LAUNCH(MODE == 1 ? "mod_gemm_mfma_ring56_kernel (factored)"
                                    : "mod_gemm_mfma_ring56_kernel (factored inverse)");
        return MFHE_OK;
    }
    const char* what = MODE == 1 ? "mod_gemm_mfma_lds_kernel (factored)" : "mod_gemm_mfma kernel (factored inverse)";
    return for_digit_runs<5, 6>(f, L, what, [&](auto D, int l0, int l1) {
        launch_staged<D(), MODE>(f.pipe, dim3(2 * Ppad / 64, FK / 64, l1 - l0), s, f, Ppad, l0);
    });
}

// b8: [512 / 32][Ppad][32] with Ppad = P rounded up to 64; the two-block tile (NC = 2) needs Ppad % 128 == 0 so that
// no stage reads past the plane
int launch_mod_gemm_smallb(const ModGemmArgs& a, const int8_t* b8, int L, hipStream_t s) {
    if (!a.Adig || !a.epi || a.M != 512 || a.K != MK || a.fold || a.ifold || a.D < 5 || a.D > 6 || a.adL == 0)
        return set_error(MFHE_EINVAL, "mod_gemm_smallb: needs the dense per-limb V planes (5 or 6 digits) and the FP64 epilogue");
    const uint32_t Ppad = pad64(a.P);
    const int nc = Ppad % 128 == 0 ? 2 : 1;
    return for_digit_runs<5, 6>(a, L, "mod_gemm_mfma_smallb_kernel", [&](auto D, int l0, int l1) {
        const dim3 grid(Ppad / (64 * nc), 512 / 64, l1 - l0);
        if (nc == 2) hipLaunchKernelGGL((mod_gemm_mfma_smallb_kernel<D(), 2>), grid, dim3(256), 0, s, a, b8, Ppad, l0);
        else hipLaunchKernelGGL((mod_gemm_mfma_smallb_kernel<D(), 1>), grid, dim3(256), 0, s, a, b8, Ppad, l0);
    });
}

static FoldSrc fold_src(const ModGemmArgs& a) {
    return FoldSrc{a.qf, a.qf_row, a.qf_step, a.delta, a.qmu, a.lbase, a.Ltot};
}
// the factored forward's digitize of a.B (a.qsrc 0) or a fused source (1..3; the grid then runs the limbs fastest)
// into a.Bdig / d0
static int launch_fold(const ModGemmArgs& a, uint64_t* d0, int L, uint32_t Ppad, const PlaneCounts& pc, hipStream_t s) {
    if (a.qsrc < 0 || a.qsrc > 3) return set_error(MFHE_EINVAL, "mod_gemm: unknown digitize source");
    const FoldSrc fs = a.qsrc ? fold_src(a) : FoldSrc{};
    const uint32_t gp = (Ppad + 127) / 128, gk = FK / 32;
    const dim3 grid = a.qsrc ? dim3(L, gp, gk) : dim3(gp, gk, L);
    return dispatch_digits<5, 6>(a.D, "mfma_digitize_fold_kernel", [&](auto D) {
        auto launch = [&](auto SRC) {
            hipLaunchKernelGGL((mfma_digitize_fold_kernel<D(), SRC()>), grid, dim3(256), 0, s, a.B, a.bL, a.sbK, a.sbY,
                               a.log_n, a.P, Ppad, a.fold, a.Bdig, d0, pc, fs);
        };
        if (a.qsrc == 0) launch(std::integral_constant<int, 0>{});
        else if (a.qsrc == 1) launch(std::integral_constant<int, 1>{});
        else if (a.qsrc == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 3>{});
    });
}

static int launch_factored(const ModGemmArgs& a, int L, hipStream_t s) {
    const uint32_t Ppad = pad64(a.P);
    ModGemmArgs f = a;
    f.d0 = BdigLayout(a.Bdig, L, a.D, Ppad).d0();
    if (int rc = launch_fold(a, f.d0, L, Ppad, plane_counts(a, L), s)) return rc;
    return launch_factored_gemm<1>(f, L, Ppad, s);
}

// what the decrypt-fused digitize needs: n = 64 (one workgroup per (row y, limb), its 64 columns) and the ring tables
static bool dec_fused_ok(const ModGemmArgs& a) {
    return a.log_n == 6 && a.P == 64u * 64u && a.dsk && a.dlf && a.dtw && a.ditw && a.dninv;
}
// MFHE_DEC_SPLIT workgroups per (row, limb), each a share of the 8 panels, the column sums finished after
static_assert(MFHE_DEC_SPLIT == 1 || MFHE_DEC_SPLIT == 2 || MFHE_DEC_SPLIT == 4 || MFHE_DEC_SPLIT == 8,
              "the 8 panels split evenly");

// factored inverse: digitize (+ rows 0 / 255 / 256 by dot products), then the 256 x 256 GEMM per run of equal
// digit counts with the MODE 2 epilogue
static int launch_factored_inv(const ModGemmArgs& a, int L, hipStream_t s) {
    const uint32_t Ppad = pad64(a.P);
    const BdigLayout ws(a.Bdig, L, a.D, Ppad);
    ModGemmArgs f = a;
    f.cc = ws.cc();
    const PlaneCounts pc = plane_counts(a, L);
    if (a.dct) {
        if (!dec_fused_ok(a))
            return set_error(MFHE_EINVAL, "mod_gemm: the decrypt-fused inverse W-CRT needs n = 64 and the ring tables");
        constexpr int G = MFHE_DEC_SPLIT;
        f.dpart = ws.dpart();
        const int rc = dispatch_digits<5, 6>(a.D, "mfma_digitize_ifold_dec_kernel", [&](auto D) {
            hipLaunchKernelGGL(mfma_digitize_ifold_dec_kernel<D()>, dim3(64, L, G), dim3(256), 0, s, f, Ppad, pc);
        });
        if (rc) return rc;
        if (G > 1) {
            hipLaunchKernelGGL(dec_colsum_kernel, dim3((Ppad + 255) / 256, L), dim3(256), 0, s, f, Ppad, G);
            MFHE_CHECK_LAUNCH("dec_colsum_kernel");
        }
    } else {
        const int rc = dispatch_digits<5, 6>(a.D, "mfma_digitize_ifold_kernel", [&](auto D) {
            hipLaunchKernelGGL(mfma_digitize_ifold_kernel<D()>, dim3(Ppad / 16, L), dim3(256), 0, s, f, Ppad, pc);
        });
        if (rc) return rc;
    }
    return launch_factored_gemm<2>(f, L, Ppad, s);
}

// Two independent W-CRT transforms of the same shape (encode's re / im from the W-IDFT's doubles, decode's decrypt-fused
// re / im) as one launch per step: digitize pair, (column sums pair), ring56 GEMM pair -- grids of 2 L limbs, the upper
// half the second component.  Their workgroups share the GPU without a stream fork and its event waits (8-13 us of
// idle per fork or join, profiles/r05_pipeline_chain_trace.txt).  Anything else runs the two sequentially.
int launch_mod_gemm_pair(const ModGemmArgs& a, const ModGemmArgs& b, int L, hipStream_t s) {
    const uint32_t Ppad = pad64(a.P);
    uint64_t d6a = 0, d6b = 0;
    const bool inv = a.Adig && a.ifold && a.dct && b.Adig && b.ifold && b.dct && ring56_pair_usable<2>();
    const bool fwd = a.Adig && a.fold && a.qsrc && b.Adig && b.fold && b.qsrc && ring56_pair_usable<1>();
    const bool same = a.P == b.P && a.D == b.D && a.M == 512 && a.K == MK && a.epi && b.epi && a.lds_stage &&
                      a.D >= 5 && a.D <= 6 && 2 * L <= 128 && ring56_all(a, L, d6a) && ring56_all(b, L, d6b) &&
                      d6a == d6b;
    if (!(inv || fwd) || !same || (inv && !(dec_fused_ok(a) && dec_fused_ok(b) && a.iz && a.phi))) {
        if (int rc = launch_mod_gemm(a, L, s)) return rc;
        return launch_mod_gemm(b, L, s);
    }
    const PlaneCounts pc = plane_counts(a, L);
    ModGemmArgs f[2] = {a, b};
    const dim3 gg(2 * Ppad / 64, FK / 64, 2 * L);
    if (inv) {
        constexpr int G = MFHE_DEC_SPLIT;
        for (auto& x : f) {
            const BdigLayout ws(x.Bdig, L, x.D, Ppad);
            x.cc = ws.cc();
            x.dpart = ws.dpart();
        }
        const int rc = dispatch_digits<5, 6>(a.D, "mfma_digitize_ifold_dec_pair_kernel", [&](auto D) {
            hipLaunchKernelGGL(mfma_digitize_ifold_dec_pair_kernel<D()>, dim3(64, 2 * L, G), dim3(256), 0, s, f[0], f[1],
                               Ppad, pc);
        });
        if (rc) return rc;
        if (G > 1) {
            hipLaunchKernelGGL(dec_colsum_pair_kernel, dim3((Ppad + 255) / 256, 2 * L), dim3(256), 0, s, f[0], f[1], Ppad, G);
            MFHE_CHECK_LAUNCH("dec_colsum_pair_kernel");
        }
        hipLaunchKernelGGL(mod_gemm_mfma_ring56_pair_kernel<2>, gg, dim3(256), 0, s, f[0], f[1], Ppad, d6a);
        MFHE_CHECK_LAUNCH("mod_gemm_mfma_ring56_pair_kernel (factored inverse)");
        return MFHE_OK;
    }
    for (auto& x : f) x.d0 = BdigLayout(x.Bdig, L, x.D, Ppad).d0();
    // the two digitizes: one launch when both read the same doubles' rows (encode's re / im), else one each (the
    // encrypt's uniform a and Gaussian e)
    if (a.qsrc == 1 && b.qsrc == 1 && a.B == b.B && a.qf_row == b.qf_row && a.qf_step == b.qf_step &&
        a.delta == b.delta) {
        const FoldSrc fs = fold_src(a);
        const FoldPair fp{L, f[1].Bdig, f[1].d0, b.qf};
        const dim3 gq(2 * L, (Ppad + 127) / 128, FK / 32);
        const int rc = dispatch_digits<5, 6>(a.D, "mfma_digitize_fold_kernel (pair)", [&](auto D) {
            hipLaunchKernelGGL((mfma_digitize_fold_kernel<D(), 1, true>), gq, dim3(256), 0, s, a.B, a.bL, a.sbK, a.sbY,
                               a.log_n, a.P, Ppad, a.fold, f[0].Bdig, f[0].d0, pc, fs, fp);
        });
        if (rc) return rc;
    } else {
        for (const auto& x : f)
            if (int rc = launch_fold(x, x.d0, L, Ppad, pc, s)) return rc;
    }
    hipLaunchKernelGGL(mod_gemm_mfma_ring56_pair_kernel<1>, gg, dim3(256), 0, s, f[0], f[1], Ppad, d6a);
    MFHE_CHECK_LAUNCH("mod_gemm_mfma_ring56_pair_kernel (factored)");
    return MFHE_OK;
}

int launch_mod_gemm(const ModGemmArgs& a, int L, hipStream_t s) {
    if (a.dct && !(a.Adig && a.ifold)) return set_error(MFHE_EINVAL, "mod_gemm: a decrypt-fused B needs the factored inverse");
    if (a.Adig && a.ifold) {
        if (a.M != 512 || a.K != MK || !a.epi || a.D < 5 || a.D > 6 || !a.lds_stage || !a.iz || !a.phi)
            return set_error(MFHE_EINVAL, "mod_gemm: factored inverse W-CRT needs M = K = 512, the FP64 epilogue and D in {5, 6}");
        return launch_factored_inv(a, L, s);
    }
    if (a.Adig && a.fold) {
        if (a.M != 512 || a.K != MK || !a.epi || a.D < 5 || a.D > 6 || !a.lds_stage)
            return set_error(MFHE_EINVAL, "mod_gemm: factored W-CRT needs M = K = 512, the FP64 epilogue and D in {5, 6}");
        return launch_factored(a, L, s);
    }
    if (a.Adig && a.M == 512 && a.K == MK) {
        const uint32_t Ppad = pad64(a.P);
        const dim3 gd((Ppad + 255) / 256, MK / 32, L);
        const int rc = dispatch_digits<5, 8>(a.D, "mfma_digitize_kernel", [&](auto D) {
            hipLaunchKernelGGL(mfma_digitize_kernel<D()>, gd, dim3(256), 0, s, a.B, a.bL, a.sbK, a.sbY, a.log_n, a.P, Ppad,
                               a.Bdig, plane_counts(a, L));
        });
        if (rc) return rc;
        return for_digit_runs<5, 8>(a, L, "mod_gemm_mfma_kernel", [&](auto D, int l0, int l1) {
            const dim3 grid(Ppad / 64, 512 / 64, l1 - l0);
            if (a.lds_stage) launch_staged<D(), 0>(a.pipe >= 2 ? a.pipe : 1, grid, s, a, Ppad, l0);
            else hipLaunchKernelGGL(mod_gemm_mfma_kernel<D()>, grid, dim3(256), 0, s, a, Ppad, l0);
        });
    }
    dim3 grid((a.P + TP - 1) / TP, (a.M + TM - 1) / TM, L);
    hipLaunchKernelGGL(mod_gemm_kernel, grid, dim3(NTH), 0, s, a);
    MFHE_CHECK_LAUNCH("mod_gemm_kernel");
    return MFHE_OK;
}

}  // namespace mfhe

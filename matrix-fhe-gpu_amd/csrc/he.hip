// he.hip -- samplers, ring / combine kernels and the encode / keygen / encrypt / decrypt / decode pipelines at
// reference geometry, on the transform layer of wtrans.hip.
//
// Reference: src/core/HE.cu (samplers 564-627, 690-713; ring ops 509-560; pipelines 1272-1307, 1370-1708),
// src/core/batched_encoder.cu:161-228.
//
// Differences by design (results identical): one batched launch instead of per-lane launch loops
// (batched_encoder.cu:192-196, HE.cu:1653-1668, 1676-1679); no per-call malloc/free (a context workspace instead); the
// W-CRT output is written straight into the layout the caller needs; CRT compose and f64/delta are fused.
#include <hip/hip_runtime.h>

#include <cmath>

#include "he_sample.hpp"
#include "mfhe_ctx.hpp"
#include "mod128.hpp"
#include "ring_row.hpp"
#include "wcrt_gemm.hpp"
#include "wtrans.hpp"

namespace mfhe {

// ---------------- samplers (deterministic in the element index; the draws are in he_sample.hpp) ----------------
// ternary_secret_kernel HE.cu:690-713, [phi][L][n]
__global__ void ternary_kernel(uint64_t* s, const uint64_t* qmu, int L, int log_n, uint64_t total) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t n = 1ull << log_n, single = (uint64_t)L * n;
    const uint64_t off = idx % single;
    const int limb = (int)(off >> log_n);
    const uint64_t coeff = off & (n - 1), poly = idx / single;
    const uint64_t t = poly * 1315423911ULL + coeff * 2654435761ULL;
    const int r = (int)((t * 11400714819323198485ULL) % 3ULL);
    const uint64_t q = qmu[2 * limb];
    s[idx] = (r == 0) ? 0 : (r == 1) ? 1 : q - 1;
}

// uniform_random_kernel HE.cu:564-578, matrix-major [phi][L][n*n]; this context's limb l is global limb lbase + l of
// Ltot (mfhe_ctx_set_limb_shard)
__global__ void uniform_kernel(uint64_t* a, const uint64_t* qmu, int L, int log_n, uint64_t total, int lbase, int Ltot) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t n2 = 1ull << (2 * log_n), pos = idx & (n2 - 1);
    const uint32_t wl = (uint32_t)(idx >> (2 * log_n)), w = wl / (uint32_t)L;   // wl < 2^32: 32-bit division
    const int limb = (int)(wl - w * (uint32_t)L);
    const uint64_t seed = uniform_seed((uint64_t)w, (uint64_t)(lbase + limb), (uint64_t)Ltot, log_n, pos);
    a[idx] = uniform_reduce(seed, qmu[2 * limb], qmu[2 * limb + 1]);
}

// gaussian_noise_kernel HE.cu:581-627: one centred sample per [w][y][x], same integer in every limb.
// One thread per sample (the reference draws it once per limb), written to all L limbs.
__global__ void gaussian_kernel(uint64_t* e, const uint64_t* qmu, int L, int log_n, uint64_t total) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t n2 = 1ull << (2 * log_n);
    const uint64_t w = idx >> (2 * log_n), pos = idx & (n2 - 1);
    const long long nz = gauss_draw(w, pos, log_n);
    uint64_t* out = e + w * L * n2 + pos;
    for (int limb = 0; limb < L; ++limb) {
        const uint64_t q = qmu[2 * limb];
        out[(uint64_t)limb * n2] = (nz >= 0) ? (uint64_t)nz : q - (uint64_t)(-nz);
    }
}

// Once per [w][y][x] as a centred integer in a double: the factored W-CRT's digitize reads it for every limb
// (wcrt_digitize.hpp FoldSrc, qsrc 3), so the L-limb residue array never reaches HBM.
__global__ void gaussian_compact_kernel(double* e, int log_n, uint64_t total) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t n2 = 1ull << (2 * log_n);
    const uint64_t w = idx >> (2 * log_n), pos = idx & (n2 - 1);
    e[idx] = (double)gauss_draw(w, pos, log_n);
}

// As the one signed digit of e in the dense W-CRT GEMM's B layout (k-panel-major [512 / 32][P][32] bytes, k = w,
// p = pos; wcrt_mfma.hpp mod_gemm_mfma_smallb_kernel), shared by every limb: |e| <= 27, so the int8 holds e exactly.
// One thread per 4 consecutive k of one position (a 4-byte store), the 8 threads of a position's 32-k panel row
// adjacent: every wave writes 2 KiB contiguous.
__global__ void gaussian_i8_kernel(int8_t* __restrict__ b8, int log_n, uint32_t P) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;   // (panel, pos, k group of 4)
    if (idx >= 128ull * P) return;
    const uint64_t row = idx >> 3;                                          // panel * P + pos
    const uint32_t pos = (uint32_t)(row % P), k0 = (uint32_t)(row / P) * 32 + (uint32_t)(idx & 7) * 4;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= (uint32_t)(uint8_t)(int8_t)gauss_draw(k0 + j, pos, log_n) << (8 * j);
    *(uint32_t*)(b8 + row * 32 + (k0 & 31)) = word;
}

// ---------------- ring ops (poly-major [phi*n][L][n]) ----------------
// pointwise_mul_s_kernel HE.cu:509-531: t = a * s[w][l][x], w = poly / n.  The reference reduces with
// an __int128 % per element (a software division here too); this uses the exact FP64 modmul of the NTT
// (ntt_arith.hpp) when every q < 2^50, else the u128 fold of mod128.hpp.
__global__ __launch_bounds__(256) void mul_s_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ s,
                                                    uint64_t* __restrict__ t, const uint64_t* __restrict__ qmu,
                                                    const uint64_t* __restrict__ r64, const LimbConst* __restrict__ lf,
                                                    int L, int log_n, uint32_t total) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t n = 1u << log_n, single = (uint32_t)L << log_n;
    const uint32_t poly = idx / single, off = idx - poly * single;
    const int l = (int)(off >> log_n);
    const uint32_t coeff = off & (n - 1), w = poly >> log_n;
    const uint64_t av = a[idx], sv = s[((uint64_t)w * L + l) * n + coeff];
    if (lf) {
        const ArithF64 ar(lf[l]);
        t[idx] = ar.canon(ar.mulmod(ArithF64::from_u64(av), ArithF64::from_u64(sv)));
        return;
    }
    t[idx] = mod_u128_fold(__umul64hi(av, sv), av * sv, qmu[2 * l], qmu[2 * l + 1], r64[l]);
}

// encrypt epilogue, fused: for matrix-major index i (x, y, l, w) and its poly-major index p,
//   ct_k.b[i] = m_k[i] - t[p] + e[p] mod q   (combine_b_kernel HE.cu:535-547, then poly_to_matrix)
//   ct_k.a[i] = a_eval[p]                   (the shared a, poly_to_matrix)
// for k = re (and im when given) in one pass: 3 + 2 reads and 2 + 2 writes instead of the 20 array
// passes of layout -> combine -> layout -> layout per component.
__global__ __launch_bounds__(256) void enc_combine_kernel(const uint64_t* __restrict__ m_re,
                                                          const uint64_t* __restrict__ m_im,
                                                          const uint64_t* __restrict__ t, const uint64_t* __restrict__ e,
                                                          const uint64_t* __restrict__ aev, uint64_t* __restrict__ ct_re,
                                                          uint64_t* __restrict__ ct_im, const uint64_t* __restrict__ qmu,
                                                          int log_n, int L, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;   // matrix-major index
    if (i >= total) return;
    const uint64_t p = pm_index(i, log_n, L);
    const uint32_t wl = (uint32_t)(i >> (2 * log_n)), l = wl - wl / (uint32_t)L * (uint32_t)L;
    const uint64_t q = qmu[2 * l];
    const uint64_t tv = t[p], ev = e[p], av = aev[p];
    auto bval = [&](uint64_t m) {
        uint64_t d = m >= tv ? m - tv : m + q - tv;
        d += ev;
        return d >= q ? d - q : d;
    };
    ct_re[i] = bval(m_re[i]);
    ct_re[total + i] = av;
    if (m_im) {
        ct_im[i] = bval(m_im[i]);
        ct_im[total + i] = av;
    }
}

// One thread of the fused ring kernels: 4 coefficients (ld_row / st_row's, from j) of matrix row R = (w L + l) n + y.
struct RingRow {
    int j;
    uint32_t w, l;
    uint64_t i0, p0;   // row starts: matrix- / poly-major
    bool live;         // dead lanes (rows past the end, clamped to row 0) still take part in the shuffles
};
template <int LOGN>
__device__ __forceinline__ RingRow ring_row_decode(const RingArgs& ra) {
    constexpr int N = 1 << LOGN, T = N / 4;
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    RingRow r;
    r.j = (int)(g % T);
    const uint64_t R = g / T;
    r.live = R < ra.rows;
    const uint64_t Rc = r.live ? R : 0;
    const uint64_t y = Rc % N;
    const uint32_t wl = (uint32_t)(Rc / N);   // wl < 2^32
    r.w = wl / (uint32_t)ra.L;
    r.l = wl - r.w * (uint32_t)ra.L;
    r.i0 = Rc * N;
    r.p0 = (((uint64_t)r.w * N + y) * ra.L + r.l) * N;
    return r;
}
constexpr bool ring_lds(int logn) { return logn == 6 && MFHE_RING_LDS; }   // ring_mul_row64_lds: reg s holds coefficient j + 16 s
#ifndef MFHE_ENC_NT
#define MFHE_ENC_NT 1   // enc_ring_kernel's row streams as nontemporal accesses (read / written once; 0 for A/B)
#endif
// encrypt, fused: t = a * s over X (ring_mul_row), then encrypt_pair's combine (HE.cu:1530-1552):
// ct_k.b = m_k - t + e, ct_k.a = a, written matrix-major; a, e poly-major.
template <int LOGN>
// a_mm: a is already in both ciphertexts (the W-CRT GEMM wrote it there, matrix-major): read it from aev + i0 and
// write only the b halves -- 6 of the 8 row streams
__global__ __launch_bounds__(256) void enc_ring_kernel(RingArgs ra, const uint64_t* __restrict__ aev,
                                                       const uint64_t* __restrict__ e, const uint64_t* __restrict__ m_re,
                                                       const uint64_t* __restrict__ m_im, uint64_t* __restrict__ ct_re,
                                                       uint64_t* __restrict__ ct_im, int a_mm) {
    constexpr int N = 1 << LOGN;
    constexpr bool LDS = ring_lds(LOGN), NT = MFHE_ENC_NT && LDS;
    const RingRow r = ring_row_decode<LOGN>(ra);
    const int j = r.j;
    const uint64_t i0 = r.i0, p0 = r.p0;
    const LimbConst lc = ra.lf[r.l];
    const ArithF64 ar(lc);
    uint64_t av[4], sk[4];
    ld_row<LDS, NT>(aev + (a_mm ? i0 : p0), j, av);
    ld4(ra.sk + ((uint64_t)r.w * ra.L + r.l) * N + 4 * j, sk);
    // the combine's operands are loaded before the ring product (clamped rows for dead lanes), so their latency
    // overlaps the butterflies instead of following them
    uint64_t ev[4], mv[4], mi[4], b[4];
    ld_row<LDS, NT>(e + p0, j, ev);
    ld_row<LDS, NT>(m_re + i0, j, mv);
    if (m_im) ld_row<LDS, NT>(m_im + i0, j, mi);
    double x[4], sv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        x[s] = ArithF64::from_u64(av[s]);
        sv[s] = centred_f(sk[s], lc.qf);
    }
    if constexpr (LDS) {
        __shared__ double rscr[16 * 68];
        ring_mul_row64_lds(x, sv, j, ar, ra.tw + r.l * N, ra.itw + r.l * N, ra.ninv[r.l], rscr + (threadIdx.x >> 4) * 68);
    } else {
        ring_mul_row<LOGN>(x, sv, j, ar, ra.tw + r.l * N, ra.itw + r.l * N, ra.ninv[r.l]);
    }
    if (!r.live) return;
    const uint64_t q = lc.q, total = ra.rows * N;
    auto bval = [&](uint64_t m, int s) {
        const uint64_t tv = ar.canon(x[s]);
        uint64_t d = m >= tv ? m - tv : m + q - tv;
        d += ev[s];
        return d >= q ? d - q : d;
    };
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = bval(mv[s], s);
    st_row<LDS, NT>(ct_re + i0, j, b);
    if (!a_mm) st_row<LDS, NT>(ct_re + total + i0, j, av);
    if (m_im) {
#pragma unroll
        for (int s = 0; s < 4; ++s) b[s] = bval(mi[s], s);
        st_row<LDS, NT>(ct_im + i0, j, b);
        if (!a_mm) st_row<LDS, NT>(ct_im + total + i0, j, av);
    }
}

// decrypt, fused: out = ct.b + INTT(NTT(ct.a) * s), ct matrix-major in, out poly-major (HE.cu:1553-1601:
// matrix_to_poly, X-NTT, pointwise_mul_s, X-INTT, add_poly).
template <int LOGN>
__global__ __launch_bounds__(256) void dec_ring_kernel(RingArgs ra, const uint64_t* __restrict__ ct,
                                                       uint64_t* __restrict__ out) {
    constexpr int N = 1 << LOGN;
    constexpr bool LDS = ring_lds(LOGN);
    const RingRow r = ring_row_decode<LOGN>(ra);
    const int j = r.j;
    const uint64_t i0 = r.i0, total = ra.rows * N;
    const LimbConst lc = ra.lf[r.l];
    const ArithF64 ar(lc);
    uint64_t av[4], sk[4], bv[4];
    ld_row<LDS>(ct + total + i0, j, av);
    ld4(ra.sk + ((uint64_t)r.w * ra.L + r.l) * N + 4 * j, sk);
    ld_row<LDS>(ct + i0, j, bv);   // before the ring product, so its latency overlaps the butterflies (clamped row if dead)
    // x = a * s, written out as in enc_ring_kernel: shared as a device function it compiles to other code (LOGN 4..6)
    double x[4], sv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        x[s] = ArithF64::from_u64(av[s]);
        sv[s] = centred_f(sk[s], lc.qf);
    }
    if constexpr (LDS) {
        __shared__ double rscr[16 * 68];
        ring_mul_row64_lds(x, sv, j, ar, ra.tw + r.l * N, ra.itw + r.l * N, ra.ninv[r.l], rscr + (threadIdx.x >> 4) * 68);
    } else {
        ring_mul_row<LOGN>(x, sv, j, ar, ra.tw + r.l * N, ra.itw + r.l * N, ra.ninv[r.l]);
    }
    if (!r.live) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint64_t sum = bv[s] + ar.canon(x[s]);
        bv[s] = sum >= lc.q ? sum - lc.q : sum;
    }
    st_row<LDS>(out + r.p0, j, bv);
}

static bool ring_fused_ok(const mfhe_ctx* c, int logn) {
    return c->he_fused && c->f64_ok && c->ph_f.tw && logn >= 2 && logn <= 6;
}

static RingArgs ring_args(const mfhe_ctx* c, const uint64_t* sk, int L, uint64_t rows) {
    return {.lf = c->d_limbs, .tw = c->ph_f.tw, .itw = c->ph_f.itw, .ninv = c->ph_f.ninv, .sk = sk, .L = L,
            .rows = rows};
}

// decrypt_and_decode: the decrypt fused into the factored inverse W-CRT's digitize (n = 64, the same conditions
// as the factored inverse in use_mfma plus ring_fused_ok)
static bool dec_fused_ok(const mfhe_ctx* c, int logn) {
    return ring_fused_ok(c, logn) && logn == 6 && c->wcrt_mfma == 1 && c->wD && c->d_wZidig && c->d_wepi &&
           c->d_wifold && c->d_wiz && c->d_wphi;
}

#define MFHE_RING_DISPATCH(KERNEL, logn, grid, s, ...)                                       \
    switch (logn) {                                                                           \
        case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, s, __VA_ARGS__); break;     \
        case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, s, __VA_ARGS__); break;     \
        case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, s, __VA_ARGS__); break;     \
        case 5: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(256), 0, s, __VA_ARGS__); break;     \
        default: hipLaunchKernelGGL(KERNEL<6>, grid, dim3(256), 0, s, __VA_ARGS__); break;    \
    }

// decrypt epilogue, fused: out[p] = ct.b[i] + t[p] mod q (matrix_to_poly of b, then add_poly_kernel
// HE.cu:549-560), over the poly-major index p.
__global__ __launch_bounds__(256) void dec_combine_kernel(const uint64_t* __restrict__ ctb, const uint64_t* __restrict__ t,
                                                          uint64_t* __restrict__ out, const uint64_t* __restrict__ qmu,
                                                          int log_n, int L, uint64_t total) {
    const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;   // poly-major index [w n + y][l][x]
    if (p >= total) return;
    const uint64_t n = 1ull << log_n;
    const uint64_t x = p & (n - 1), rest = p >> log_n, l = rest % L, wy = rest / L;
    const uint64_t y = wy & (n - 1), w = wy >> log_n;
    const uint64_t i = (((w * L + l) << log_n) + y) * n + x;            // matrix-major [w][l][y][x]
    const uint64_t q = qmu[2 * l];
    const uint64_t sum = ctb[i] + t[p];
    out[p] = sum >= q ? sum - q : sum;
}

// add_ct_kernel HE.cu:631-645 / mul_tensor_kernel HE.cu:648-669 over matrix-major [phi][L][n2]
// (limb = (idx / n2) % L).  `half` = words of one ciphertext component.
__global__ void ct_add_kernel(const uint64_t* x, const uint64_t* y, uint64_t* r,
                              const uint64_t* qmu, int L, int log_n2, uint64_t half) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= 2 * half) return;
    const int l = (int)(((idx % half) >> log_n2) % (uint64_t)L);
    const uint64_t q = qmu[2 * l];
    const uint64_t s = x[idx] + y[idx];
    r[idx] = s >= q ? s - q : s;
}
__global__ void ct_mul_kernel(const uint64_t* __restrict__ c1, const uint64_t* __restrict__ c2, uint64_t* d0,
                              uint64_t* d1, uint64_t* d2, const uint64_t* qmu, const uint64_t* r64, int L, int log_n2,
                              uint64_t half) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= half) return;
    const int l = (int)((idx >> log_n2) % (uint64_t)L);
    const uint64_t q = qmu[2 * l], mu = qmu[2 * l + 1], rr = r64[l];
    const uint64_t b1 = c1[idx], a1 = c1[half + idx], b2 = c2[idx], a2 = c2[half + idx];
    d0[idx] = mulmod_fold(b1, b2, q, mu, rr);
    const uint64_t t1 = mulmod_fold(b1, a2, q, mu, rr), t2 = mulmod_fold(a1, b2, q, mu, rr);
    const uint64_t t = t1 + t2;
    d1[idx] = t >= q ? t - q : t;
    d2[idx] = mulmod_fold(a1, a2, q, mu, rr);
}

// keygen, encrypt and decrypt run the X-NTT
static int need_xntt(const mfhe_ctx* c, const char* what) {
    if (c->conv & MFHE_CONV_PHANTOM) return MFHE_OK;
    return set_error(MFHE_ENOTREADY, std::string(what) + " needs MFHE_CONV_PHANTOM (X-NTT)");
}

// Two independent chains of one call (encode's re / im W-CRT, encrypt's a / e W-CRT, decode's re / im W-INTT +
// compose): the second runs on the context's side stream, forked from and joined back into the caller's stream by
// events, so the digitize (memory / FP64-VALU bound) of one overlaps the i8-MFMA GEMM of the other and each GEMM's
// tail.  The side chain's GEMM uses its own digit planes (WcrtReq slot 1).  MFHE_OPT_HE_STREAMS 0: x = s.
static int he_side_stream(mfhe_ctx* c) {   // created once (mfhe_ctx_reserve_workspace, or the first forked call)
    if (c->he_side) return MFHE_OK;
    MFHE_HIP(hipEventCreateWithFlags(&c->he_fork, hipEventDisableTiming));
    MFHE_HIP(hipEventCreateWithFlags(&c->he_join, hipEventDisableTiming));
    MFHE_HIP(hipStreamCreateWithFlags(&c->he_side, hipStreamNonBlocking));
    return MFHE_OK;
}
struct HeFork {
    hipStream_t s = nullptr, x = nullptr;
    mfhe_ctx* c = nullptr;
    bool on = false;
    int begin(mfhe_ctx* c_, hipStream_t s_, bool enable) {
        c = c_;
        s = x = s_;
        if (!enable) return MFHE_OK;
        RC(he_side_stream(c));
        MFHE_HIP(hipEventRecord(c->he_fork, s));
        MFHE_HIP(hipStreamWaitEvent(c->he_side, c->he_fork, 0));
        x = c->he_side;
        on = true;
        return MFHE_OK;
    }
    // every later use of the side chain's results (and of its workspace) is ordered after this on s
    int join() {
        if (!on) return MFHE_OK;
        on = false;
        MFHE_HIP(hipEventRecord(c->he_join, x));
        MFHE_HIP(hipStreamWaitEvent(s, c->he_join, 0));
        return MFHE_OK;
    }
    ~HeFork() { (void)join(); }   // an early error return still joins the side stream into s
};

static int encode_impl(mfhe_ctx* c, const double* msg, uint64_t* out_re, uint64_t* out_im, hipStream_t s) {
    RC(need_wcrt(c));
    if (!msg || !out_re || !out_im) return set_error(MFHE_EINVAL, "mfhe_encode: null pointer");
    RC(ensure_xy(c));
    RC(ensure_ws(c));
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    double2* xy = b.get<double2>(g.cnt);
    double2* tmp = b.get<double2>(g.cnt);
    uint64_t* cre = b.get<uint64_t>(g.words);
    // 1) XY-IDFT per lane (Encoder::idft2, encoder.cu:460-467)
    RC(xy3(c, c->d_encVi, (const double2*)msg, c->d_encViT, tmp, xy, 512, s));
    // 2) W-IDFT (w_idft_kernel, batched_encoder.cu:104-123); planar (real plane, then imaginary) when the fused
    // digitize reads it, so each of its per-limb passes reads whole 8-byte lanes (r06)
    const bool planar = quant_fused_ok(c) && wdft_planar_ok(c);
    RC(wdft(c, c->d_wdVinv, xy, tmp, s, planar));
    // 3) quantize + RNS split, 4) W-CRT -> matrix-major eval (re, then im); fused into the W-CRT's digitize
    // kernel when the factored forward runs (the residues never reach HBM)
    if (quant_fused_ok(c)) {
        const double* qre = (const double*)tmp;
        const double* qim = planar ? qre + 512ull * g.n2 : qre + 1;
        WcrtReq re{.A = c->d_wV, .B = (const uint64_t*)tmp, .C = out_re, .out = WOut::Matrix, .src = WSrc::Quant,
                   .qf = qre, .step = planar ? 1u : 2u};
        WcrtReq im = re;
        im.C = out_im;
        im.qf = qim;
        if (c->he_streams >= 2) {   // modes 2, 3: re and im as one launch per step (wcrt_gemm.hip launch_mod_gemm_pair)
            ModGemmArgs ar, ai;
            im.slot = 1;
            RC(wcrt_args(c, ar, re));
            RC(wcrt_args(c, ai, im));
            return launch_mod_gemm_pair(ar, ai, g.L, s);
        }
        HeFork f;
        RC(f.begin(c, s, c->he_streams == 1));
        im.slot = f.on ? 1 : 0;
        RC(wcrt_gemm(c, re, s));
        RC(wcrt_gemm(c, im, f.x));
        return f.join();
    }
    RC(mfhe_rns_decompose(c, (const double*)tmp, 2, 512, g.n2, cre, (mfhe_stream_t)s));
    RC(wcrt_gemm(c, {.A = c->d_wV, .B = cre, .C = out_re, .out = WOut::Matrix}, s));
    RC(mfhe_rns_decompose(c, (const double*)tmp + 1, 2, 512, g.n2, cre, (mfhe_stream_t)s));
    RC(wcrt_gemm(c, {.A = c->d_wV, .B = cre, .C = out_im, .out = WOut::Matrix}, s));
    return MFHE_OK;
}

// dec: ev_re / ev_im are the ciphertexts, decrypted inside the W-INTT's digitize (dec_fused_ok only)
static int decode_impl(mfhe_ctx* c, const uint64_t* ev_re, const uint64_t* ev_im, double* msg, hipStream_t s,
                       Bump* pb = nullptr, const RingArgs* dec = nullptr) {
    RC(need_wcrt(c));
    if (!ev_re || !ev_im || !msg) return set_error(MFHE_EINVAL, "mfhe_decode: null pointer");
    RC(ensure_xy(c));
    Bump b0{nullptr};
    if (!pb) {
        RC(ensure_ws(c));   // may allocate or move the workspace: take its address only afterwards
        b0.p = (char*)c->ws;
        pb = &b0;
    }
    const Geo2 g = geo(c);
    uint64_t* coeff = pb->get<uint64_t>(g.words);
    double2* ccx = pb->get<double2>(g.cnt);
    double2* ecx = pb->get<double2>(g.cnt);
    // W-INTT (poly-major in -> matrix-major coeff), CRT compose + centre + /delta fused, into re / im (im on the side
    // stream with its own coefficient buffer; the two composes write alternate doubles of ccx)
    WcrtReq re{.A = c->d_wVinv, .B = ev_re, .b_poly = true, .C = coeff, .out = WOut::Matrix, .dec = dec};
    WcrtReq im = re;
    im.B = ev_im;
    if (c->he_streams == 2) {
        // re and im as one launch per step: W-INTT pair (wcrt_gemm.hip launch_mod_gemm_pair), then one compose launch
        uint64_t* coeff_im = pb->get<uint64_t>(g.words);
        ModGemmArgs ar, ai;
        im.C = coeff_im;
        im.slot = 1;
        RC(wcrt_args(c, ar, re));
        RC(wcrt_args(c, ai, im));
        RC(launch_mod_gemm_pair(ar, ai, g.L, s));
        RC(crt_compose_f64_pair(c, coeff, coeff_im, 512, g.n2, (double*)ccx, (double*)ccx + 1, 2, s));
    } else {
        HeFork f;
        RC(f.begin(c, s, c->he_streams == 1 || c->he_streams == 3));
        uint64_t* coeff_im = f.on ? pb->get<uint64_t>(g.words) : coeff;
        im.C = coeff_im;
        im.slot = f.on ? 1 : 0;
        RC(wcrt_gemm(c, re, s));
        RC(mfhe_crt_compose_f64(c, coeff, 512, g.n2, (double*)ccx, 2, (mfhe_stream_t)s));
        RC(wcrt_gemm(c, im, f.x));
        RC(mfhe_crt_compose_f64(c, coeff_im, 512, g.n2, (double*)ccx + 1, 2, (mfhe_stream_t)f.x));
        RC(f.join());
    }
    // W-DFT, then XY-DFT per lane: M = V E V^T
    RC(wdft(c, c->d_wdV, ccx, ecx, s));
    return xy3(c, c->d_encV, ecx, c->d_encVT, ccx, (double2*)msg, 512, s);
}

static int keygen_impl(mfhe_ctx* c, uint64_t* sk, hipStream_t s) {
    RC(need_wcrt(c));
    RC(need_xntt(c, "keygen"));
    if (!sk) return set_error(MFHE_EINVAL, "mfhe_keygen: null pointer");
    RC(ensure_ws(c));
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    uint64_t* sc = b.get<uint64_t>(512ull * g.L * g.n);
    const uint64_t total = 512ull * g.L * g.n;
    hipLaunchKernelGGL(ternary_kernel, g1(total), dim3(256), 0, s, sc, c->d_rns_mu, g.L, g.logn, total);
    MFHE_CHECK_LAUNCH("ternary_kernel");
    RC(wcrt_gemm(c, {.A = c->d_wV, .B = sc, .C = sk, .out = WOut::Vector, .vector = true}, s));
    return mfhe_ntt_fwd(c, sk, 512, 0, g.L, (mfhe_stream_t)s);
}

// the unfused ring product: t = INTT(NTT(a) * s) over every X row, a poly-major (transformed in place)
static int ring_mul_s(mfhe_ctx* c, uint64_t* a, const uint64_t* sk, uint64_t* t, hipStream_t s) {
    const Geo2 g = geo(c);
    RC(mfhe_ntt_fwd(c, a, 512 * g.n, 0, g.L, (mfhe_stream_t)s));
    if (g.words >= (1ull << 32)) return set_error(MFHE_EUNSUPPORTED, "ciphertext of 2^32 words or more");
    hipLaunchKernelGGL(mul_s_kernel, g1(g.words), dim3(256), 0, s, a, sk, t, c->d_rns_mu, c->d_r64,
                       c->f64_ok ? c->d_limbs : nullptr, g.L, g.logn, (uint32_t)g.words);
    MFHE_CHECK_LAUNCH("mul_s_kernel");
    return mfhe_ntt_inv(c, t, 512 * g.n, 0, g.L, (mfhe_stream_t)s);
}

// encrypt (HE.cu:1370-1453) / encrypt_pair (HE.cu:1455-1552)
static int encrypt_impl(mfhe_ctx* c, const uint64_t* m_re, const uint64_t* m_im, const uint64_t* sk, uint64_t* ct_re,
                        uint64_t* ct_im, hipStream_t s) {
    RC(need_wcrt(c));
    RC(need_xntt(c, "encrypt"));
    if (!m_re || !sk || !ct_re || (m_im && !ct_im)) return set_error(MFHE_EINVAL, "mfhe_encrypt: null pointer");
    RC(ensure_ws(c));
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    uint64_t* ap = b.get<uint64_t>(g.words);
    uint64_t* aev = b.get<uint64_t>(g.words);
    uint64_t* ant = b.get<uint64_t>(g.words);
    uint64_t* ep = b.get<uint64_t>(g.words);
    uint64_t* eev = b.get<uint64_t>(g.words);
    const uint64_t W = g.words;
    const bool a_mm = quant_fused_ok(c) && ring_fused_ok(c, g.logn) && c->enc_a_direct;
    // shared a: W coeff -> W-CRT eval (poly-major) -> X-NTT
    // e: identical for re and im (seed depends only on the coefficient, HE.cu:605-608)
    const WcrtReq e_plain{.A = c->d_wV, .B = ep, .C = eev, .out = WOut::Poly};
    if (quant_fused_ok(c)) {
        // the samplers evaluated inside the factored W-CRT's digitize: a in place, e from one draw per coefficient;
        // with the fused ring, a straight into both ciphertexts' a halves (matrix-major), where enc_ring reads it.
        // MFHE_OPT_HE_STREAMS 2: the two GEMMs as one launch (wcrt_gemm.hip launch_mod_gemm_pair; measured no faster than
        // two: 301 vs 160 + 138 us, profiles/r05_he_stream_modes.txt, so mode 3 keeps two)
        const bool pair = c->he_streams == 2;
        ModGemmArgs aa, ae;
        RC(wcrt_args(c, aa, {.A = c->d_wV, .B = ap, .C = a_mm ? ct_re + W : aev, .out = a_mm ? WOut::Matrix : WOut::Poly,
                             .src = WSrc::Uniform, .C2 = a_mm && m_im ? ct_im + W : nullptr}));
        // the noise: its W-CRT forward as the dense product with its one signed digit (MFHE_OPT_ENC_E_SMALL, wcrt_mfma.hpp
        // mod_gemm_mfma_smallb_kernel) where the dense V planes have 5-6 digits; else factored from its residues
        const bool e_small = c->enc_e_small && !pair && c->d_wVdig && c->wD >= 5 && c->wD <= 6 && g.n2 % 64 == 0;
        if (e_small) {
            RC(wcrt_args(c, ae, e_plain));
            ae.Adig = c->d_wVdig;   // the dense V planes (use_mfma chose the factored ones)
            ae.adL = (uint64_t)c->wD * 512 * 512;
            ae.fold = nullptr;
            RC(launch_mod_gemm(aa, g.L, s));
            int8_t* b8 = (int8_t*)ep;   // 512 x n^2 bytes, inside the unused residue buffer
            hipLaunchKernelGGL(gaussian_i8_kernel, g1(128ull * g.n2), dim3(256), 0, s, b8, g.logn, (uint32_t)g.n2);
            MFHE_CHECK_LAUNCH("gaussian_i8_kernel");
            RC(launch_mod_gemm_smallb(ae, b8, g.L, s));
        } else {
            WcrtReq e_noise = e_plain;
            e_noise.src = WSrc::Noise;
            e_noise.qf = (const double*)ep;
            e_noise.slot = pair ? 1 : 0;
            RC(wcrt_args(c, ae, e_noise));
            if (!pair) RC(launch_mod_gemm(aa, g.L, s));
            hipLaunchKernelGGL(gaussian_compact_kernel, g1(W / g.L), dim3(256), 0, s, (double*)ep, g.logn, W / g.L);
            MFHE_CHECK_LAUNCH("gaussian_compact_kernel");
            if (pair) RC(launch_mod_gemm_pair(aa, ae, g.L, s));
            else RC(launch_mod_gemm(ae, g.L, s));
        }
    } else {
        hipLaunchKernelGGL(uniform_kernel, g1(W), dim3(256), 0, s, ap, c->d_rns_mu, g.L, g.logn, W, c->limb_base,
                           c->limbs_total ? c->limbs_total : g.L);
        MFHE_CHECK_LAUNCH("uniform_kernel");
        RC(wcrt_gemm(c, {.A = c->d_wV, .B = ap, .C = aev, .out = WOut::Poly}, s));
        hipLaunchKernelGGL(gaussian_kernel, g1(W / g.L), dim3(256), 0, s, ep, c->d_rns_mu, g.L, g.logn, W / g.L);
        MFHE_CHECK_LAUNCH("gaussian_kernel");
        RC(wcrt_gemm(c, e_plain, s));
    }
    if (ring_fused_ok(c, g.logn)) {
        const uint64_t rows = W / g.n;
        const RingArgs ra = ring_args(c, sk, g.L, rows);
        MFHE_RING_DISPATCH(enc_ring_kernel, g.logn, g1(rows * (g.n / 4)), s, ra, a_mm ? ct_re + W : aev, eev, m_re, m_im,
                           ct_re, ct_im, (int)a_mm);
        MFHE_CHECK_LAUNCH("enc_ring_kernel");
        return MFHE_OK;
    }
    MFHE_HIP(hipMemcpyAsync(ant, aev, W * 8, hipMemcpyDeviceToDevice, s));
    uint64_t* t = ep;   // reuse ep as t
    RC(ring_mul_s(c, ant, sk, t, s));
    hipLaunchKernelGGL(enc_combine_kernel, g1(W), dim3(256), 0, s, m_re, m_im, t, eev, aev, ct_re, ct_im,
                       c->d_rns_mu, g.logn, g.L, W);
    MFHE_CHECK_LAUNCH("enc_combine_kernel");
    return MFHE_OK;
}

static int decrypt_impl(mfhe_ctx* c, const uint64_t* ct, const uint64_t* sk, uint64_t* out, hipStream_t s, Bump* pb) {
    const Geo2 g = geo(c);
    const uint64_t W = g.words;
    if (ring_fused_ok(c, g.logn)) {
        const uint64_t rows = W / g.n;
        const RingArgs ra = ring_args(c, sk, g.L, rows);
        MFHE_RING_DISPATCH(dec_ring_kernel, g.logn, g1(rows * (g.n / 4)), s, ra, ct, out);
        MFHE_CHECK_LAUNCH("dec_ring_kernel");
        return MFHE_OK;
    }
    uint64_t* ap = pb->get<uint64_t>(W);
    uint64_t* t = pb->get<uint64_t>(W);
    RC(layout(c, ct + W, ap, true, s));
    RC(ring_mul_s(c, ap, sk, t, s));
    hipLaunchKernelGGL(dec_combine_kernel, g1(W), dim3(256), 0, s, ct, t, out, c->d_rns_mu, g.logn, g.L, W);
    MFHE_CHECK_LAUNCH("dec_combine_kernel");
    return MFHE_OK;
}

// What a decode after a decrypt reads.  Where the decrypt runs inside the W-INTT's digitize (dec_fused_ok): the
// ciphertexts themselves, with dec = &ra.  Else re / im become the two decrypted evaluations, taken from *b (the decode
// carves its own buffers from *b after them), and dec is null.
static int decrypt_pair(mfhe_ctx* c, const uint64_t*& re, const uint64_t*& im, const uint64_t* sk, hipStream_t s,
                        Bump* b, RingArgs& ra, const RingArgs*& dec) {
    const Geo2 g = geo(c);
    ra = ring_args(c, sk, g.L, g.words / g.n);
    dec = dec_fused_ok(c, g.logn) ? &ra : nullptr;
    if (dec) return MFHE_OK;
    uint64_t* er = b->get<uint64_t>(g.words);
    uint64_t* ei = b->get<uint64_t>(g.words);
    Bump inner = *b;
    RC(decrypt_impl(c, re, sk, er, s, &inner));
    inner = *b;
    RC(decrypt_impl(c, im, sk, ei, s, &inner));
    re = er;
    im = ei;
    return MFHE_OK;
}

// Residue-sharded decode (BASELINE C4): this rank's W-INTT of its limbs, the RCCL recombine of every lane's
// L residues (dist.cpp) into this rank's lane slice of the centred / delta values, an all-gather of those
// f64 slices, then the W-DFT and XY-DFT of the whole batch (FP64, replicated on every rank).  Replaces
// decode_eval_pair_to_complex (HE.cu:1619-1689) whose per-lane compose loop (:1653-1668) is the exchange step.
static int decode_sharded_impl(mfhe_ctx* c, mfhe_ctx* call, mfhe_comm* comm, int mode, const uint64_t* ev_re,
                               const uint64_t* ev_im, double* msg, hipStream_t s, Bump* pb,
                               const RingArgs* dec = nullptr) {
    const Geo2 g = geo(c);
    int G = 1, rank = 0;
    RC(comm_size_rank(comm, &G, &rank));
    uint64_t* coeff_re = pb->get<uint64_t>(g.words);
    uint64_t* coeff_im = pb->get<uint64_t>(g.words);
    double2* ccx = pb->get<double2>(g.cnt);
    double2* ecx = pb->get<double2>(g.cnt);
    // both W-INTTs first, then the two chunked recombines back to back; the im call passes MFHE_RECOMBINE_AFTER_PREV
    // (coeff_im was complete when the re call was entered), so the exchange stream runs the im chunks right after the
    // re chunks, waiting only for the composes whose receive half it refills (dist.cpp mfhe_crt_recombine_chunked).
    // Rows land at their
    // lane index (MFHE_RECOMBINE_ROWS_GLOBAL), so each chunk's lanes [p0, p0 + cp) are [rank][cp / G] in lane order
    // and one in-place all-gather per chunk completes them on every rank.
    const size_t cp = mfhe_ctx::PHI / 4 >= (size_t)G ? mfhe_ctx::PHI / 4 / G * G : (size_t)G;
    RC(wcrt_gemm(c, {.A = c->d_wVinv, .B = ev_re, .b_poly = true, .C = coeff_re, .out = WOut::Matrix, .dec = dec}, s));
    RC(wcrt_gemm(c, {.A = c->d_wVinv, .B = ev_im, .b_poly = true, .C = coeff_im, .out = WOut::Matrix, .dec = dec}, s));
    // Both recombines are always issued and their statuses agreed on once at the end: a rank whose re call fails
    // locally after its exchanges started still joins the im call's collectives and the agreement, so no peer is left
    // waiting in a collective this rank skipped; every rank then returns the error.
    const int rre = mfhe_crt_recombine_chunked(call, comm, mode, coeff_re, 512, g.n2, cp, (double*)ccx, 2,
                                               MFHE_RECOMBINE_ROWS_GLOBAL, (mfhe_stream_t)s);
    const std::string ere = rre ? mfhe_last_error() : "";
    const int rim = mfhe_crt_recombine_chunked(call, comm, mode, coeff_im, 512, g.n2, cp, (double*)ccx + 1, 2,
                                               MFHE_RECOMBINE_ROWS_GLOBAL | MFHE_RECOMBINE_AFTER_PREV, (mfhe_stream_t)s);
    RC(comm_agree(comm, rre ? set_error(rre, ere) : rim, s));
    for (size_t p0 = 0; p0 < 512; p0 += cp) {
        const size_t bs = (512 - p0 < cp ? 512 - p0 : cp) / (size_t)G;
        RC(comm_allgather_bytes(comm, ccx + (p0 + (size_t)rank * bs) * g.n2, ccx + p0 * g.n2,
                                bs * g.n2 * sizeof(double2), s));   // in place
    }
    RC(wdft(c, c->d_wdV, ccx, ecx, s));
    return xy3(c, c->d_encV, ecx, c->d_encVT, ccx, (double2*)msg, 512, s);
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ctx_reserve_workspace(mfhe_ctx* c) {
    RC(need_wcrt(c));
    RC(ensure_ws(c));
    // both GEMM digit-plane workspaces (the caller's stream and the side stream of MFHE_OPT_HE_STREAMS) at the
    // matrix transforms' size, so no W-CRT call allocates afterwards
    if (c->wcrt_mfma && c->wD) {
        const Geo2 g = geo(c);
        ModGemmArgs a;
        a.P = (uint32_t)g.n2;
        a.aL = 512ull * 512;
        RC(use_mfma(c, a, c->d_wV, g.L, 0));
        RC(use_mfma(c, a, c->d_wV, g.L, 1));
    }
    return he_side_stream(c);
}

extern "C" int mfhe_encode(mfhe_ctx* c, const double* msg, uint64_t* re, uint64_t* im, mfhe_stream_t s) {
    return encode_impl(c, msg, re, im, (hipStream_t)s);
}
extern "C" int mfhe_decode(mfhe_ctx* c, const uint64_t* re, const uint64_t* im, double* msg, mfhe_stream_t s) {
    return decode_impl(c, re, im, msg, (hipStream_t)s);
}
extern "C" int mfhe_keygen(mfhe_ctx* c, uint64_t* sk, mfhe_stream_t s) { return keygen_impl(c, sk, (hipStream_t)s); }
extern "C" int mfhe_encrypt(mfhe_ctx* c, const uint64_t* m, const uint64_t* sk, uint64_t* ct, mfhe_stream_t s) {
    return encrypt_impl(c, m, nullptr, sk, ct, nullptr, (hipStream_t)s);
}
extern "C" int mfhe_encrypt_pair(mfhe_ctx* c, const uint64_t* mre, const uint64_t* mim, const uint64_t* sk,
                                 uint64_t* cre, uint64_t* cim, mfhe_stream_t s) {
    if (!mim || !cim) return set_error(MFHE_EINVAL, "mfhe_encrypt_pair: null pointer");
    return encrypt_impl(c, mre, mim, sk, cre, cim, (hipStream_t)s);
}
extern "C" int mfhe_decrypt_to_eval(mfhe_ctx* c, const uint64_t* ct, const uint64_t* sk, uint64_t* out,
                                    mfhe_stream_t s) {
    RC(need_wcrt(c));
    RC(need_xntt(c, "decrypt"));
    if (!ct || !sk || !out) return set_error(MFHE_EINVAL, "mfhe_decrypt_to_eval: null pointer");
    RC(ensure_ws(c));
    Bump b{(char*)c->ws};
    return decrypt_impl(c, ct, sk, out, (hipStream_t)s, &b);
}
extern "C" int mfhe_decrypt_and_decode(mfhe_ctx* c, const uint64_t* cre, const uint64_t* cim, const uint64_t* sk,
                                       double* msg, mfhe_stream_t s) {
    RC(need_wcrt(c));
    RC(need_xntt(c, "decrypt"));
    if (!cre || !cim || !sk || !msg) return set_error(MFHE_EINVAL, "mfhe_decrypt_and_decode: null pointer");
    RC(ensure_ws(c));
    Bump b{(char*)c->ws};
    RingArgs ra;
    const RingArgs* dec;
    RC(decrypt_pair(c, cre, cim, sk, (hipStream_t)s, &b, ra, dec));
    return decode_impl(c, cre, cim, msg, (hipStream_t)s, &b, dec);
}

// Every argument check of a sharded decode, run by each rank on its own arguments.
static int sharded_args(mfhe_ctx* c, mfhe_ctx* call, mfhe_comm* comm, const void* a, const void* b, const void* m) {
    RC(need_wcrt(c));
    if (!call || !a || !b || !m) return set_error(MFHE_EINVAL, "sharded decode: null pointer");
    if (call->N != c->N) return set_error(MFHE_EINVAL, "sharded decode: ctx_all has another ring degree");
    // the compose divides by ctx_all's delta: another scale would give silently wrong messages
    if (call->delta != c->delta) return set_error(MFHE_EINVAL, "sharded decode: ctx_all has another scale (delta)");
    int G = 1, rank = 0;
    RC(comm_size_rank(comm, &G, &rank));
    if (512 % G) return set_error(MFHE_EINVAL, "sharded decode: the communicator size must divide 512 lanes");
    if (call->L != (c->limbs_total ? c->limbs_total : c->L) || call->L != c->L * G)
        return set_error(MFHE_EINVAL, "sharded decode: ctx_all must hold the G * L_shard moduli of the whole set");
    // the exchange layout puts rank g's limbs at [g L, (g + 1) L) of ctx_all: the shard must be exactly that
    if (c->limb_base != rank * c->L)
        return set_error(MFHE_EINVAL, "sharded decode: this rank's shard must start at limb rank * L_shard "
                                      "(mfhe_ctx_set_limb_shard)");
    for (int k = 0; k < c->L; ++k)
        if (call->moduli[(size_t)(rank * c->L + k)] != c->moduli[(size_t)k])
            return set_error(MFHE_EINVAL, "sharded decode: the shard's moduli differ from ctx_all's limbs rank * L_shard..");
    RC(ensure_xy(c));
    return ensure_ws(c);
}
extern "C" int mfhe_decode_sharded(mfhe_ctx* c, mfhe_ctx* call, mfhe_comm* comm, int mode, const uint64_t* re,
                                   const uint64_t* im, double* msg, mfhe_stream_t s) {
    if (!comm) return set_error(MFHE_EINVAL, "sharded decode: null communicator");
    // the ranks agree on the verdict before any collective: one rank's bad arguments fail every rank instead of
    // leaving the others blocked in the exchange
    RC(comm_agree(comm, sharded_args(c, call, comm, re, im, msg), (hipStream_t)s));
    Bump b{(char*)c->ws};
    return decode_sharded_impl(c, call, comm, mode, re, im, msg, (hipStream_t)s, &b);
}
extern "C" int mfhe_decrypt_and_decode_sharded(mfhe_ctx* c, mfhe_ctx* call, mfhe_comm* comm, int mode,
                                               const uint64_t* cre, const uint64_t* cim, const uint64_t* sk, double* msg,
                                               mfhe_stream_t s) {
    if (!comm) return set_error(MFHE_EINVAL, "sharded decode: null communicator");
    int rc = sharded_args(c, call, comm, cre, cim, msg);
    if (!rc) rc = need_xntt(c, "decrypt");
    if (!rc && !sk) rc = set_error(MFHE_EINVAL, "sharded decrypt: null key");
    RC(comm_agree(comm, rc, (hipStream_t)s));
    Bump b{(char*)c->ws};
    RingArgs ra;
    const RingArgs* dec;
    RC(decrypt_pair(c, cre, cim, sk, (hipStream_t)s, &b, ra, dec));
    return decode_sharded_impl(c, call, comm, mode, cre, cim, msg, (hipStream_t)s, &b, dec);
}

extern "C" int mfhe_ct_add(mfhe_ctx* c, const uint64_t* x, const uint64_t* y, uint64_t* r, mfhe_stream_t s) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (!x || !y || !r) return set_error(MFHE_EINVAL, "mfhe_ct_add: null pointer");
    const Geo2 g = geo(c);
    hipLaunchKernelGGL(ct_add_kernel, g1(2 * g.words), dim3(256), 0, (hipStream_t)s, x, y, r, c->d_rns_mu, g.L,
                       2 * g.logn, g.words);
    MFHE_CHECK_LAUNCH("ct_add_kernel");
    return MFHE_OK;
}
extern "C" int mfhe_ct_mul_tensor(mfhe_ctx* c, const uint64_t* x, const uint64_t* y, uint64_t* d0, uint64_t* d1,
                                  uint64_t* d2, mfhe_stream_t s) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (!x || !y || !d0 || !d1 || !d2) return set_error(MFHE_EINVAL, "mfhe_ct_mul_tensor: null pointer");
    const Geo2 g = geo(c);
    hipLaunchKernelGGL(ct_mul_kernel, g1(g.words), dim3(256), 0, (hipStream_t)s, x, y, d0, d1, d2, c->d_rns_mu,
                       c->d_r64, g.L, 2 * g.logn, g.words);
    MFHE_CHECK_LAUNCH("ct_mul_kernel");
    return MFHE_OK;
}

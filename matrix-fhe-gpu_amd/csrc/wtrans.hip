// wtrans.hip -- the W-axis transforms (W-CRT over the RNS limbs, complex W-DFT), the per-lane XY encoder transforms
// and the matrix-major <-> poly-major layouts at reference geometry, with their entry points (pipelines: he.hip).
//
// Reference: src/core/HE.cu (W-CRT 437-470, 716-781, 1029-1114, 1245-1270; layouts 1330-1368),
// src/core/batched_encoder.cu:161-228, src/core/encoder.cu:425-501.  Differences by design: he.hip.
#include "wtrans.hpp"

#include "cdft.hpp"
#include "ring_row.hpp"

namespace mfhe {

// ---------------- layouts: HE.cu:1330-1368 ----------------
template <bool TO_POLY>
__global__ void layout_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int log_n, int L,
                              uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;   // matrix-major index
    if (i >= total) return;
    const uint64_t p = pm_index(i, log_n, L);
    if (TO_POLY) out[p] = in[i];
    else out[i] = in[p];
}

// centred int64 -> RNS matrix-major (centered_int_to_rns_matrix_kernel HE.cu:815-835)
__global__ void centered_to_rns_kernel(const int64_t* in, uint64_t* out, const uint64_t* qmu, int L, uint64_t n2,
                                       uint64_t total) {
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t pos = idx % n2, t = idx / n2;
    const int l = (int)(t % L);
    const uint64_t w = t / L;
    const int64_t v = in[w * n2 + pos];
    const int64_t q = (int64_t)qmu[2 * l];
    int64_t r = v % q;
    if (r < 0) r += q;
    out[idx] = (uint64_t)r;
}

// he_big_to_i64_checked HE.cu:904-915 over compose output
__global__ void big_to_i64_kernel(const uint64_t* mag, const uint8_t* neg, int W, int64_t* out, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    bool over = mag[i * W] > (uint64_t)INT64_MAX;
    for (int k = 1; k < W; ++k) over |= mag[i * W + k] != 0;
    const bool ng = neg[i] != 0;
    out[i] = over ? (ng ? INT64_MIN : INT64_MAX) : (ng ? -(int64_t)mag[i * W] : (int64_t)mag[i * W]);
}

// limb-0 centring after the inverse (HE.cu:1112-1113)
__global__ void center_limb0_kernel(const uint64_t* in, int64_t* out, uint64_t q, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t a = in[i];
    out[i] = (a > (q >> 1)) ? (int64_t)a - (int64_t)q : (int64_t)a;
}

// planar <-> interleaved complex for the split re/im W-DFT entry points (HE.cu:472-502)
__global__ void pack_i64_pair_kernel(const int64_t* re, const int64_t* im, double2* out, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < total) out[i] = make_double2((double)re[i], (double)im[i]);
}
__global__ void pack_f64_pair_kernel(const double* re, const double* im, double2* out, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < total) out[i] = make_double2(re[i], im[i]);
}
__global__ void unpack_pair_kernel(const double2* in, double* re, double* im, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < total) {
        const double2 v = in[i];
        re[i] = v.x;
        im[i] = v.y;
    }
}

// ---------------- helpers ----------------
int need_wcrt(const mfhe_ctx* c) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (!(c->conv & MFHE_CONV_WCRT)) return set_error(MFHE_ENOTREADY, "context was created without MFHE_CONV_WCRT");
    return MFHE_OK;
}

Geo2 geo(const mfhe_ctx* c) {
    const uint64_t n2 = c->N * c->N;
    return {.L = c->L, .logn = c->logN, .n = c->N, .n2 = n2, .words = (uint64_t)mfhe_ctx::PHI * c->L * n2,
            .cnt = (uint64_t)mfhe_ctx::PHI * n2};
}

static size_t ws_need(const mfhe_ctx* c) {
    const Geo2 g = geo(c);
    return 10 * g.words * 8 + g.cnt * (size_t)c->W * 8 + 4 * g.cnt * 16 + 2 * g.cnt + (64 << 10);
}

int ensure_ws(mfhe_ctx* c) { return grow_ws(c, ws_need(c)); }

// leaves a on the VALU kernel when the MFMA operands are unavailable
int use_mfma(mfhe_ctx* c, ModGemmArgs& a, const uint64_t* A, int L, int slot) {
    if (!c->wcrt_mfma || !c->wD || (A != c->d_wV && A != c->d_wVinv)) return MFHE_OK;
    void*& ws = slot ? c->gemm_ws2 : c->gemm_ws;
    RC(grow_dev(ws, slot ? c->gemm_ws2_bytes : c->gemm_ws_bytes, mod_gemm_mfma_ws(a.P, L, c->wD)));
    a.Adig = A == c->d_wV ? c->d_wVdig : c->d_wVidig;
    a.adL = a.aL ? (uint64_t)c->wD * 512 * 512 : 0;
    a.D = c->wD;
    a.rtab = c->d_wrtab;
    a.Bdig = (int8_t*)ws;
    // a.aL == 0: one A shared by every limb (vector transforms) -> every limb uses the full digit count
    a.limbD = (a.aL && (int)c->wDl.size() == L) ? c->wDl.data() : nullptr;
    a.epi = c->d_wepi;
    a.lds_stage = c->wcrt_mfma != 2;
    a.pipe = c->wcrt_pipe;
    // mode 1: the forward transform of a per-limb V runs factored (half the MACs, wcrt_digitize.hpp)
    if (c->wcrt_mfma == 1 && A == c->d_wV && a.aL && c->d_wZdig && a.epi) {
        a.Adig = c->d_wZdig;
        a.adL = (uint64_t)c->wD * 256 * 256;
        a.fold = c->d_wfold;
    }
    // ... and the inverse of a per-limb V^-1 (interpolation through 771 = 3 x 257, reduced mod Phi_771)
    if (c->wcrt_mfma == 1 && A == c->d_wVinv && a.aL && c->d_wZidig && a.epi) {
        a.Adig = c->d_wZidig;
        a.adL = (uint64_t)c->wD * 256 * 256;
        a.ifold = c->d_wifold;
        a.iz = c->d_wiz;
        a.phi = c->d_wphi;
    }
    return MFHE_OK;
}

bool quant_fused_ok(const mfhe_ctx* c) {
    return c->wcrt_mfma == 1 && c->wD && c->d_wZdig && c->d_wepi && c->d_wfold;
}

int wcrt_args(mfhe_ctx* c, ModGemmArgs& a, const WcrtReq& r) {
    const Geo2 g = geo(c);
    a.A = r.A;
    a.aL = 512ull * 512;
    a.M = a.K = 512;
    a.qmu = c->d_rns_mu;
    a.r64 = c->d_r64;
    a.B = r.B;
    a.C = r.C;
    a.C2 = r.C2;
    a.log_n = g.logn;
    if (r.vector) {
        a.P = (uint32_t)g.n;
        a.bL = g.n; a.sbK = (uint64_t)g.L * g.n; a.sbY = 0;
        a.cL = g.n; a.scM = (uint64_t)g.L * g.n; a.scY = 0;
    } else {
        a.P = (uint32_t)g.n2;
        if (r.b_poly) { a.bL = g.n; a.sbK = g.n * g.L * g.n; a.sbY = (uint64_t)g.L * g.n; }
        else { a.bL = g.n2; a.sbK = (uint64_t)g.L * g.n2; a.sbY = g.n; }
        if (r.out == WOut::Poly) { a.cL = g.n; a.scM = g.n * g.L * g.n; a.scY = (uint64_t)g.L * g.n; }
        else { a.cL = g.n2; a.scM = (uint64_t)g.L * g.n2; a.scY = g.n; }
    }
    RC(use_mfma(c, a, r.A, g.L, r.slot));
    if (r.C2 && !a.fold) return set_error(MFHE_EINVAL, "W-CRT: a second output needs the factored forward");
    if (r.dec) {
        // B is the ciphertext: the factored inverse's digitize decrypts it row by row (wcrt_digitize.hpp
        // mfma_digitize_ifold_dec_kernel)
        if (!a.ifold) return set_error(MFHE_EINVAL, "W-CRT: a decrypt-fused source needs the factored inverse");
        a.dct = r.B;
        a.dtotal = g.words;
        a.dsk = r.dec->sk;
        a.dlf = r.dec->lf;
        a.dtw = r.dec->tw;
        a.ditw = r.dec->itw;
        a.dninv = r.dec->ninv;
    }
    if (r.src != WSrc::None) {
        if (!a.fold) return set_error(MFHE_EINVAL, "W-CRT: a fused digitize source needs the factored forward");
        a.qsrc = (int)r.src;
        a.qf = r.qf;
        a.qf_row = g.n2 * r.step;
        a.qf_step = r.step;
        a.delta = c->delta;
        a.lbase = c->limb_base;
        a.Ltot = c->limbs_total ? c->limbs_total : g.L;
    }
    return MFHE_OK;
}
int wcrt_gemm(mfhe_ctx* c, const WcrtReq& r, hipStream_t s) {
    ModGemmArgs a;
    RC(wcrt_args(c, a, r));
    return launch_mod_gemm(a, c->L, s);
}

// MFHE_OPT_CGEMM_MFMA = 2 (default): factored through 771 = 3 x 257 (cdft.hip cgemm_mfma_kernel<1 / 2>), half the flops
// of the dense 512 x 512 product
bool wdft_planar_ok(const mfhe_ctx* c) { return c->cgemm_mfma >= 2 && c->d_wdZ; }
int wdft(mfhe_ctx* c, const double2* A, const double2* in, double2* out, hipStream_t s, bool planar) {
    const Geo2 g = geo(c);
    if (planar && !(wdft_planar_ok(c) && A == c->d_wdVinv))
        return set_error(MFHE_EINVAL, "wdft: planar output needs the factored W-IDFT");
    if (c->cgemm_mfma >= 2 && c->d_wdZ && (A == c->d_wdV || A == c->d_wdVinv)) {
        CGemmArgs f;
        f.mfma = true;
        f.B = in;
        f.C = out;
        f.aB = f.bB = f.cB = 0;
        f.M = f.K = 256;
        f.Pf = (uint32_t)g.n2;
        f.P = 2 * f.Pf;
        f.scM = g.n2;
        if (A == c->d_wdV) {
            // mode 2: the 257-point DFTs by Rader's algorithm (cdft.hip wdft_rader_kernel, r06); 3: the GEMM
            if (c->cgemm_mfma == 2 && c->d_wdrad && in != out)
                return launch_wdft_rader(in, out, (uint32_t)g.n2, c->d_wdrad, c->d_wdgp, s);
            f.fac = 1;
            f.A = c->d_wdZ;
            return launch_cgemm(f, 1, s);
        }
        if (c->cgemm_mfma == 2 && c->d_wdrad && in != out)   // Rader (cdft.hip wdft_rader_inv_kernel, r06)
            return launch_wdft_rader_inv(in, out, planar ? (double*)out + 512ull * g.n2 : nullptr, (uint32_t)g.n2,
                                         c->d_wdrad + 256, c->d_wdgp, c->d_wdlam, c->d_wdphi, s);
        RC(grow_dev(c->wd_ws, c->wd_ws_bytes, (size_t)g.n2 * 2 * sizeof(double2)));
        f.fac = 2;
        if (planar) f.Cim = (double*)out + 512ull * g.n2;
        f.A = c->d_wdZi;
        f.cc = (const double2*)c->wd_ws;
        f.lam = c->d_wdlam;
        f.phi = c->d_wdphi;
        RC(launch_cwdft_inv_dots(f, in, c->d_wdxp, s));
        return launch_cgemm(f, 1, s);
    }
    CGemmArgs a;
    a.mfma = c->cgemm_mfma != 0;
    a.A = A; a.B = in; a.C = out;
    a.aB = a.bB = a.cB = 0;
    a.M = a.K = 512;
    a.P = (uint32_t)g.n2;
    a.log_n = 2 * g.logn;
    a.sbK = g.n2; a.sbY = 0; a.scM = g.n2; a.scY = 0;
    return launch_cgemm(a, 1, s);
}

int xy3(const mfhe_ctx* c, const double2* A, const double2* in, const double2* B, double2* tmp, double2* out,
        size_t lanes, hipStream_t s) {
    const Geo2 g = geo(c);
    // n = 64: mode 2 by 64-point FFTs (cdft.hip xy_fft_kernel, equal to rounding); mode 3 both GEMMs in one launch
    // (cdft.hip xy_fused_kernel), the same doubles as the two launches of mode 1
    if (c->cgemm_mfma == 2 && g.n == 64) {
        if (A == c->d_encV && B == c->d_encVT) return launch_xy_fft(in, out, false, (int)lanes, s);
        if (A == c->d_encVi && B == c->d_encViT) return launch_xy_fft(in, out, true, (int)lanes, s);
    }
    if (c->cgemm_mfma >= 2 && g.n == 64 && in != out) return launch_xy_fused(A, in, B, out, (int)lanes, s);
    CGemmArgs a;
    a.mfma = c->cgemm_mfma != 0;
    a.M = a.K = (int)g.n;
    a.P = (uint32_t)g.n;
    a.log_n = g.logn;
    a.sbK = g.n; a.sbY = 0; a.scM = g.n; a.scY = 0;
    a.A = A; a.aB = 0; a.B = in; a.bB = g.n2; a.C = tmp; a.cB = g.n2;        // T = A M
    int rc = launch_cgemm(a, (int)lanes, s);
    if (rc) return rc;
    a.A = tmp; a.aB = g.n2; a.B = B; a.bB = 0; a.C = out; a.cB = g.n2;       // out = T B
    return launch_cgemm(a, (int)lanes, s);
}

int layout(const mfhe_ctx* c, const uint64_t* in, uint64_t* out, bool to_poly, hipStream_t s) {
    const Geo2 g = geo(c);
    if (to_poly) hipLaunchKernelGGL(layout_kernel<true>, g1(g.words), dim3(256), 0, s, in, out, g.logn, g.L, g.words);
    else hipLaunchKernelGGL(layout_kernel<false>, g1(g.words), dim3(256), 0, s, in, out, g.logn, g.L, g.words);
    MFHE_CHECK_LAUNCH("layout_kernel");
    return MFHE_OK;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_wcrt_fwd(mfhe_ctx* c, const uint64_t* in, uint64_t* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out) return set_error(MFHE_EINVAL, "mfhe_wcrt_fwd: null pointer");
    return wcrt_gemm(c, {.A = c->d_wV, .B = in, .C = out, .out = WOut::Poly}, (hipStream_t)s);
}
extern "C" int mfhe_wcrt_inv(mfhe_ctx* c, const uint64_t* in, uint64_t* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out) return set_error(MFHE_EINVAL, "mfhe_wcrt_inv: null pointer");
    return wcrt_gemm(c, {.A = c->d_wVinv, .B = in, .b_poly = true, .C = out, .out = WOut::Matrix}, (hipStream_t)s);
}
extern "C" int mfhe_wcrt_fwd_vector(mfhe_ctx* c, const uint64_t* in, uint64_t* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out) return set_error(MFHE_EINVAL, "mfhe_wcrt_fwd_vector: null pointer");
    return wcrt_gemm(c, {.A = c->d_wV, .B = in, .C = out, .out = WOut::Vector, .vector = true}, (hipStream_t)s);
}

extern "C" int mfhe_wcrt_fwd_centered(mfhe_ctx* c, const int64_t* in, int64_t* out, mfhe_stream_t s_) {
    RC(need_wcrt(c));
    if (!in || !out) return set_error(MFHE_EINVAL, "mfhe_wcrt_fwd_centered: null pointer");
    RC(ensure_ws(c));
    hipStream_t s = (hipStream_t)s_;
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    uint64_t* rns = b.get<uint64_t>(g.words);
    uint64_t* ev = b.get<uint64_t>(g.words);
    uint64_t* mag = b.get<uint64_t>(g.cnt * c->W);
    uint8_t* neg = b.get<uint8_t>(g.cnt);
    hipLaunchKernelGGL(centered_to_rns_kernel, g1(g.words), dim3(256), 0, s, in, rns, c->d_rns_mu, g.L, g.n2, g.words);
    MFHE_CHECK_LAUNCH("centered_to_rns_kernel");
    RC(wcrt_gemm(c, {.A = c->d_wV, .B = rns, .C = ev, .out = WOut::Matrix}, s));
    RC(mfhe_crt_compose(c, ev, 512, g.n2, mag, neg, s_));
    hipLaunchKernelGGL(big_to_i64_kernel, g1(g.cnt), dim3(256), 0, s, mag, neg, c->W, out, g.cnt);
    MFHE_CHECK_LAUNCH("big_to_i64_kernel");
    return MFHE_OK;
}

extern "C" int mfhe_wcrt_inv_centered(mfhe_ctx* c, const int64_t* in, int64_t* out, mfhe_stream_t s_) {
    RC(need_wcrt(c));
    if (!in || !out) return set_error(MFHE_EINVAL, "mfhe_wcrt_inv_centered: null pointer");
    RC(ensure_ws(c));
    hipStream_t s = (hipStream_t)s_;
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    uint64_t* rns = b.get<uint64_t>(g.cnt);
    uint64_t* co = b.get<uint64_t>(g.cnt);
    // limb 0 only (HE.cu:1101): treat the input as a 1-limb matrix-major array
    hipLaunchKernelGGL(centered_to_rns_kernel, g1(g.cnt), dim3(256), 0, s, in, rns, c->d_rns_mu, 1, g.n2, g.cnt);
    MFHE_CHECK_LAUNCH("centered_to_rns_kernel");
    ModGemmArgs a;
    a.A = c->d_wVinv; a.aL = 0; a.M = a.K = 512; a.qmu = c->d_rns_mu; a.r64 = c->d_r64;
    a.B = rns; a.bL = 0; a.sbK = g.n2; a.sbY = g.n; a.log_n = g.logn; a.P = (uint32_t)g.n2;
    a.C = co; a.cL = 0; a.scM = g.n2; a.scY = g.n;
    RC(use_mfma(c, a, c->d_wVinv, 1));
    RC(launch_mod_gemm(a, 1, s));
    hipLaunchKernelGGL(center_limb0_kernel, g1(g.cnt), dim3(256), 0, s, co, out, c->moduli[0], g.cnt);
    MFHE_CHECK_LAUNCH("center_limb0_kernel");
    return MFHE_OK;
}

extern "C" int mfhe_wdft_fwd(mfhe_ctx* c, const double* in, double* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out || in == out) return set_error(MFHE_EINVAL, "mfhe_wdft_fwd: need distinct in/out");
    return wdft(c, c->d_wdV, (const double2*)in, (double2*)out, (hipStream_t)s);
}
extern "C" int mfhe_wdft_inv(mfhe_ctx* c, const double* in, double* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out || in == out) return set_error(MFHE_EINVAL, "mfhe_wdft_inv: need distinct in/out");
    return wdft(c, c->d_wdVinv, (const double2*)in, (double2*)out, (hipStream_t)s);
}

static int wdft_pair(mfhe_ctx* c, const void* re, const void* im, bool i64, double* ore, double* oim, bool inv,
                     hipStream_t s) {
    RC(need_wcrt(c));
    if (!re || !im || !ore || !oim) return set_error(MFHE_EINVAL, "mfhe_wdft_*_pair: null pointer");
    RC(ensure_ws(c));
    const Geo2 g = geo(c);
    Bump b{(char*)c->ws};
    double2* x = b.get<double2>(g.cnt);
    double2* y = b.get<double2>(g.cnt);
    if (i64)
        hipLaunchKernelGGL(pack_i64_pair_kernel, g1(g.cnt), dim3(256), 0, s, (const int64_t*)re, (const int64_t*)im, x,
                           g.cnt);
    else
        hipLaunchKernelGGL(pack_f64_pair_kernel, g1(g.cnt), dim3(256), 0, s, (const double*)re, (const double*)im, x,
                           g.cnt);
    MFHE_CHECK_LAUNCH("pack_pair_kernel");
    RC(wdft(c, inv ? c->d_wdVinv : c->d_wdV, x, y, s));
    hipLaunchKernelGGL(unpack_pair_kernel, g1(g.cnt), dim3(256), 0, s, y, ore, oim, g.cnt);
    MFHE_CHECK_LAUNCH("unpack_pair_kernel");
    return MFHE_OK;
}
extern "C" int mfhe_wdft_fwd_pair_i64(mfhe_ctx* c, const int64_t* re, const int64_t* im, double* ore, double* oim,
                                      mfhe_stream_t s) {
    return wdft_pair(c, re, im, true, ore, oim, false, (hipStream_t)s);
}
extern "C" int mfhe_wdft_inv_pair(mfhe_ctx* c, const double* re, const double* im, double* ore, double* oim,
                                  mfhe_stream_t s) {
    return wdft_pair(c, re, im, false, ore, oim, true, (hipStream_t)s);
}

static int xy_entry(mfhe_ctx* c, const double* in, double* out, size_t lanes, mfhe_stream_t s, bool inv) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (lanes == 0) return MFHE_OK;
    if (!in || !out || in == out) return set_error(MFHE_EINVAL, "mfhe_xy_(i)dft: need distinct in/out");
    if (lanes > 65535) return set_error(MFHE_EINVAL, "mfhe_xy_(i)dft: at most 65535 lanes per call");
    RC(ensure_xy(c));
    RC(ensure_ws(c));
    double2* tmp = (double2*)c->ws;
    const Geo2 g = geo(c);
    if (lanes * g.n2 * 16 > c->ws_bytes) return set_error(MFHE_EINVAL, "too many lanes for the workspace");
    return inv ? xy3(c, c->d_encVi, (const double2*)in, c->d_encViT, tmp, (double2*)out, lanes, (hipStream_t)s)
               : xy3(c, c->d_encV, (const double2*)in, c->d_encVT, tmp, (double2*)out, lanes, (hipStream_t)s);
}
extern "C" int mfhe_xy_idft(mfhe_ctx* c, const double* in, double* out, size_t lanes, mfhe_stream_t s) {
    return xy_entry(c, in, out, lanes, s, true);
}
extern "C" int mfhe_xy_dft(mfhe_ctx* c, const double* in, double* out, size_t lanes, mfhe_stream_t s) {
    return xy_entry(c, in, out, lanes, s, false);
}

extern "C" int mfhe_matrix_to_poly(mfhe_ctx* c, const uint64_t* in, uint64_t* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out || in == out) return set_error(MFHE_EINVAL, "layout needs distinct in/out");
    return layout(c, in, out, true, (hipStream_t)s);
}
extern "C" int mfhe_poly_to_matrix(mfhe_ctx* c, const uint64_t* in, uint64_t* out, mfhe_stream_t s) {
    RC(need_wcrt(c));
    if (!in || !out || in == out) return set_error(MFHE_EINVAL, "layout needs distinct in/out");
    return layout(c, in, out, false, (hipStream_t)s);
}

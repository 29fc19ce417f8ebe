// bconv.hip -- RNS basis conversion for gfx950: fast / centred base conversion, ModUp, ModDown and rescale.
//
// For a source range with moduli s_i (product S) and canonical residues x_i, y_i = [x_i (S/s_i)^-1]_(s_i) and
//   FAST     : out_j = (sum_i y_i (S/s_i)) mod d_j                       = (x + u S) mod d_j, 0 <= u < ns
//   CENTERED : v = rint(sum_i (double)y_i (1/s_i)) in ascending i, out_j = (sum_i y_i c_ij - v (S mod d_j)) mod d_j,
//              the centred value of x mod d_j
//   MODDOWN  : out_j = (x_j - centred_j) S^-1 mod d_j on the kept limbs, the centred conversion staying in registers
//
// Design: one thread per coefficient (two with 16-byte loads and stores when the layout allows, as
// rns_decompose_x2_kernel), the ns source residues loaded once and turned into y_i in registers (ns <= kBconvUnroll,
// template-unrolled; longer sources are re-read per destination limb, from the cache), then one pass over the
// destination limbs: a u128 sum of ns products (< 2^124 each, so 16 fit; longer sources reduce every 16 terms) and
// one 128-bit Barrett reduction with the DModulus constants of d_dmod.  Per-limb constants are wave-uniform.
#include "bconv.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

#include "host_math.hpp"
#include "mod128.hpp"

namespace mfhe {

// largest template-unrolled source count: 16 y values (32 VGPRs) at two coefficients, every instantiation at
// <= 63 VGPRs and 8 waves/SIMD (compiler resource usage)
constexpr int kBconvUnroll = 8;

__device__ __forceinline__ double bits_to_f64(uint64_t b) { return __longlong_as_double((long long)b); }

// NS: source count (template-unrolled) or 0 (generic loop over a.ns); V: coefficients per thread; MODE: kBconv*.
// `in` and `out` may be the same buffer (ModDown in place): a thread reads the kept residue it overwrites first, and
// source rows are never written, so neither pointer is __restrict__.  The tables (t0 .. t2: a.r[k].tab) and dmod are
// __restrict__ kernel parameters: only then are they known not to alias the stores, and read as wave-uniform scalars.
template <int NS, int V, int MODE>
__global__ __launch_bounds__(256) void bconv_kernel(BconvArgs a, const uint64_t* __restrict__ t0,
                                                    const uint64_t* __restrict__ t1, const uint64_t* __restrict__ t2,
                                                    const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (idx >= a.total) return;
    uint64_t p, c;
    if (a.lg >= 0) {
        p = idx >> a.lg;
        c = idx & (a.ncoeff - 1);
    } else {
        p = idx / a.ncoeff;
        c = idx - p * a.ncoeff;
    }
    const T* in = (const T*)a.in + p * a.in_stride + c;
    T* out = (T*)a.out + p * a.out_stride + c;
    const T* src = in + (uint64_t)a.src_row * a.ncoeff;
    const int ns = NS ? NS : a.ns;
    const uint64_t* st = t0;   // source section (the same in every range's table)

    constexpr int NY = NS ? NS : 1;
    uint64_t y[NY][V];
    double est[V];
#pragma unroll
    for (int k = 0; k < V; ++k) est[k] = 0.0;
    if (NS) {
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            uint64_t x[V];
            Lane<V>::load(src + (uint64_t)i * a.ncoeff, x);
            if (a.copy_row >= 0) Lane<V>::store(out + (uint64_t)(a.copy_row + i) * a.ncoeff, x);
            const uint64_t s = st[4 * i], w = st[4 * i + 1], ws = st[4 * i + 2];
            const double sinv = bits_to_f64(st[4 * i + 3]);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                y[i][k] = shoup_mul(x[k], w, ws, s);
                if (MODE != kBconvFast) est[k] += (double)y[i][k] * sinv;
            }
        }
    } else if (MODE != kBconvFast || a.copy_row >= 0) {
        for (int i = 0; i < ns; ++i) {
            uint64_t x[V];
            Lane<V>::load(src + (uint64_t)i * a.ncoeff, x);
            if (a.copy_row >= 0) Lane<V>::store(out + (uint64_t)(a.copy_row + i) * a.ncoeff, x);
            if (MODE != kBconvFast) {
                const uint64_t s = st[4 * i], w = st[4 * i + 1], ws = st[4 * i + 2];
                const double sinv = bits_to_f64(st[4 * i + 3]);
#pragma unroll
                for (int k = 0; k < V; ++k) est[k] += (double)shoup_mul(x[k], w, ws, s) * sinv;
            }
        }
    }
    uint64_t v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = MODE != kBconvFast ? (uint64_t)__builtin_rint(est[k]) : 0;

#pragma unroll
    for (int rk = 0; rk < 3; ++rk) {
        if (rk >= a.nr) break;
        const BconvRange R = a.r[rk];
        const uint64_t* dt = (rk == 0 ? t0 : rk == 1 ? t1 : t2) + (uint64_t)kBconvSrcWords * ns;
        for (int j = 0; j < R.count; ++j) {
            const uint64_t* h = dt + (uint64_t)j * (kBconvDstHead + ns);
            const uint64_t* dm = dmod + 3 * (uint64_t)(R.limb + j);
            const uint64_t q = dm[0], r0 = dm[1], r1 = dm[2];
            uint64_t res[V];
            if (NS) {
                u128 acc[V];
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] = 0;
#pragma unroll
                for (int i = 0; i < NY; ++i) {
                    const uint64_t cij = h[kBconvDstHead + i];
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] += (u128)y[i][k] * cij;
                }
#pragma unroll
                for (int k = 0; k < V; ++k) res[k] = barrett128(acc[k], q, r0, r1);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) res[k] = 0;
                for (int i0 = 0; i0 < ns; i0 += 16) {   // 16 products < 2^124 and a residue < 2^62 fit a u128
                    u128 acc[V];
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] = res[k];
                    const int i1 = i0 + 16 < ns ? i0 + 16 : ns;
                    for (int i = i0; i < i1; ++i) {
                        uint64_t x[V];
                        Lane<V>::load(src + (uint64_t)i * a.ncoeff, x);
                        const uint64_t s = st[4 * i], w = st[4 * i + 1], ws = st[4 * i + 2];
                        const uint64_t cij = h[kBconvDstHead + i];
#pragma unroll
                        for (int k = 0; k < V; ++k) acc[k] += (u128)shoup_mul(x[k], w, ws, s) * cij;
                    }
#pragma unroll
                    for (int k = 0; k < V; ++k) res[k] = barrett128(acc[k], q, r0, r1);
                }
            }
            if (MODE != kBconvFast) {
                const uint64_t negS = h[0];
#pragma unroll
                for (int k = 0; k < V; ++k) res[k] = barrett128((u128)v[k] * negS + res[k], q, r0, r1);
            }
            T* o = out + (uint64_t)(R.row + j) * a.ncoeff;
            if (MODE == kBconvModDown) {
                const uint64_t pinv = h[1], pinvs = h[2];
                uint64_t x[V];
                Lane<V>::load(in + (uint64_t)(R.row + j) * a.ncoeff, x);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const uint64_t t = x[k] >= res[k] ? x[k] - res[k] : x[k] + q - res[k];
                    res[k] = shoup_mul(t, pinv, pinvs, q);
                }
            }
            Lane<V>::store(o, res);
        }
    }
}

// words contiguous words of every polynomial: dst[p * dst_stride + w] = src[p * src_stride + w]
__global__ __launch_bounds__(256) void bconv_copy_rows_kernel(const uint64_t* __restrict__ src, uint64_t src_stride,
                                                              uint64_t* __restrict__ dst, uint64_t dst_stride,
                                                              uint64_t words, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t p = i / words, w = i - p * words;
    dst[p * dst_stride + w] = src[p * src_stride + w];
}

// ModDown tail in the evaluation domain: out[p][j][c] = (in[p][j][c] - r[p][j][c]) P^-1 mod q_j, j < keep;
// r [npoly][keep][N], r_stride words per polynomial.  out may equal in.  add (may be null, may equal out): the same
// layout as out, added to the result mod q_j (the key switch's MFHE_KS_ADD).
__global__ __launch_bounds__(256) void bconv_sub_scale_kernel(const uint64_t* in, uint64_t in_stride,
                                                              const uint64_t* __restrict__ r, uint64_t r_stride,
                                                              uint64_t* out, uint64_t out_stride, const uint64_t* add,
                                                              int keep, int logN, int ns,
                                                              const uint64_t* __restrict__ tab,
                                                              const uint64_t* __restrict__ dmod, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t row = i >> logN, c = i & ((1ull << logN) - 1);
    const uint64_t p = row / (uint64_t)keep, j = row - p * (uint64_t)keep;
    const uint64_t* h = tab + (uint64_t)kBconvSrcWords * ns + j * (uint64_t)(kBconvDstHead + ns);
    const uint64_t q = dmod[3 * j];
    const uint64_t off = (j << logN) + c;
    const uint64_t x = in[p * in_stride + off], rr = r[p * r_stride + off];
    const uint64_t t = x >= rr ? x - rr : x + q - rr;
    uint64_t v = shoup_mul(t, h[1], h[2], q);
    if (add) {
        v += add[p * out_stride + off];
        v = v >= q ? v - q : v;
    }
    out[p * out_stride + off] = v;
}

int bconv_table(mfhe_ctx* c, int ss, int sc, int ds, int dc, const uint64_t** tab) {
    std::lock_guard<std::mutex> lock(c->bconv_mu);
    for (const auto& e : c->bconv)
        if (e.src_start == ss && e.src_count == sc && e.dst_start == ds && e.dst_count == dc) {
            *tab = e.d_tab;
            return MFHE_OK;
        }
    hm::BconvTables t;
    if (!hm::bconv_tables(c->moduli.data() + ss, sc, c->moduli.data() + ds, dc, t))
        return set_error(MFHE_EINVAL, "basis conversion: bad limb ranges");
    std::vector<uint64_t> h((size_t)kBconvSrcWords * sc + (size_t)dc * (kBconvDstHead + sc), 0);
    for (int i = 0; i < sc; ++i) {
        uint64_t* s = h.data() + (size_t)kBconvSrcWords * i;
        s[0] = c->moduli[ss + i];
        s[1] = t.inv[i];
        s[2] = t.inv_shoup[i];
        std::memcpy(&s[3], &t.sinv[i], 8);
    }
    for (int j = 0; j < dc; ++j) {
        uint64_t* d = h.data() + (size_t)kBconvSrcWords * sc + (size_t)j * (kBconvDstHead + sc);
        const uint64_t q = c->moduli[ds + j];
        d[0] = t.smod[j] ? q - t.smod[j] : 0;
        d[1] = t.pinv[j];
        d[2] = t.pinv_shoup[j];
        for (int i = 0; i < sc; ++i) d[kBconvDstHead + i] = t.c[(size_t)j * sc + i];
    }
    void* d = nullptr;
    MFHE_HIP(hipMalloc(&d, h.size() * 8));
    hipError_t e = hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_error(e, "hipMemcpy (basis conversion table)");
    }
    c->allocs.push_back(d);
    c->bconv.push_back({ss, sc, ds, dc, (uint64_t*)d});
    *tab = (const uint64_t*)d;
    return MFHE_OK;
}

using BconvKernel = void (*)(BconvArgs, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*);

template <int V, int MODE>
static BconvKernel pick_ns(int ns) {
    switch (ns) {
        case 1: return bconv_kernel<1, V, MODE>;
        case 2: return bconv_kernel<2, V, MODE>;
        case 3: return bconv_kernel<3, V, MODE>;
        case 4: return bconv_kernel<4, V, MODE>;
        case 5: return bconv_kernel<5, V, MODE>;
        case 6: return bconv_kernel<6, V, MODE>;
        case 7: return bconv_kernel<7, V, MODE>;
        case 8: return bconv_kernel<8, V, MODE>;
        default: return bconv_kernel<0, V, MODE>;
    }
}
static_assert(kBconvUnroll == 8, "pick_ns lists the unrolled source counts");

template <int V>
static BconvKernel pick_mode(int ns, int mode) {
    if (mode == kBconvFast) return pick_ns<V, kBconvFast>(ns);
    if (mode == kBconvCentered) return pick_ns<V, kBconvCentered>(ns);
    return pick_ns<V, kBconvModDown>(ns);
}

int launch_bconv(BconvArgs a, size_t npoly, int kernel_mode, hipStream_t st) {
    const bool wide = ks_wide({&a.ncoeff, &a.in_stride, &a.out_stride}, {a.in, a.out});
    a.total = (uint64_t)npoly * a.ncoeff;
    a.lg = (a.ncoeff && !(a.ncoeff & (a.ncoeff - 1))) ? __builtin_ctzll(a.ncoeff) : -1;
    const uint64_t blocks = (a.total + 255) / 256;
    if (blocks == 0) return MFHE_OK;
    if (blocks > 0x7fffffffull) return set_error(MFHE_EINVAL, "basis conversion: too many coefficients for one launch");
    const BconvKernel k = wide ? pick_mode<2>(a.ns, kernel_mode) : pick_mode<1>(a.ns, kernel_mode);
    const uint64_t* t0 = a.r[0].tab;
    hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(256), 0, st, a, t0, a.nr > 1 ? a.r[1].tab : t0,
                       a.nr > 2 ? a.r[2].tab : t0, a.dmod);
    MFHE_CHECK_LAUNCH("bconv_kernel");
    return MFHE_OK;
}

int launch_copy_rows(const uint64_t* src, size_t src_stride, uint64_t* dst, size_t dst_stride, size_t npoly,
                     size_t words, hipStream_t st) {
    const uint64_t total = (uint64_t)npoly * words;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks == 0) return MFHE_OK;
    if (blocks > 0x7fffffffull) return set_error(MFHE_EINVAL, "basis conversion: too many coefficients for one launch");
    hipLaunchKernelGGL(bconv_copy_rows_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, src, (uint64_t)src_stride, dst,
                       (uint64_t)dst_stride, (uint64_t)words, total);
    MFHE_CHECK_LAUNCH("bconv_copy_rows_kernel");
    return MFHE_OK;
}

// ---- argument checks (nothing here touches the device) ----
static int check_range(const mfhe_ctx* c, int start, int count, const char* what) {
    if (start < 0 || count < 1 || start > c->L || count > c->L - start)
        return set_error(MFHE_EINVAL, std::string(what) + ": limb range outside the context");
    return MFHE_OK;
}
static bool overlap(int a, int na, int b, int nb) { return a < b + nb && b < a + na; }

static int check_buffers(const void* in, size_t in_stride, size_t in_rows, const void* out, size_t out_stride,
                         size_t out_rows, size_t ncoeff, const char* what) {
    if (!in || !out) return set_error(MFHE_EINVAL, std::string(what) + ": null pointer");
    if (ncoeff && (in_stride / ncoeff < in_rows || out_stride / ncoeff < out_rows))
        return set_error(MFHE_EINVAL, std::string(what) + ": poly stride smaller than rows * ncoeff");
    return MFHE_OK;
}

int check_modup(const mfhe_ctx* c, int level, int ds, int dc, int sp, int nsp, ModUpPlan& pl) {
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "modup: level outside the context");
    if (ds < 0 || dc < 1 || ds > level || dc > level - ds) return set_error(MFHE_EINVAL, "modup: digit outside [0, level)");
    if (nsp < 0 || sp < 0 || sp > c->L || nsp > c->L - sp) return set_error(MFHE_EINVAL, "modup: special limbs outside the context");
    if (nsp > 0 && sp < level) return set_error(MFHE_EINVAL, "modup: special limbs overlap [0, level)");
    auto add = [&](int limb, int row, int count) {
        if (count <= 0) return;
        pl.limb[pl.nr] = limb;
        pl.row[pl.nr] = row;
        pl.count[pl.nr] = count;
        ++pl.nr;
    };
    add(0, 0, ds);
    add(ds + dc, ds + dc, level - ds - dc);
    add(sp, level, nsp);
    return MFHE_OK;
}
static int check_moddown(const mfhe_ctx* c, int keep, int drop_start, int drop_count) {
    if (keep < 1 || keep > c->L) return set_error(MFHE_EINVAL, "moddown: keep_count outside the context");
    if (drop_start < keep) return set_error(MFHE_EINVAL, "moddown: drop_start < keep_count");
    return check_range(c, drop_start, drop_count, "moddown");
}

// ---- NTT-domain bodies with the scratch base as an argument (the public calls pass the context workspace; the key
// switch passes a part of its own block) ----
int ntt_modup_tables(mfhe_ctx* c, int digit_start, int digit_count, const ModUpPlan& pl, const uint64_t* tab[3]) {
    for (int k = 0; k < 3; ++k) tab[k] = nullptr;
    for (int k = 0; k < pl.nr; ++k) {
        int rc = bconv_table(c, digit_start, digit_count, pl.limb[k], pl.count[k], &tab[k]);
        if (rc) return rc;
    }
    return MFHE_OK;
}

// scratch: npoly * (level + nspecial) * N words
int ntt_modup_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                   size_t npoly, int digit_start, int digit_count, const ModUpPlan& pl, const uint64_t* const tab[3],
                   uint64_t* scratch, hipStream_t st) {
    const size_t N = c->N;
    mfhe_stream_t s = (mfhe_stream_t)st;
    int rc;
    // digit rows pass through
    if (d_in != d_out || in_stride != out_stride)
        if ((rc = launch_copy_rows(d_in + (size_t)digit_start * N, in_stride, d_out + (size_t)digit_start * N,
                                   out_stride, npoly, (size_t)digit_count * N, st)))
            return rc;
    if (pl.nr == 0) return MFHE_OK;
    uint64_t* dig = scratch;   // [npoly][digit_count][N]
    if ((rc = launch_copy_rows(d_in + (size_t)digit_start * N, in_stride, dig, (size_t)digit_count * N, npoly,
                               (size_t)digit_count * N, st)))
        return rc;
    if ((rc = mfhe_ntt_inv(c, dig, npoly, digit_start, digit_count, s))) return rc;
    uint64_t* blk = dig + npoly * (size_t)digit_count * N;
    for (int k = 0; k < pl.nr; ++k) {
        const size_t bw = (size_t)pl.count[k] * N;   // [npoly][count][N]
        BconvArgs a{};
        a.in = dig; a.out = blk; a.in_stride = (size_t)digit_count * N; a.out_stride = bw; a.ncoeff = N;
        a.ns = digit_count; a.src_row = 0; a.copy_row = -1; a.nr = 1;
        a.r[0].tab = tab[k]; a.r[0].limb = pl.limb[k]; a.r[0].row = 0; a.r[0].count = pl.count[k];
        a.dmod = c->d_dmod;
        if ((rc = launch_bconv(a, npoly, kBconvFast, st))) return rc;
        if ((rc = mfhe_ntt_fwd(c, blk, npoly, pl.limb[k], pl.count[k], s))) return rc;
        if ((rc = launch_copy_rows(blk, bw, d_out + (size_t)pl.row[k] * N, out_stride, npoly, bw, st))) return rc;
        blk += npoly * bw;
    }
    return MFHE_OK;
}

// The centred conversion of the dropped rows, forward-transformed: *cen = [npoly][keep_count][N] inside scratch
// (npoly * (keep_count + drop_count) * N words).
int ntt_moddown_center(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, size_t npoly, int keep_count,
                       int drop_start, int drop_count, const uint64_t* tab, uint64_t* scratch, const uint64_t** cen_out,
                       hipStream_t st) {
    const size_t N = c->N;
    mfhe_stream_t s = (mfhe_stream_t)st;
    int rc;
    uint64_t* drp = scratch;                                   // [npoly][drop_count][N]
    uint64_t* cen = drp + npoly * (size_t)drop_count * N;     // [npoly][keep_count][N]
    const size_t dw = (size_t)drop_count * N, kw = (size_t)keep_count * N;
    if ((rc = launch_copy_rows(d_in + kw, in_stride, drp, dw, npoly, dw, st))) return rc;
    if ((rc = mfhe_ntt_inv(c, drp, npoly, drop_start, drop_count, s))) return rc;
    BconvArgs a{};
    a.in = drp; a.out = cen; a.in_stride = dw; a.out_stride = kw; a.ncoeff = N;
    a.ns = drop_count; a.src_row = 0; a.copy_row = -1; a.nr = 1;
    a.r[0].tab = tab; a.r[0].limb = 0; a.r[0].row = 0; a.r[0].count = keep_count;
    a.dmod = c->d_dmod;
    if ((rc = launch_bconv(a, npoly, kBconvCentered, st))) return rc;
    if ((rc = mfhe_ntt_fwd(c, cen, npoly, 0, keep_count, s))) return rc;
    *cen_out = cen;
    return MFHE_OK;
}

int launch_sub_scale(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, const uint64_t* cen, size_t cen_stride,
                     uint64_t* d_out, size_t out_stride, const uint64_t* d_add, size_t npoly, int keep_count,
                     int drop_count, const uint64_t* tab, hipStream_t st) {
    const uint64_t total = (uint64_t)npoly * keep_count * c->N;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks == 0) return MFHE_OK;
    if (blocks > 0x7fffffffull) return set_error(MFHE_EINVAL, "ntt_moddown: too many coefficients for one launch");
    hipLaunchKernelGGL(bconv_sub_scale_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, d_in, (uint64_t)in_stride, cen,
                       (uint64_t)cen_stride, d_out, (uint64_t)out_stride, d_add, keep_count, c->logN, drop_count, tab,
                       (const uint64_t*)c->d_dmod, total);
    MFHE_CHECK_LAUNCH("bconv_sub_scale_kernel");
    return MFHE_OK;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_rns_bconv_reserve(mfhe_ctx* c, int src_start, int src_count, int dst_start, int dst_count) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    RC(check_range(c, src_start, src_count, "bconv source"));
    RC(check_range(c, dst_start, dst_count, "bconv destination"));
    if (overlap(src_start, src_count, dst_start, dst_count))
        return set_error(MFHE_EINVAL, "bconv: source and destination ranges overlap");
    const uint64_t* tab;
    return bconv_table(c, src_start, src_count, dst_start, dst_count, &tab);
}

extern "C" int mfhe_rns_bconv(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                              size_t npoly, size_t ncoeff, int src_start, int src_count, int dst_start, int dst_count,
                              int mode, mfhe_stream_t s) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (mode != MFHE_BCONV_FAST && mode != MFHE_BCONV_CENTERED) return set_error(MFHE_EINVAL, "bconv: unknown mode");
    RC(check_range(c, src_start, src_count, "bconv source"));
    RC(check_range(c, dst_start, dst_count, "bconv destination"));
    if (overlap(src_start, src_count, dst_start, dst_count))
        return set_error(MFHE_EINVAL, "bconv: source and destination ranges overlap");
    RC(check_buffers(d_in, in_stride, src_count, d_out, out_stride, dst_count, ncoeff, "bconv"));
    if (npoly == 0 || ncoeff == 0) return MFHE_OK;
    BconvArgs a{};
    RC(bconv_table(c, src_start, src_count, dst_start, dst_count, &a.r[0].tab));
    a.in = d_in; a.out = d_out; a.in_stride = in_stride; a.out_stride = out_stride; a.ncoeff = ncoeff;
    a.ns = src_count; a.src_row = 0; a.copy_row = -1; a.nr = 1;
    a.r[0].limb = dst_start; a.r[0].row = 0; a.r[0].count = dst_count;
    a.dmod = c->d_dmod;
    return launch_bconv(a, npoly, mode == MFHE_BCONV_FAST ? kBconvFast : kBconvCentered, (hipStream_t)s);
}

extern "C" int mfhe_rns_moddown(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out,
                                size_t out_stride, size_t npoly, size_t ncoeff, int keep_count, int drop_start,
                                int drop_count, mfhe_stream_t s) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    RC(check_moddown(c, keep_count, drop_start, drop_count));
    RC(check_buffers(d_in, in_stride, (size_t)keep_count + drop_count, d_out, out_stride, keep_count, ncoeff, "moddown"));
    if (d_in == d_out && in_stride != out_stride)
        return set_error(MFHE_EINVAL, "moddown: in place needs equal poly strides");
    if (npoly == 0 || ncoeff == 0) return MFHE_OK;
    BconvArgs a{};
    RC(bconv_table(c, drop_start, drop_count, 0, keep_count, &a.r[0].tab));
    a.in = d_in; a.out = d_out; a.in_stride = in_stride; a.out_stride = out_stride; a.ncoeff = ncoeff;
    a.ns = drop_count; a.src_row = keep_count; a.copy_row = -1; a.nr = 1;
    a.r[0].limb = 0; a.r[0].row = 0; a.r[0].count = keep_count;
    a.dmod = c->d_dmod;
    return launch_bconv(a, npoly, kBconvModDown, (hipStream_t)s);
}

extern "C" int mfhe_rns_modup(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                              size_t npoly, size_t ncoeff, int level, int digit_start, int digit_count,
                              int special_start, int nspecial, mfhe_stream_t s) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    ModUpPlan pl;
    RC(check_modup(c, level, digit_start, digit_count, special_start, nspecial, pl));
    RC(check_buffers(d_in, in_stride, level, d_out, out_stride, (size_t)level + nspecial, ncoeff, "modup"));
    if (npoly == 0 || ncoeff == 0) return MFHE_OK;
    if (pl.nr == 0)   // the digit is the whole basis: nothing to convert
        return launch_copy_rows(d_in, in_stride, d_out, out_stride, npoly, (size_t)level * ncoeff, (hipStream_t)s);
    BconvArgs a{};
    for (int k = 0; k < pl.nr; ++k) {
        RC(bconv_table(c, digit_start, digit_count, pl.limb[k], pl.count[k], &a.r[k].tab));
        a.r[k].limb = pl.limb[k]; a.r[k].row = pl.row[k]; a.r[k].count = pl.count[k];
    }
    a.in = d_in; a.out = d_out; a.in_stride = in_stride; a.out_stride = out_stride; a.ncoeff = ncoeff;
    a.ns = digit_count; a.src_row = digit_start; a.copy_row = digit_start; a.nr = pl.nr;
    a.dmod = c->d_dmod;
    return launch_bconv(a, npoly, kBconvFast, (hipStream_t)s);
}

// ---- NTT-domain forms: the source rows are staged into the context workspace, inverse-transformed there and
// converted into dense per-range blocks, which are forward-transformed and written to their rows (ntt.hip's launchers
// take dense [batch][nlimbs][N] blocks only) ----
static int check_ntt(const mfhe_ctx* c) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (!(c->conv & MFHE_CONV_PHANTOM)) return set_error(MFHE_ENOTREADY, "context was created without MFHE_CONV_PHANTOM");
    return MFHE_OK;
}

extern "C" int mfhe_ntt_bconv_reserve(mfhe_ctx* c, size_t npoly, int rows) {
    RC(check_ntt(c));
    if (rows < 0) return set_error(MFHE_EINVAL, "ntt_bconv_reserve: negative rows");
    return grow_ws(c, npoly * (size_t)rows * c->N * 8);
}

extern "C" int mfhe_ntt_modup(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride,
                              size_t npoly, int level, int digit_start, int digit_count, int special_start,
                              int nspecial, mfhe_stream_t s) {
    RC(check_ntt(c));
    ModUpPlan pl;
    RC(check_modup(c, level, digit_start, digit_count, special_start, nspecial, pl));
    const size_t N = c->N;
    RC(check_buffers(d_in, in_stride, level, d_out, out_stride, (size_t)level + nspecial, N, "ntt_modup"));
    if (npoly == 0) return MFHE_OK;
    const uint64_t* tab[3];
    RC(ntt_modup_tables(c, digit_start, digit_count, pl, tab));
    RC(grow_ws(c, npoly * ((size_t)level + nspecial) * N * 8));
    return ntt_modup_body(c, d_in, in_stride, d_out, out_stride, npoly, digit_start, digit_count, pl, tab,
                          (uint64_t*)c->ws, (hipStream_t)s);
}

extern "C" int mfhe_ntt_moddown(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* d_out,
                                size_t out_stride, size_t npoly, int keep_count, int drop_start, int drop_count,
                                mfhe_stream_t s) {
    RC(check_ntt(c));
    RC(check_moddown(c, keep_count, drop_start, drop_count));
    const size_t N = c->N;
    RC(check_buffers(d_in, in_stride, (size_t)keep_count + drop_count, d_out, out_stride, keep_count, N, "ntt_moddown"));
    if (d_in == d_out && in_stride != out_stride)
        return set_error(MFHE_EINVAL, "ntt_moddown: in place needs equal poly strides");
    if (npoly == 0) return MFHE_OK;
    hipStream_t st = (hipStream_t)s;
    const uint64_t* tab = nullptr;
    RC(bconv_table(c, drop_start, drop_count, 0, keep_count, &tab));
    RC(grow_ws(c, npoly * ((size_t)keep_count + drop_count) * N * 8));
    const uint64_t* cen = nullptr;
    RC(ntt_moddown_center(c, d_in, in_stride, npoly, keep_count, drop_start, drop_count, tab, (uint64_t*)c->ws, &cen, st));
    return launch_sub_scale(c, d_in, in_stride, cen, (size_t)keep_count * N, d_out, out_stride, nullptr, npoly,
                            keep_count, drop_count, tab, st);
}

// slot.hip -- CKKS slot encoding and decoding on the key switch's layout (include/mfhe.h mfhe_slot_*; slot.hpp).
//
// One kernel template runs every launch: a workgroup fills a 2^12-point double2 tile in LDS (`2^lc` transforms of
// `2^lm` points, element idx of transform c at idx 2^lc + c), runs the transforms in place as Stockham passes of radix
// 8 (then 4 or 2) with the butterflies in registers, and writes the tile out.  STAGE 0 is a whole transform per
// polynomial (n <= 2^12: the columns are polynomials); above that n = n1 n2 and STAGE 1 transforms n2 points of stride
// n1 for 2^lc neighbouring k1, multiplies by w^(k1 t2) and writes [t2][k1] to the workspace, STAGE 2 transforms the n1
// contiguous points of 2^lc neighbouring t2 and produces output n2 t1 + t2.  The two ends are fused: decode's first
// stage composes the residues of limbs [0, d) (Garner, centred, to f64) and twists by zeta^k while loading; encode's
// last stage multiplies by zeta^-k scale / n, rounds and writes the residues of every row (two coefficients per lane in
// 16-byte stores where the strides are even and the rows 16-byte aligned).  Every twiddle and twist is
// sincospi of an argument reduced in integers; there is no recurrence anywhere.
#include "slot.hpp"

#include <cmath>
#include <mutex>
#include <vector>

#include "bconv.hpp"
#include "keyswitch.hpp"
#include "mfhe_ctx.hpp"
#include "mod128.hpp"

namespace mfhe {
namespace slot {

__device__ __forceinline__ double2 cmul(double2 x, double2 y) {
    return make_double2(__fma_rn(x.x, y.x, -x.y * y.y), __fma_rn(x.x, y.y, x.y * y.x));
}
// e^(i pi x)
__device__ __forceinline__ double2 expipi(double x) {
    double sn, cs;
    sincospi(x, &sn, &cs);
    return make_double2(cs, sn);
}
// v e^(SG 2 pi i k / 8), k = 0..3
template <int SG>
__device__ __forceinline__ double2 mul_w8(double2 v, int k) {
    constexpr double h = 0.70710678118654752440;
    if (k == 0) return v;
    if (k == 2) return make_double2(-SG * v.y, SG * v.x);
    if (k == 1) return make_double2(h * (v.x - SG * v.y), h * (SG * v.x + v.y));
    return make_double2(-h * (v.x + SG * v.y), h * (SG * v.x - v.y));
}
// in-register R-point DFT (R = 2, 4, 8), natural order in and out: X[k] = sum_s x[s] e^(SG 2 pi i s k / R)
template <int R, int SG>
__device__ __forceinline__ void fft_reg(double2 (&x)[R]) {
    auto sw = [&](int i, int j) {
        const double2 t = x[i];
        x[i] = x[j];
        x[j] = t;
    };
    if constexpr (R == 8) {
        sw(1, 4);
        sw(3, 6);
    }
    if constexpr (R == 4) sw(1, 2);
#pragma unroll
    for (int len = 2; len <= R; len <<= 1)
#pragma unroll
        for (int i = 0; i < R; i += len)
#pragma unroll
            for (int j = 0; j < len / 2; ++j) {
                const double2 u = x[i + j], v = mul_w8<SG>(x[i + j + len / 2], j * (8 / len));
                x[i + j] = make_double2(u.x + v.x, u.y + v.y);
                x[i + j + len / 2] = make_double2(u.x - v.x, u.y - v.y);
            }
}

// One Stockham pass of radix R = 2^RL over the tile, in place: the sub-transforms so far have 2^lns points.  Work item
// (j, c), j < m / R: inputs j + r m / R, twiddle e^(SG 2 pi i r k / (Ns R)) with k = j mod Ns, outputs
// (j / Ns) Ns R + k + r Ns.  A thread holds all its inputs (8 points) across the barrier.
template <int RL, int SG>
__device__ __forceinline__ void lds_pass(double2* S, int lm, int lc, int lns, int t) {
    constexpr int R = 1 << RL, I = 8 >> RL;
    const int items = 1 << (lm + lc - RL), mr = 1 << (lm - RL);
    double2 v[I][R];
#pragma unroll
    for (int i = 0; i < I; ++i) {
        const int w = t + kSlotThreads * i;
        if (w < items) {
            const int c = w & ((1 << lc) - 1), j = w >> lc, k = j & ((1 << lns) - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) v[i][r] = S[((j + r * mr) << lc) + c];
            if (lns > 0) {
                const double inv = 1.0 / (double)(1 << (lns + RL - 1));   // a power of two: r k inv is exact
#pragma unroll
                for (int r = 1; r < R; ++r) v[i][r] = cmul(v[i][r], expipi(SG * (double)(r * k) * inv));
            }
            fft_reg<R, SG>(v[i]);
        }
    }
    __syncthreads();   // every thread has read its inputs
#pragma unroll
    for (int i = 0; i < I; ++i) {
        const int w = t + kSlotThreads * i;
        if (w < items) {
            const int c = w & ((1 << lc) - 1), j = w >> lc, k = j & ((1 << lns) - 1);
            const int j0 = ((j >> lns) << (lns + RL)) + k;
#pragma unroll
            for (int r = 0; r < R; ++r) S[((j0 + (r << lns)) << lc) + c] = v[i][r];
        }
    }
    __syncthreads();
}

template <int SG>
__device__ __forceinline__ void lds_fft(double2* S, int lm, int lc, int t) {
    int lns = 0;
#pragma unroll 1
    while (lns < lm) {
        const int rem = lm - lns;
        if (rem >= 3) {
            lds_pass<3, SG>(S, lm, lc, lns, t);
            lns += 3;
        } else if (rem == 2) {
            lds_pass<2, SG>(S, lm, lc, lns, t);
            lns += 2;
        } else {
            lds_pass<1, SG>(S, lm, lc, lns, t);
            lns += 1;
        }
    }
}

// |x| < 2^128 to the nearest double: the leading 64 bits with the rest as a sticky bit, scaled back
__device__ __forceinline__ double u128_to_f64(u128 x) {
    const uint64_t hi = (uint64_t)(x >> 64), lo = (uint64_t)x;
    if (hi == 0) return (double)lo;
    const int lz = __clzll((long long)hi);
    const u128 y = x << lz;
    const uint64_t top = (uint64_t)(y >> 64) | ((uint64_t)y != 0 ? 1ull : 0ull);
    return ldexp((double)top, 64 - lz);
}

// the centred value of coefficient `coef` of polynomial p on limbs [0, d), as a double
__device__ __forceinline__ double load_lift(const SlotArgs& a, uint64_t p, uint32_t coef) {
    const uint64_t* src = a.res_in + p * a.stride0;
    const uint64_t r0 = src[coef];
    if (a.d == 1) {
        const bool neg = r0 > (a.q0 - 1) / 2;
        const double m = (double)(neg ? a.q0 - r0 : r0);
        return neg ? -m : m;
    }
    const uint64_t r1 = src[((uint64_t)1 << a.logN) + coef];
    const uint64_t b0 = a.dmod[4], b1 = a.dmod[5];   // floor(2^128 / q_1)
    const uint64_t r0m = barrett128((u128)r0, a.q1, b0, b1);
    const uint64_t dl = r1 >= r0m ? r1 - r0m : r1 + a.q1 - r0m;
    const uint64_t h = barrett128((u128)dl * a.q0inv1, a.q1, b0, b1);
    const u128 Q = (u128)a.q0 * a.q1, x = (u128)a.q0 * h + r0;
    const bool neg = x > (Q - 1) / 2;
    const double m = u128_to_f64(neg ? Q - x : x);
    return neg ? -m : m;
}

// the integer x (an integral double, |x| < 2^63) mod q, canonical
__device__ __forceinline__ uint64_t reduce_rounded(double x, uint64_t q, uint64_t b0, uint64_t b1) {
    const long long v = (long long)x;
    const bool neg = v < 0;
    const uint64_t mag = neg ? 0ull - (uint64_t)v : (uint64_t)v;
    const uint64_t r = barrett128((u128)mag, q, b0, b1);
    return neg && r ? q - r : r;
}

// the rounded coefficients k and k + n of output point g: v zeta^-k scale / n
__device__ __forceinline__ void encode_point(const SlotArgs& a, double2 v, uint32_t g, uint32_t N, double& xr, double& xi) {
    const double2 u = cmul(v, expipi(-(double)g / (double)N));
    xr = rint(u.x * a.mul);
    xi = rint(u.y * a.mul);
}

// V: coefficients per residue store of encode's last stage (2: the 16-byte form; every other access is 8 bytes)
template <bool ENC, int STAGE, int V>
__global__ __launch_bounds__(kSlotThreads) void slot_kernel(SlotArgs a) {
    __shared__ double2 S[1 << kSlotTileLog];
    constexpr int SG = ENC ? -1 : 1;
    const int t = threadIdx.x;
    const int lm = a.lm, lc = a.lc, E = 1 << (lm + lc);
    const uint32_t N = 1u << a.logN, n = N >> 1;
    const int l2 = a.logN - 1 - a.l1;
    uint64_t p0;
    uint32_t base = 0;
    if constexpr (STAGE == 0) {
        p0 = (uint64_t)blockIdx.x << lc;
    } else {
        const int lt = (STAGE == 1 ? a.l1 : l2) - lc;   // log2 of the tiles of a polynomial
        p0 = blockIdx.x >> lt;
        base = (blockIdx.x & ((1u << lt) - 1)) << lc;
    }
    // ---- fill the tile ----
    for (int e = t; e < E; e += kSlotThreads) {
        int idx, c;
        if constexpr (STAGE == 1) {
            c = e & ((1 << lc) - 1);
            idx = e >> lc;
        } else {
            idx = e & ((1 << lm) - 1);
            c = e >> lm;
        }
        const uint64_t p = STAGE == 0 ? p0 + c : p0;
        double2 val = make_double2(0.0, 0.0);
        if (p < a.npoly) {
            if constexpr (STAGE == 2) {
                val = a.ws[p * n + ((uint64_t)(base + c) << a.l1) + idx];
            } else {
                const uint32_t g = STAGE == 0 ? (uint32_t)idx : base + c + ((uint32_t)idx << a.l1);
                if constexpr (ENC) {
                    const uint32_t j = a.jinv[g];
                    const double* z = a.slots_in + p * a.slot_stride;
                    val = a.real ? make_double2(z[j], 0.0) : make_double2(z[2ull * j], z[2ull * j + 1]);
                } else {
                    const double2 u = make_double2(load_lift(a, p, g), load_lift(a, p, g + n));
                    val = cmul(u, expipi((double)g / (double)N));   // zeta^k
                }
            }
        }
        S[(idx << lc) + c] = val;
    }
    __syncthreads();
    lds_fft<SG>(S, lm, lc, t);
    // ---- write the tile ----
    if constexpr (ENC && STAGE != 1 && V == 2) {
        // two neighbouring coefficients per lane: points (idx, idx + 1) of a column in the whole form, columns
        // (c, c + 1) in pass B; g is even, so with even strides and 16-byte-aligned rows every store is aligned
        for (int e = t; e < E / 2; e += kSlotThreads) {
            int idx, c, step;
            if constexpr (STAGE == 0) {
                idx = (e & ((1 << (lm - 1)) - 1)) << 1;
                c = e >> (lm - 1);
                step = 1 << lc;
            } else {
                c = (e & ((1 << (lc - 1)) - 1)) << 1;
                idx = e >> (lc - 1);
                step = 1;
            }
            const uint64_t p = STAGE == 0 ? p0 + c : p0;
            if (p >= a.npoly) continue;
            const uint32_t g = STAGE == 0 ? (uint32_t)idx : ((uint32_t)idx << l2) + base + c;
            double xr[2], xi[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) encode_point(a, S[(idx << lc) + c + h * step], g + h, N, xr[h], xi[h]);
            const int rows = a.level + a.nspecial;
            for (int r = 0; r < rows; ++r) {
                const int limb = r < a.level ? r : a.special_start + r - a.level;
                const uint64_t q = a.dmod[3 * limb], b0 = a.dmod[3 * limb + 1], b1 = a.dmod[3 * limb + 2];
                uint64_t* dst = r < a.level ? a.res0 + p * a.stride0 + (uint64_t)r * N
                                            : a.res1 + p * a.stride1 + (uint64_t)(r - a.level) * N;
                *(ulonglong2*)(dst + g) = make_ulonglong2(reduce_rounded(xr[0], q, b0, b1), reduce_rounded(xr[1], q, b0, b1));
                *(ulonglong2*)(dst + g + n) =
                    make_ulonglong2(reduce_rounded(xi[0], q, b0, b1), reduce_rounded(xi[1], q, b0, b1));
            }
        }
        return;
    }
    for (int e = t; e < E; e += kSlotThreads) {
        int idx, c;
        if constexpr (STAGE == 0) {
            idx = e & ((1 << lm) - 1);
            c = e >> lm;
        } else {
            c = e & ((1 << lc) - 1);
            idx = e >> lc;
        }
        const uint64_t p = STAGE == 0 ? p0 + c : p0;
        if (p >= a.npoly) continue;
        const double2 v = S[(idx << lc) + c];
        if constexpr (STAGE == 1) {
            const uint32_t k1 = base + c, t2 = (uint32_t)idx;   // k1 t2 < n
            const double2 w = expipi(SG * (double)(k1 * t2) / (double)(n >> 1));
            a.ws[p * n + ((uint64_t)t2 << a.l1) + k1] = cmul(v, w);
        } else {
            const uint32_t g = STAGE == 0 ? (uint32_t)idx : ((uint32_t)idx << l2) + base + c;
            if constexpr (ENC) {
                double xr, xi;
                encode_point(a, v, g, N, xr, xi);
                const int rows = a.level + a.nspecial;
                for (int r = 0; r < rows; ++r) {
                    const int limb = r < a.level ? r : a.special_start + r - a.level;
                    const uint64_t q = a.dmod[3 * limb], b0 = a.dmod[3 * limb + 1], b1 = a.dmod[3 * limb + 2];
                    uint64_t* dst = r < a.level ? a.res0 + p * a.stride0 + (uint64_t)r * N
                                                : a.res1 + p * a.stride1 + (uint64_t)(r - a.level) * N;
                    dst[g] = reduce_rounded(xr, q, b0, b1);
                    dst[g + n] = reduce_rounded(xi, q, b0, b1);
                }
            } else {
                const uint32_t j = a.jinv[g];
                double* z = a.slots_out + p * a.slot_stride;
                if (a.real) {
                    z[j] = v.x * a.mul;
                } else {
                    z[2ull * j] = v.x * a.mul;
                    z[2ull * j + 1] = v.y * a.mul;
                }
            }
        }
    }
}

template <bool ENC, int STAGE>
static int launch_stage(SlotArgs a, uint64_t blocks, hipStream_t st) {
    if (blocks > 0x7fffffffull) return set_error(MFHE_EINVAL, "slot: too many polynomials for one launch");
    if constexpr (ENC && STAGE != 1) {
        // the 16-byte form, chosen as the RNS kernels choose theirs: even strides and 16-byte-aligned rows (N is even)
        if (!((a.stride0 | a.stride1) & 1) && !(((uintptr_t)a.res0 | (uintptr_t)a.res1) & 15)) {
            hipLaunchKernelGGL((slot_kernel<ENC, STAGE, 2>), dim3((uint32_t)blocks), dim3(kSlotThreads), 0, st, a);
            MFHE_CHECK_LAUNCH("slot_kernel");
            return MFHE_OK;
        }
    }
    hipLaunchKernelGGL((slot_kernel<ENC, STAGE, 1>), dim3((uint32_t)blocks), dim3(kSlotThreads), 0, st, a);
    MFHE_CHECK_LAUNCH("slot_kernel");
    return MFHE_OK;
}

// the one or two launches of the transforms of `a` (everything but lm, lc, l1 filled in)
template <bool ENC>
static int launch_transform(SlotArgs a, const SlotGeom& g, hipStream_t st) {
    if (g.whole) {
        a.lm = g.ln;
        a.lc = g.lcW;
        a.l1 = 0;
        return launch_stage<ENC, 0>(a, (a.npoly + ((uint64_t)1 << g.lcW) - 1) >> g.lcW, st);
    }
    a.l1 = g.l1;
    a.lm = g.l2;
    a.lc = g.lcA;
    int rc = launch_stage<ENC, 1>(a, a.npoly << (g.l1 - g.lcA), st);
    if (rc) return rc;
    a.lm = g.l1;
    a.lc = g.lcB;
    return launch_stage<ENC, 2>(a, a.npoly << (g.l2 - g.lcB), st);
}

// the cached table jinv[t] of the context's ring degree; built and uploaded on first use
static int jinv_table(mfhe_ctx* c, const uint32_t** tab) {
    std::lock_guard<std::mutex> lk(c->bconv_mu);
    if (!c->d_slot_jinv) {
        std::vector<uint32_t> h(c->N / 2);
        slot_jinv_table(c->logN, h.data());
        uint32_t* d = nullptr;
        MFHE_HIP(hipMalloc(&d, h.size() * sizeof(uint32_t)));
        hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return hip_error(e, "slot: table upload");
        }
        c->allocs.push_back(d);
        c->d_slot_jinv = d;
    }
    *tab = c->d_slot_jinv;
    return MFHE_OK;
}

static int check_ctx(const mfhe_ctx* c) {
    int rc = ks_check_ctx(c);
    if (rc) return rc;
    if (c->logN < 2) return set_error(MFHE_EUNSUPPORTED, "slot: log_n must be >= 2");
    return MFHE_OK;
}

static int check_rows(const mfhe_ctx* c, int level, int special_start, int nspecial, const char* what) {
    const std::string w(what);
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, w + ": level outside the context");
    if (nspecial < 0) return set_error(MFHE_EINVAL, w + ": nspecial < 0");
    if (nspecial == 0) return MFHE_OK;
    return ks_check_geom(c, KsGeom{level, level, special_start, nspecial}, what);
}

static uint64_t mulmod(uint64_t x, uint64_t y, uint64_t q) { return (uint64_t)((unsigned __int128)x * y % q); }
// x^-1 mod the prime q
static uint64_t invmod(uint64_t x, uint64_t q) {
    uint64_t r = 1, b = x % q, e = q - 2;
    for (; e; e >>= 1, b = mulmod(b, b, q))
        if (e & 1) r = mulmod(r, b, q);
    return r;
}

}  // namespace slot
}  // namespace mfhe

using namespace mfhe;
using namespace mfhe::slot;

extern "C" int mfhe_slot_reserve(mfhe_ctx* c, size_t npoly, int level, int special_start, int nspecial) {
    RC(check_ctx(c));
    RC(check_rows(c, level, special_start, nspecial, "slot_reserve"));
    const uint32_t* tab;
    RC(jinv_table(c, &tab));
    const size_t rows = (size_t)level + nspecial;
    return grow_ws(c, slot_ws_words(c->logN, npoly, rows > 2 ? rows : 2) * 8);
}

extern "C" int mfhe_slot_encode(mfhe_ctx* c, const double* d_slots, size_t slot_stride, double scale, uint64_t* d_out,
                                size_t out_poly_stride, size_t npoly, int level, int special_start, int nspecial,
                                int flags, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!d_slots || !d_out) return set_error(MFHE_EINVAL, "slot_encode: null pointer");
    if (flags & ~(MFHE_SLOT_REAL | MFHE_SLOT_COEFF)) return set_error(MFHE_EINVAL, "slot_encode: unknown flag");
    if (!(scale > 0.0) || !std::isfinite(scale)) return set_error(MFHE_EINVAL, "slot_encode: scale is not finite and positive");
    RC(check_rows(c, level, special_start, nspecial, "slot_encode"));
    const size_t N = c->N, rows = (size_t)level + nspecial;
    const bool real = flags & MFHE_SLOT_REAL, coeff = flags & MFHE_SLOT_COEFF;
    const size_t sw = real ? N / 2 : N;
    if (slot_stride < sw) return set_error(MFHE_EINVAL, "slot_encode: slot stride smaller than a polynomial's slots");
    if (out_poly_stride < rows * N) return set_error(MFHE_EINVAL, "slot_encode: poly stride smaller than rows * N");
    if (ks_ranges_overlap((const uint64_t*)d_slots, ks_span(npoly, slot_stride, sw), d_out,
                          ks_span(npoly, out_poly_stride, rows * N)))
        return set_error(MFHE_EINVAL, "slot_encode: the slots overlap the output");
    if (npoly == 0) return MFHE_OK;
    hipStream_t st = (hipStream_t)s;
    const SlotGeom g = slot_geom(c->logN, npoly);
    const bool direct = coeff || (nspecial == 0 && out_poly_stride == rows * N);   // the kernel writes d_out itself
    const uint32_t* tab;
    RC(jinv_table(c, &tab));
    RC(grow_ws(c, slot_ws_words(c->logN, npoly, direct ? 0 : rows) * 8));
    uint64_t* ws = (uint64_t*)c->ws;
    uint64_t* dense = ws + (g.whole ? 0 : npoly * N);
    SlotArgs a{};
    a.slots_in = d_slots; a.slot_stride = slot_stride; a.ws = (double2*)ws; a.jinv = tab; a.dmod = c->d_dmod;
    a.mul = scale / (double)(N / 2); a.npoly = npoly; a.logN = c->logN;
    a.level = level; a.special_start = special_start; a.nspecial = nspecial; a.real = real;
    uint64_t* blkS = dense + npoly * (size_t)level * N;
    if (direct) {
        a.res0 = d_out; a.stride0 = out_poly_stride;
        a.res1 = d_out + (size_t)level * N; a.stride1 = out_poly_stride;
    } else {
        a.res0 = dense; a.stride0 = (size_t)level * N;
        a.res1 = blkS; a.stride1 = (size_t)nspecial * N;
    }
    RC(launch_transform<true>(a, g, st));
    if (coeff) return MFHE_OK;
    if (direct) return mfhe_ntt_fwd(c, d_out, npoly, 0, level, s);
    RC(mfhe_ntt_fwd(c, dense, npoly, 0, level, s));
    RC(launch_copy_rows(dense, (size_t)level * N, d_out, out_poly_stride, npoly, (size_t)level * N, st));
    if (nspecial > 0) {
        RC(mfhe_ntt_fwd(c, blkS, npoly, special_start, nspecial, s));
        RC(launch_copy_rows(blkS, (size_t)nspecial * N, d_out + (size_t)level * N, out_poly_stride, npoly,
                       (size_t)nspecial * N, st));
    }
    return MFHE_OK;
}

extern "C" int mfhe_slot_decode(mfhe_ctx* c, const uint64_t* d_in, size_t in_poly_stride, double scale, double* d_slots,
                                size_t slot_stride, size_t npoly, int level, int flags, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!d_in || !d_slots) return set_error(MFHE_EINVAL, "slot_decode: null pointer");
    if (flags & ~(MFHE_SLOT_REAL | MFHE_SLOT_COEFF)) return set_error(MFHE_EINVAL, "slot_decode: unknown flag");
    if (!(scale > 0.0) || !std::isfinite(scale)) return set_error(MFHE_EINVAL, "slot_decode: scale is not finite and positive");
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "slot_decode: level outside the context");
    const size_t N = c->N;
    const int d = level < 2 ? level : 2;
    const bool real = flags & MFHE_SLOT_REAL, coeff = flags & MFHE_SLOT_COEFF;
    const size_t sw = real ? N / 2 : N;
    if (slot_stride < sw) return set_error(MFHE_EINVAL, "slot_decode: slot stride smaller than a polynomial's slots");
    if (in_poly_stride < (size_t)d * N) return set_error(MFHE_EINVAL, "slot_decode: poly stride smaller than the rows read");
    if (ks_ranges_overlap(d_in, ks_span(npoly, in_poly_stride, (size_t)d * N), (const uint64_t*)d_slots,
                          ks_span(npoly, slot_stride, sw)))
        return set_error(MFHE_EINVAL, "slot_decode: the residues overlap the slots");
    if (npoly == 0) return MFHE_OK;
    hipStream_t st = (hipStream_t)s;
    const SlotGeom g = slot_geom(c->logN, npoly);
    const uint32_t* tab;
    RC(jinv_table(c, &tab));
    RC(grow_ws(c, slot_ws_words(c->logN, npoly, coeff ? 0 : d) * 8));
    uint64_t* ws = (uint64_t*)c->ws;
    uint64_t* dense = ws + (g.whole ? 0 : npoly * N);
    SlotArgs a{};
    a.slots_out = d_slots; a.slot_stride = slot_stride; a.ws = (double2*)ws; a.jinv = tab; a.dmod = c->d_dmod;
    a.mul = 1.0 / scale; a.npoly = npoly; a.logN = c->logN; a.d = d; a.real = real;
    a.q0 = c->moduli[0];
    if (d == 2) {
        a.q1 = c->moduli[1];
        a.q0inv1 = invmod(a.q0, a.q1);
    }
    if (coeff) {
        a.res_in = d_in; a.stride0 = in_poly_stride;
    } else {
        RC(launch_copy_rows(d_in, in_poly_stride, dense, (size_t)d * N, npoly, (size_t)d * N, st));
        RC(mfhe_ntt_inv(c, dense, npoly, 0, d, s));
        a.res_in = dense; a.stride0 = (size_t)d * N;
    }
    return launch_transform<false>(a, g, st);
}

// rlwe.hip -- the RLWE client side on the key switch's layout (include/mfhe.h mfhe_rlwe_*; rlwe.hpp): seeded
// samplers, secret / public / switching / relinearisation / Galois keys, symmetric and public-key encryption,
// decryption.  Everything is in the evaluation domain (phantom NTT) and canonical; row r < level is limb r, otherwise
// limb special_start + r - level.  The draws are rlwe_draw.hpp's, the one definition for host and device.
//
//   rlwe_small_kernel : a thread expands one ChaCha block into eight small integers (or reads eight int32) of one
//                       polynomial and stores their residues on every row; the rows then go through mfhe_ntt_fwd in
//                       dense blocks of the workspace (Q rows, then special rows), as mfhe_slot_encode's do
//   rlwe_mask_kernel  : a thread expands one ChaCha block into four neighbouring mask residues a of one row (128 bits
//                       each, barrett128) and walks a run of polynomials: out1 = a, out0 = e + x - a s with NTT(e) from
//                       the dense blocks and x = 0, m or F s_from.  a never comes from memory.  The row is the grid's y
//                       index, so the modulus, its Barrett constants, the seed and the nonce are scalar.
//   rlwe_pk_kernel    : c0 = pk0 u + e0 + m, c1 = pk1 u + e1 from the three dense blocks
//   rlwe_dec_kernel   : out = c0 + c1 s
// Every store is a vector store from plain C++; no value read from memory or drawn selects a branch or an address,
// except the Galois gather's index, which depends on the public element alone.
#include "rlwe.hpp"

#include <string>

#include "bconv.hpp"
#include "galois.hpp"
#include "keyswitch.hpp"
#include "mfhe_ctx.hpp"
#include "mod128.hpp"
#include "rlwe_draw.hpp"

namespace mfhe {
namespace rlwe {

// shortest run of polynomials one thread walks with its slice of s (the whole batch when it is smaller)
constexpr uint64_t kRlweMinRun = 4;

template <bool LIFT, bool WIDE>
__global__ __launch_bounds__(256) void rlwe_small_kernel(RlweSmallArgs a) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;   // the block of eight coefficients
    const uint32_t N = 1u << a.logN;
    if (b >= (N >> 3)) return;
    const uint64_t pp = blockIdx.y + (uint64_t)blockIdx.z * gridDim.y;
    if (pp >= a.npoly * (uint64_t)a.nsets) return;
    const uint64_t set = pp / a.npoly, p = pp - set * a.npoly;
    int v[8];
    if constexpr (LIFT) {
        const int32_t* src = a.coeffs + p * a.coeff_stride + 8ull * b;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[k];
    } else {
        const int stream = set == 0 ? a.stream0 : set == 1 ? a.stream1 : a.stream2;
        uint32_t nonce[3], out[16];
        rlwe_nonce(stream, 0, a.first_id + p, nonce);
        chacha20_block(a.seed.w, b, nonce, out);
        const bool ternary = rlwe_stream_is_ternary(stream);   // uniform over the launch's set
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint64_t w = rlwe_small_word(out, k);
            v[k] = ternary ? rlwe_ternary(w) : rlwe_noise(w);
        }
    }
    const int rows = a.level + a.nspecial;
    for (int r = 0; r < rows; ++r) {
        const int limb = r < a.level ? r : a.special_start + r - a.level;
        const uint64_t q = a.dmod[3 * limb];
        uint64_t* dst = (r < a.level ? a.res0 + pp * a.stride0 + (uint64_t)r * N
                                     : a.res1 + pp * a.stride1 + (uint64_t)(r - a.level) * N) + 8ull * b;
        uint64_t x[8];
        if constexpr (LIFT) {
            // any int32: |v| mod q with the sign put back by a select
            const uint64_t r0 = a.dmod[3 * limb + 1], r1 = a.dmod[3 * limb + 2];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t s = v[k];
                const uint64_t mag = (uint64_t)((s ^ (s >> 63)) - (s >> 63));
                const uint64_t m = barrett128((u128)mag, q, r0, r1);
                const uint64_t n = m ? q - m : 0;
                x[k] = s < 0 ? n : m;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = rlwe_small_residue(v[k], q);
        }
        if constexpr (WIDE) {
#pragma unroll
            for (int k = 0; k < 8; k += 2) *(ulonglong2*)(dst + k) = make_ulonglong2(x[k], x[k + 1]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[k] = x[k];
        }
    }
}

template <bool WIDE>
static __device__ __forceinline__ void load4(const uint64_t* p, uint64_t (&x)[4]) {
    if constexpr (WIDE) {
        const ulonglong2 lo = *(const ulonglong2*)p, hi = *(const ulonglong2*)(p + 2);
        x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = p[k];
    }
}
template <bool WIDE>
static __device__ __forceinline__ void store4(uint64_t* p, const uint64_t (&x)[4]) {
    if constexpr (WIDE) {
        *(ulonglong2*)p = make_ulonglong2(x[0], x[1]);
        *(ulonglong2*)(p + 2) = make_ulonglong2(x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = x[k];
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void rlwe_mask_kernel(RlweMaskArgs a) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;   // the ChaCha block: coefficients 4 b .. 4 b + 3
    const uint32_t N = 1u << a.logN;
    if (b >= (N >> 2)) return;
    const int r = blockIdx.y;
    const int limb = r < a.level ? r : a.special_start + r - a.level;
    const uint64_t q = a.dmod[3 * limb], r0 = a.dmod[3 * limb + 1], r1 = a.dmod[3 * limb + 2];
    const uint64_t off = (uint64_t)r * N + 4ull * b;
    const int kind = a.kind;
    uint64_t sv[4] = {0, 0, 0, 0}, xs[4] = {0, 0, 0, 0};
    if (kind != kRlweMaskOnly) load4<WIDE>(a.s + off, sv);
    if (kind == kRlweKeySwitch) load4<WIDE>(a.add + off, xs);
    if (kind == kRlweKeyRelin) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = barrett128((u128)sv[k] * sv[k], q, r0, r1);
    }
    if (kind == kRlweKeyGalois) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = a.s[(uint64_t)r * N + galois_perm_index(4u * b + k, a.galois_elt, a.logN)];
    }
    const uint64_t* ebase = r < a.level ? a.e0 + (uint64_t)r * N : a.e1 + (uint64_t)(r - a.level) * N;
    const uint64_t estride = r < a.level ? a.e_stride0 : a.e_stride1;
    const uint64_t p0 = blockIdx.z * a.prun;
    const uint64_t p1 = p0 + a.prun < a.npoly ? p0 + a.prun : a.npoly;
    for (uint64_t p = p0; p < p1; ++p) {
        uint32_t nonce[3], out[16];
        rlwe_nonce(kRlweMask, limb, a.first_id + p, nonce);
        chacha20_block(a.seed.w, b, nonce, out);
        uint64_t av[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint64_t lo, hi;
            rlwe_mask_word(out, k, lo, hi);
            av[k] = barrett128(((u128)hi << 64) | lo, q, r0, r1);
        }
        store4<WIDE>(a.out1 + p * a.out_stride + off, av);
        if (kind == kRlweMaskOnly) continue;
        uint64_t ev[4], o[4];
        load4<WIDE>(ebase + p * estride + 4ull * b, ev);
        uint64_t F = 0;
        if (kind == kRlweEncMsg) {
            F = 1;
            load4<WIDE>(a.add + p * a.add_stride + off, xs);
        } else if (kind >= kRlweKeySwitch) {
            F = (r < a.level && (uint64_t)(r / a.alpha) == p) ? a.pmod[r] : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t as = barrett128((u128)av[k] * sv[k], q, r0, r1);
            o[k] = barrett128((u128)F * xs[k] + ev[k] + (q - as), q, r0, r1);
        }
        store4<WIDE>(a.out0 + p * a.out_stride + off, o);
    }
}

template <int V>
__global__ __launch_bounds__(256) void rlwe_pk_kernel(RlwePkArgs a) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t q = a.dmod[3 * r], r0 = a.dmod[3 * r + 1], r1 = a.dmod[3 * r + 2];
    const uint64_t off = (uint64_t)r * a.ncoeff + c;
    uint64_t k0[V], k1[V];
    Lane<V>::load((const T*)a.pk0 + off, k0);
    Lane<V>::load((const T*)a.pk1 + off, k1);
    const uint64_t p0 = blockIdx.z * a.prun;
    const uint64_t p1 = p0 + a.prun < a.npoly ? p0 + a.prun : a.npoly;
    for (uint64_t p = p0; p < p1; ++p) {
        const T* w = (const T*)a.ws + p * a.dense_stride + off;
        uint64_t u[V], e0[V], e1[V], m[V], o0[V], o1[V];
        Lane<V>::load(w, u);
        Lane<V>::load(w + a.set_stride, e0);
        Lane<V>::load(w + 2 * a.set_stride, e1);
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = 0;
        if (a.m) Lane<V>::load((const T*)a.m + p * a.m_stride + off, m);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            o0[k] = barrett128((u128)k0[k] * u[k] + e0[k] + m[k], q, r0, r1);
            o1[k] = barrett128((u128)k1[k] * u[k] + e1[k], q, r0, r1);
        }
        Lane<V>::store((T*)a.c0 + p * a.out_stride + off, o0);
        Lane<V>::store((T*)a.c1 + p * a.out_stride + off, o1);
    }
}

template <int V>
__global__ __launch_bounds__(256) void rlwe_dec_kernel(RlweDecArgs a) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const uint64_t q = a.dmod[3 * r], r0 = a.dmod[3 * r + 1], r1 = a.dmod[3 * r + 2];
    const uint64_t off = (uint64_t)r * a.ncoeff + c;
    uint64_t sv[V];
    Lane<V>::load((const T*)a.s + off, sv);
    const uint64_t p0 = blockIdx.z * a.prun;
    const uint64_t p1 = p0 + a.prun < a.npoly ? p0 + a.prun : a.npoly;
    for (uint64_t p = p0; p < p1; ++p) {
        uint64_t x0[V], x1[V], o[V];
        Lane<V>::load((const T*)a.c0 + p * a.in_stride + off, x0);
        Lane<V>::load((const T*)a.c1 + p * a.in_stride + off, x1);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = barrett128((u128)x1[k] * sv[k] + x0[k], q, r0, r1);
        Lane<V>::store((T*)a.out + p * a.out_stride + off, o);
    }
}

// ---- argument checks (nothing here touches the device) ----
static int check_ctx(const mfhe_ctx* c) {
    RC(ks_check_ctx(c));
    if (c->logN < 3) return set_error(MFHE_EUNSUPPORTED, "rlwe: log_n must be >= 3");
    return MFHE_OK;
}

static int check_rows(const mfhe_ctx* c, int level, int special_start, int nspecial, const char* what) {
    const std::string w(what);
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, w + ": level outside the context");
    if (nspecial < 0) return set_error(MFHE_EINVAL, w + ": nspecial < 0");
    if (nspecial > 0) RC(ks_check_geom(c, KsGeom{level, level, special_start, nspecial}, what));
    for (int r = 0; r < level + nspecial; ++r)
        if (c->moduli[r < level ? r : special_start + r - level] <= (uint64_t)kRlweNoiseBits)
            return set_error(MFHE_EUNSUPPORTED, w + ": a modulus does not exceed the noise's range");
    return MFHE_OK;
}

static RlweSeed load_seed(const uint32_t* seed) {
    RlweSeed s;
    for (int i = 0; i < 8; ++i) s.w[i] = seed[i];
    return s;
}

static bool aligned16(std::initializer_list<const void*> ptrs, std::initializer_list<uint64_t> strides) {
    uintptr_t bits = 0;
    uint64_t odd = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    for (uint64_t s : strides) odd |= s;
    return !(bits & 15) && !(odd & 1);
}

// ---- launches (arguments checked) ----
template <bool LIFT>
static int launch_small(const RlweSmallArgs& a, hipStream_t st) {
    const uint64_t total = a.npoly * (uint64_t)a.nsets;
    const KsRowGrid rg = ks_row_grid(((uint64_t)1 << a.logN) >> 3);
    const KsFold f = ks_fold(total);
    if (rg.bx > 0x7fffffffull || f.gz > 65535) return set_error(MFHE_EINVAL, "rlwe: too many polynomials for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)f.gy, (uint32_t)f.gz);
    if (aligned16({a.res0, a.res1}, {a.stride0, a.stride1}))
        hipLaunchKernelGGL((rlwe_small_kernel<LIFT, true>), grid, dim3(rg.block), 0, st, a);
    else
        hipLaunchKernelGGL((rlwe_small_kernel<LIFT, false>), grid, dim3(rg.block), 0, st, a);
    MFHE_CHECK_LAUNCH("rlwe_small_kernel");
    return MFHE_OK;
}

static int launch_mask(RlweMaskArgs a, hipStream_t st) {
    const KsRowGrid rg = ks_row_grid(((uint64_t)1 << a.logN) >> 2);
    const uint64_t rows = (uint64_t)a.level + a.nspecial;
    if (rg.bx > 0x7fffffffull || rows > 65535) return set_error(MFHE_EINVAL, "rlwe: too large for one launch");
    const KsRuns run = ks_runs(a.npoly, rg.bx, rows, kRlweMinRun);
    a.prun = run.prun;
    const dim3 grid((uint32_t)rg.bx, (uint32_t)rows, (uint32_t)run.runs);
    if (aligned16({a.out0, a.out1, a.e0, a.e1, a.s, a.add}, {a.out_stride, a.e_stride0, a.e_stride1, a.add_stride}))
        hipLaunchKernelGGL(rlwe_mask_kernel<true>, grid, dim3(rg.block), 0, st, a);
    else
        hipLaunchKernelGGL(rlwe_mask_kernel<false>, grid, dim3(rg.block), 0, st, a);
    MFHE_CHECK_LAUNCH("rlwe_mask_kernel");
    return MFHE_OK;
}

// The small polynomials of `a` (res0 .. stride1 filled in here) into the dense blocks at the workspace's start,
// forward-transformed: *blk0 [total][level][N], *blk1 [total][nspecial][N].
template <bool LIFT>
static int small_to_ws(mfhe_ctx* c, RlweSmallArgs a, uint64_t** blk0, uint64_t** blk1, mfhe_stream_t s) {
    const size_t N = c->N, total = a.npoly * (size_t)a.nsets;
    RC(grow_ws(c, total * ((size_t)a.level + a.nspecial) * N * 8));
    uint64_t* ws = (uint64_t*)c->ws;
    a.res0 = ws;
    a.stride0 = (size_t)a.level * N;
    a.res1 = ws + total * (size_t)a.level * N;
    a.stride1 = (size_t)a.nspecial * N;
    RC(launch_small<LIFT>(a, (hipStream_t)s));
    RC(mfhe_ntt_fwd(c, a.res0, total, 0, a.level, s));
    if (a.nspecial > 0) RC(mfhe_ntt_fwd(c, a.res1, total, a.special_start, a.nspecial, s));
    *blk0 = a.res0;
    *blk1 = a.res1;
    return MFHE_OK;
}

static RlweSmallArgs small_args(const mfhe_ctx* c, size_t npoly, int level, int special_start, int nspecial) {
    RlweSmallArgs a{};
    a.dmod = c->d_dmod;
    a.npoly = npoly;
    a.nsets = 1;
    a.logN = c->logN;
    a.level = level;
    a.special_start = special_start;
    a.nspecial = nspecial;
    return a;
}

// the body of sample_small and lift_small: `a` has its source; checks done
template <bool LIFT>
static int small_body(mfhe_ctx* c, RlweSmallArgs a, uint64_t* d_out, size_t out_poly_stride, bool coeff,
                      mfhe_stream_t s) {
    const size_t N = c->N;
    hipStream_t st = (hipStream_t)s;
    if (coeff) {
        a.res0 = d_out;
        a.res1 = d_out + (size_t)a.level * N;
        a.stride0 = a.stride1 = out_poly_stride;
        return launch_small<LIFT>(a, st);
    }
    uint64_t *b0, *b1;
    RC(small_to_ws<LIFT>(c, a, &b0, &b1, s));
    RC(launch_copy_rows(b0, (size_t)a.level * N, d_out, out_poly_stride, a.npoly, (size_t)a.level * N, st));
    if (a.nspecial > 0)
        RC(launch_copy_rows(b1, (size_t)a.nspecial * N, d_out + (size_t)a.level * N, out_poly_stride, a.npoly,
                            (size_t)a.nspecial * N, st));
    return MFHE_OK;
}

}  // namespace rlwe
}  // namespace mfhe

using namespace mfhe;
using namespace mfhe::rlwe;

extern "C" int mfhe_rlwe_reserve(mfhe_ctx* c, size_t npoly, int level, int special_start, int nspecial) {
    RC(check_ctx(c));
    RC(check_rows(c, level, special_start, nspecial, "rlwe_reserve"));
    if (nspecial > 0) {
        const uint64_t* pmod;
        RC(ksk_pmod_table(c, level, special_start, nspecial, &pmod));
    }
    return grow_ws(c, rlwe_ws_words(npoly, (size_t)level, (size_t)nspecial, c->N) * 8);
}

extern "C" int mfhe_rlwe_sample_uniform(mfhe_ctx* c, const uint32_t* seed, uint64_t first_id, uint64_t* d_out,
                                        size_t out_poly_stride, size_t npoly, int level, int special_start,
                                        int nspecial, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!seed || !d_out) return set_error(MFHE_EINVAL, "rlwe_sample_uniform: null pointer");
    RC(check_rows(c, level, special_start, nspecial, "rlwe_sample_uniform"));
    if (out_poly_stride < ((size_t)level + nspecial) * c->N)
        return set_error(MFHE_EINVAL, "rlwe_sample_uniform: poly stride smaller than rows * N");
    if (npoly == 0) return MFHE_OK;
    RlweMaskArgs a{};
    a.seed = load_seed(seed); a.first_id = first_id;
    a.out1 = d_out; a.out_stride = out_poly_stride;
    a.dmod = c->d_dmod; a.npoly = npoly; a.kind = kRlweMaskOnly; a.alpha = 1;
    a.logN = c->logN; a.level = level; a.special_start = special_start; a.nspecial = nspecial;
    return launch_mask(a, (hipStream_t)s);
}

extern "C" int mfhe_rlwe_sample_small(mfhe_ctx* c, const uint32_t* seed, int stream, uint64_t first_id, uint64_t* d_out,
                                      size_t out_poly_stride, size_t npoly, int level, int special_start, int nspecial,
                                      int flags, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!seed || !d_out) return set_error(MFHE_EINVAL, "rlwe_sample_small: null pointer");
    if (!rlwe_stream_is_small(stream)) return set_error(MFHE_EINVAL, "rlwe_sample_small: not a stream of small integers");
    if (flags & ~MFHE_RLWE_COEFF) return set_error(MFHE_EINVAL, "rlwe_sample_small: unknown flag");
    RC(check_rows(c, level, special_start, nspecial, "rlwe_sample_small"));
    if (out_poly_stride < ((size_t)level + nspecial) * c->N)
        return set_error(MFHE_EINVAL, "rlwe_sample_small: poly stride smaller than rows * N");
    if (npoly == 0) return MFHE_OK;
    RlweSmallArgs a = small_args(c, npoly, level, special_start, nspecial);
    a.seed = load_seed(seed); a.first_id = first_id; a.stream0 = stream;
    return small_body<false>(c, a, d_out, out_poly_stride, flags & MFHE_RLWE_COEFF, s);
}

extern "C" int mfhe_rlwe_lift_small(mfhe_ctx* c, const int32_t* d_coeffs, size_t coeff_stride, uint64_t* d_out,
                                    size_t out_poly_stride, size_t npoly, int level, int special_start, int nspecial,
                                    int flags, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!d_coeffs || !d_out) return set_error(MFHE_EINVAL, "rlwe_lift_small: null pointer");
    if (flags & ~MFHE_RLWE_COEFF) return set_error(MFHE_EINVAL, "rlwe_lift_small: unknown flag");
    RC(check_rows(c, level, special_start, nspecial, "rlwe_lift_small"));
    const size_t N = c->N, rows = (size_t)level + nspecial;
    if (coeff_stride < N) return set_error(MFHE_EINVAL, "rlwe_lift_small: coefficient stride smaller than N");
    if (out_poly_stride < rows * N) return set_error(MFHE_EINVAL, "rlwe_lift_small: poly stride smaller than rows * N");
    // the coefficients' span in 8-byte words, rounded out to whole words
    const uintptr_t cb = (uintptr_t)d_coeffs, ce = cb + 4 * ks_span(npoly, coeff_stride, N);
    if (ks_ranges_overlap((const uint64_t*)(cb & ~(uintptr_t)7), (((ce + 7) & ~(uintptr_t)7) - (cb & ~(uintptr_t)7)) / 8,
                          d_out, ks_span(npoly, out_poly_stride, rows * N)))
        return set_error(MFHE_EINVAL, "rlwe_lift_small: the coefficients overlap the output");
    if (npoly == 0) return MFHE_OK;
    RlweSmallArgs a = small_args(c, npoly, level, special_start, nspecial);
    a.coeffs = d_coeffs; a.coeff_stride = coeff_stride;
    return small_body<true>(c, a, d_out, out_poly_stride, flags & MFHE_RLWE_COEFF, s);
}

extern "C" int mfhe_rlwe_encrypt_sk(mfhe_ctx* c, const uint32_t* seed, uint64_t first_id, const uint64_t* d_s,
                                    const uint64_t* d_m, size_t m_poly_stride, uint64_t* d_c0, uint64_t* d_c1,
                                    size_t out_poly_stride, size_t npoly, int level, int special_start, int nspecial,
                                    mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!seed || !d_s || !d_c0 || !d_c1) return set_error(MFHE_EINVAL, "rlwe_encrypt_sk: null pointer");
    RC(check_rows(c, level, special_start, nspecial, "rlwe_encrypt_sk"));
    const size_t N = c->N, pw = ((size_t)level + nspecial) * N;
    if (out_poly_stride < pw || (d_m && m_poly_stride < pw))
        return set_error(MFHE_EINVAL, "rlwe_encrypt_sk: poly stride smaller than rows * N");
    const size_t osp = ks_span(npoly, out_poly_stride, pw);
    RC(ks_check_overlap("rlwe_encrypt_sk", {{d_s, pw}, {d_m, d_m ? ks_span(npoly, m_poly_stride, pw) : 0}},
                        {{d_c0, osp}, {d_c1, osp}}));
    if (npoly == 0) return MFHE_OK;
    RlweSmallArgs sa = small_args(c, npoly, level, special_start, nspecial);
    sa.seed = load_seed(seed); sa.first_id = first_id; sa.stream0 = kRlweNoise;
    uint64_t *b0, *b1;
    RC(small_to_ws<false>(c, sa, &b0, &b1, s));
    RlweMaskArgs a{};
    a.seed = sa.seed; a.first_id = first_id;
    a.out0 = d_c0; a.out1 = d_c1; a.out_stride = out_poly_stride;
    a.e0 = b0; a.e1 = b1; a.e_stride0 = (size_t)level * N; a.e_stride1 = (size_t)nspecial * N;
    a.s = d_s; a.add = d_m; a.add_stride = d_m ? m_poly_stride : 0;
    a.dmod = c->d_dmod; a.npoly = npoly; a.kind = d_m ? kRlweEncMsg : kRlweEncZero; a.alpha = 1;
    a.logN = c->logN; a.level = level; a.special_start = special_start; a.nspecial = nspecial;
    return launch_mask(a, (hipStream_t)s);
}

extern "C" int mfhe_rlwe_ksk_gen(mfhe_ctx* c, const uint32_t* seed, uint64_t first_id, int kind, int galois_elt,
                                 const uint64_t* d_s_from, const uint64_t* d_s_to, uint64_t* d_ksk, int key_level,
                                 int alpha, int special_start, int nspecial, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (kind != MFHE_RLWE_KEY_SWITCH && kind != MFHE_RLWE_KEY_RELIN && kind != MFHE_RLWE_KEY_GALOIS)
        return set_error(MFHE_EINVAL, "rlwe_ksk_gen: unknown kind");
    if (!seed || !d_s_to || !d_ksk || (kind == MFHE_RLWE_KEY_SWITCH && !d_s_from))
        return set_error(MFHE_EINVAL, "rlwe_ksk_gen: null pointer");
    const KsGeom g{key_level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "rlwe_ksk_gen"));
    RC(check_rows(c, key_level, special_start, nspecial, "rlwe_ksk_gen"));
    if (kind == MFHE_RLWE_KEY_GALOIS) RC(ks_check_galois(c, galois_elt, "rlwe_ksk_gen"));
    const size_t N = c->N, rows = (size_t)g.key_rows(), beta = (size_t)ks_beta(key_level, alpha);
    if (kind != MFHE_RLWE_KEY_SWITCH) d_s_from = nullptr;
    RC(ks_check_overlap("rlwe_ksk_gen", {{d_s_from, d_s_from ? rows * N : 0}, {d_s_to, rows * N}},
                        {{d_ksk, beta * 2 * rows * N}}));
    const uint64_t* pmod = nullptr;
    RC(ksk_pmod_table(c, key_level, special_start, nspecial, &pmod));
    RlweSmallArgs sa = small_args(c, beta, key_level, special_start, nspecial);
    sa.seed = load_seed(seed); sa.first_id = first_id; sa.stream0 = kRlweNoise;
    uint64_t *b0, *b1;
    RC(small_to_ws<false>(c, sa, &b0, &b1, s));
    RlweMaskArgs a{};
    a.seed = sa.seed; a.first_id = first_id;
    a.out0 = d_ksk; a.out1 = d_ksk + rows * N; a.out_stride = 2 * rows * N;
    a.e0 = b0; a.e1 = b1; a.e_stride0 = (size_t)key_level * N; a.e_stride1 = (size_t)nspecial * N;
    a.s = d_s_to; a.add = d_s_from; a.pmod = pmod;
    a.dmod = c->d_dmod; a.npoly = beta; a.alpha = alpha; a.galois_elt = (uint32_t)galois_elt;
    a.kind = kind == MFHE_RLWE_KEY_SWITCH ? kRlweKeySwitch : kind == MFHE_RLWE_KEY_RELIN ? kRlweKeyRelin : kRlweKeyGalois;
    a.logN = c->logN; a.level = key_level; a.special_start = special_start; a.nspecial = nspecial;
    return launch_mask(a, (hipStream_t)s);
}

extern "C" int mfhe_rlwe_encrypt_pk(mfhe_ctx* c, const uint32_t* seed, uint64_t first_id, const uint64_t* d_pk0,
                                    const uint64_t* d_pk1, const uint64_t* d_m, size_t m_poly_stride, uint64_t* d_c0,
                                    uint64_t* d_c1, size_t out_poly_stride, size_t npoly, int level, mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!seed || !d_pk0 || !d_pk1 || !d_c0 || !d_c1) return set_error(MFHE_EINVAL, "rlwe_encrypt_pk: null pointer");
    RC(check_rows(c, level, 0, 0, "rlwe_encrypt_pk"));
    const size_t N = c->N, pw = (size_t)level * N;
    if (out_poly_stride < pw || (d_m && m_poly_stride < pw))
        return set_error(MFHE_EINVAL, "rlwe_encrypt_pk: poly stride smaller than level * N");
    const size_t osp = ks_span(npoly, out_poly_stride, pw);
    RC(ks_check_overlap("rlwe_encrypt_pk",
                        {{d_pk0, pw}, {d_pk1, pw}, {d_m, d_m ? ks_span(npoly, m_poly_stride, pw) : 0}},
                        {{d_c0, osp}, {d_c1, osp}}));
    if (npoly == 0) return MFHE_OK;
    hipStream_t st = (hipStream_t)s;
    RlweSmallArgs sa = small_args(c, npoly, level, 0, 0);
    sa.seed = load_seed(seed); sa.first_id = first_id;
    sa.nsets = 3; sa.stream0 = kRlweEphemeral; sa.stream1 = kRlweNoise0; sa.stream2 = kRlweNoise1;
    uint64_t *b0, *b1;
    RC(small_to_ws<false>(c, sa, &b0, &b1, s));
    RlwePkArgs a{};
    a.pk0 = d_pk0; a.pk1 = d_pk1; a.ws = b0; a.m = d_m; a.c0 = d_c0; a.c1 = d_c1;
    a.set_stride = npoly * pw; a.dense_stride = pw; a.m_stride = d_m ? m_poly_stride : 0; a.out_stride = out_poly_stride;
    a.ncoeff = N; a.npoly = npoly; a.dmod = c->d_dmod;
    const bool wide = ks_wide({&a.ncoeff, &a.set_stride, &a.dense_stride, &a.m_stride, &a.out_stride},
                              {a.pk0, a.pk1, a.ws, a.m, a.c0, a.c1});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull) return set_error(MFHE_EINVAL, "rlwe_encrypt_pk: too large for one launch");
    const KsRuns run = ks_runs(npoly, rg.bx, (uint64_t)level, kRlweMinRun);
    a.prun = run.prun;
    const dim3 grid((uint32_t)rg.bx, (uint32_t)level, (uint32_t)run.runs);
    if (wide)
        hipLaunchKernelGGL(rlwe_pk_kernel<2>, grid, dim3(rg.block), 0, st, a);
    else
        hipLaunchKernelGGL(rlwe_pk_kernel<1>, grid, dim3(rg.block), 0, st, a);
    MFHE_CHECK_LAUNCH("rlwe_pk_kernel");
    return MFHE_OK;
}

extern "C" int mfhe_rlwe_decrypt(mfhe_ctx* c, const uint64_t* d_c0, const uint64_t* d_c1, size_t in_poly_stride,
                                 const uint64_t* d_s, uint64_t* d_out, size_t out_poly_stride, size_t npoly, int rows,
                                 mfhe_stream_t s) {
    RC(check_ctx(c));
    if (!d_c0 || !d_c1 || !d_s || !d_out) return set_error(MFHE_EINVAL, "rlwe_decrypt: null pointer");
    if (rows < 1 || rows > c->L) return set_error(MFHE_EINVAL, "rlwe_decrypt: rows outside the context");
    const size_t N = c->N, pw = (size_t)rows * N;
    if (in_poly_stride < pw || out_poly_stride < pw)
        return set_error(MFHE_EINVAL, "rlwe_decrypt: poly stride smaller than rows * N");
    const size_t isp = ks_span(npoly, in_poly_stride, pw);
    RC(ks_check_overlap("rlwe_decrypt", {{d_c0, isp}, {d_c1, isp}, {d_s, pw}},
                        {{d_out, ks_span(npoly, out_poly_stride, pw)}}));
    if (npoly == 0) return MFHE_OK;
    RlweDecArgs a{};
    a.c0 = d_c0; a.c1 = d_c1; a.s = d_s; a.out = d_out;
    a.in_stride = in_poly_stride; a.out_stride = out_poly_stride; a.ncoeff = N; a.npoly = npoly; a.dmod = c->d_dmod;
    const bool wide = ks_wide({&a.ncoeff, &a.in_stride, &a.out_stride}, {a.c0, a.c1, a.s, a.out});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    if (rg.bx > 0x7fffffffull) return set_error(MFHE_EINVAL, "rlwe_decrypt: too large for one launch");
    const KsRuns run = ks_runs(npoly, rg.bx, (uint64_t)rows, kRlweMinRun);
    a.prun = run.prun;
    const dim3 grid((uint32_t)rg.bx, (uint32_t)rows, (uint32_t)run.runs);
    if (wide)
        hipLaunchKernelGGL(rlwe_dec_kernel<2>, grid, dim3(rg.block), 0, (hipStream_t)s, a);
    else
        hipLaunchKernelGGL(rlwe_dec_kernel<1>, grid, dim3(rg.block), 0, (hipStream_t)s, a);
    MFHE_CHECK_LAUNCH("rlwe_dec_kernel");
    return MFHE_OK;
}

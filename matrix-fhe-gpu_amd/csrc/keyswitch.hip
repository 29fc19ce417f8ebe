// keyswitch.hip -- hybrid key switching for gfx950: switching-key assembly, the digit-by-key inner product and the
// driver that chains ModUp, inner product and ModDown (include/mfhe.h mfhe_ksk_assemble, mfhe_ksk_inner_product,
// mfhe_keyswitch).
//
// Everything is in the evaluation domain (phantom NTT) and canonical.  Digits are runs of alpha consecutive Q limbs;
// a call at `level` has beta = ceil(level / alpha) of them.  A (level + K)-row block has modulus limb r on row
// r < level, else limb special_start + r - level; a key made at key_level keeps its special rows at key rows
// key_level .. key_level + K - 1 and serves every level <= key_level.
//
//   assemble      : ksk[j][1] = a_j, ksk[j][0][r] = e_j - a_j s_to + F s_from mod q_r, F = P mod q_r when limb r lies
//                   in digit j, else 0 (P = product of the special moduli)
//   inner product : acc[p][c][r] = sum_j raised[j][p][r] ksk[j][c][keyrow(r)] mod q_r
//   keyswitch     : raise every digit (ModUp), inner product, ModDown both components by the special limbs
//
// Inner product design: one thread owns one (row, coefficient) -- two adjacent coefficients with 16-byte loads and
// stores when the layout allows -- and walks a run of polynomials with its slice of the key held in registers
// (ndigits <= kKsipUnroll; longer keys are re-read per polynomial, from the cache).  Both components accumulate as
// unreduced u128 sums (products of canonical residues of moduli < 2^62 are < 2^124, so 16 fit; longer sums reduce
// every 16 terms) and end in one 128-bit Barrett reduction against d_dmod.  The row is the grid's y index, so the
// modulus constants are wave-uniform scalar loads.  The Galois forms (galois.hip) use the same kernel with the raised
// digits read through the gather pi_g of galois.hpp, a template parameter.
#include "keyswitch.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "galois.hpp"
#include "host_math.hpp"
#include "mod128.hpp"

namespace mfhe {

// largest digit count whose key slice stays in registers: 2 * 6 * 2 u64 at two coefficients
constexpr int kKsipUnroll = 6;
// shortest run of polynomials one thread walks with its key slice (the whole batch when it is smaller)
constexpr uint64_t kKsipMinRun = 4;

// A raised element (V words) as the thread uses it: the pair swapped when the Galois gather asks for it.
template <int V, bool PERM>
static __device__ __forceinline__ void load_raised(const typename Lane<V>::T* p, bool swap, uint64_t (&x)[V]) {
    Lane<V>::load(p, x);
    if constexpr (PERM && V == 2) {
        const uint64_t lo = swap ? x[V - 1] : x[0], hi = swap ? x[0] : x[V - 1];
        x[0] = lo;
        x[V - 1] = hi;
    }
}

// ND: digits (template-unrolled, the key slice in registers) or 0 (generic loop over a.ndigits); V: coefficients per
// thread.  dmod is a __restrict__ kernel parameter, indexed by the block's row: scalar loads.  PERM: the raised digits
// are read through the Galois gather pi_g (galois.hpp) -- element pi(c), or the pair pi(2c) >> 1 swapped when pi(2c)
// is odd; the index is computed once, before the polynomial loop, and the key and the output keep index c.
template <int ND, int V, bool PERM>
__global__ __launch_bounds__(256) void ksk_inner_product_kernel(KsipArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    uint64_t cs = c;        // where the raised digits are read
    bool swap = false;
    if constexpr (PERM) {
        const uint32_t src = galois_perm_index((uint32_t)c * V, a.galois_elt, a.log_n);
        cs = V == 2 ? src >> 1 : src;
        swap = V == 2 && (src & 1u);
    }
    const int r = blockIdx.y;
    const int level = a.g.level, rows = level + a.g.nspecial;
    const int limb = r < level ? r : a.g.special_start + r - level;
    const int krow = r < level ? r : a.g.key_level + r - level;
    const uint64_t q = dmod[3 * limb], r0 = dmod[3 * limb + 1], r1 = dmod[3 * limb + 2];
    const uint64_t kcs = (uint64_t)(a.g.key_level + a.g.nspecial) * a.ncoeff;   // one key component
    const T* key = (const T*)a.ksk + (uint64_t)krow * a.ncoeff + c;
    const T* rp = (const T*)a.raised + (uint64_t)r * a.ncoeff + cs;
    T* op = (T*)a.acc + (uint64_t)r * a.ncoeff + c;
    const uint64_t p0 = blockIdx.z * a.prun;
    const uint64_t p1 = p0 + a.prun < a.npoly ? p0 + a.prun : a.npoly;
    const uint64_t cstride = (uint64_t)rows * a.ncoeff;   // one component of acc

    if (ND) {
        constexpr int NK = ND ? ND : 1;
        uint64_t k0[NK][V], k1[NK][V];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            Lane<V>::load(key + (uint64_t)(2 * j) * kcs, k0[j]);
            Lane<V>::load(key + (uint64_t)(2 * j + 1) * kcs, k1[j]);
        }
        for (uint64_t p = p0; p < p1; ++p) {
            uint64_t x[NK][V];
#pragma unroll
            for (int j = 0; j < NK; ++j)
                load_raised<V, PERM>(rp + (uint64_t)j * a.digit_stride + p * a.poly_stride, swap, x[j]);
            u128 s0[V], s1[V];
#pragma unroll
            for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0;
#pragma unroll
            for (int j = 0; j < NK; ++j)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    s0[k] += (u128)x[j][k] * k0[j][k];
                    s1[k] += (u128)x[j][k] * k1[j][k];
                }
            uint64_t o0[V], o1[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                o0[k] = barrett128(s0[k], q, r0, r1);
                o1[k] = barrett128(s1[k], q, r0, r1);
            }
            Lane<V>::store(op + p * a.acc_stride, o0);
            Lane<V>::store(op + p * a.acc_stride + cstride, o1);
        }
    } else {
        for (uint64_t p = p0; p < p1; ++p) {
            uint64_t o0[V], o1[V];
#pragma unroll
            for (int k = 0; k < V; ++k) o0[k] = o1[k] = 0;
            for (int j0 = 0; j0 < a.ndigits; j0 += 16) {   // 16 products < 2^124 and a residue < 2^62 fit a u128
                u128 s0[V], s1[V];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    s0[k] = o0[k];
                    s1[k] = o1[k];
                }
                const int j1 = j0 + 16 < a.ndigits ? j0 + 16 : a.ndigits;
                for (int j = j0; j < j1; ++j) {
                    uint64_t x[V], ka[V], kb[V];
                    load_raised<V, PERM>(rp + (uint64_t)j * a.digit_stride + p * a.poly_stride, swap, x);
                    Lane<V>::load(key + (uint64_t)(2 * j) * kcs, ka);
                    Lane<V>::load(key + (uint64_t)(2 * j + 1) * kcs, kb);
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        s0[k] += (u128)x[k] * ka[k];
                        s1[k] += (u128)x[k] * kb[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    o0[k] = barrett128(s0[k], q, r0, r1);
                    o1[k] = barrett128(s1[k], q, r0, r1);
                }
            }
            Lane<V>::store(op + p * a.acc_stride, o0);
            Lane<V>::store(op + p * a.acc_stride + cstride, o1);
        }
    }
}

// One thread per (digit j, key row r, coefficient): ksk[j][1][r] = a_j[r], ksk[j][0][r] = e_j[r] - a_j[r] s_to[r] +
// F s_from[r] mod q_r, F = pmod[r] on the rows of digit j and 0 elsewhere (the special rows included).
__global__ __launch_bounds__(256) void ksk_assemble_kernel(const uint64_t* __restrict__ s_from,
                                                           const uint64_t* __restrict__ s_to,
                                                           const uint64_t* __restrict__ av,
                                                           const uint64_t* __restrict__ ev, uint64_t* __restrict__ ksk,
                                                           int key_level, int key_rows, int alpha, int special_start,
                                                           int logN, const uint64_t* __restrict__ pmod,
                                                           const uint64_t* __restrict__ dmod, uint64_t total) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t row = i >> logN, c = i & ((1ull << logN) - 1);
    const uint64_t j = row / (uint64_t)key_rows, r = row - j * (uint64_t)key_rows;
    const uint64_t limb = r < (uint64_t)key_level ? r : (uint64_t)special_start + r - key_level;
    const uint64_t q = dmod[3 * limb], r0 = dmod[3 * limb + 1], r1 = dmod[3 * limb + 2];
    const uint64_t F = (r < (uint64_t)key_level && r / (uint64_t)alpha == j) ? pmod[r] : 0;
    const uint64_t sk = (r << logN) + c;
    const uint64_t aa = av[i], as = barrett128((u128)aa * s_to[sk], q, r0, r1);
    const uint64_t b = barrett128((u128)F * s_from[sk] + ev[i] + (q - as), q, r0, r1);
    const uint64_t o = ((j * 2 * (uint64_t)key_rows + r) << logN) + c;
    ksk[o] = b;
    ksk[o + ((uint64_t)key_rows << logN)] = aa;
}

using KsipKernel = void (*)(KsipArgs, const uint64_t*);

// PERM: the instantiations that read the raised digits through a Galois gather
template <int V, bool PERM>
static KsipKernel pick_ksip(int nd) {
    switch (nd) {
        case 1: return ksk_inner_product_kernel<1, V, PERM>;
        case 2: return ksk_inner_product_kernel<2, V, PERM>;
        case 3: return ksk_inner_product_kernel<3, V, PERM>;
        case 4: return ksk_inner_product_kernel<4, V, PERM>;
        case 5: return ksk_inner_product_kernel<5, V, PERM>;
        case 6: return ksk_inner_product_kernel<6, V, PERM>;
        default: return ksk_inner_product_kernel<0, V, PERM>;
    }
}
static_assert(kKsipUnroll == 6, "pick_ksip lists the unrolled digit counts");

int launch_ksk_inner_product(mfhe_ctx* c, KsipArgs a, hipStream_t st) {
    if (a.npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    a.log_n = 0;
    if (a.galois_elt) {   // the gather is defined on power-of-two rows, for an odd element below 2 N
        while ((1ull << a.log_n) < a.ncoeff) ++a.log_n;
        if ((1ull << a.log_n) != a.ncoeff || a.log_n > 30 || !(a.galois_elt & 1u) || a.galois_elt >= 2 * a.ncoeff)
            return set_error(MFHE_EINVAL, "ksk_inner_product: Galois element is not an odd integer in [1, 2 N)");
    }
    const bool wide = ks_wide({&a.ncoeff, &a.digit_stride, &a.poly_stride, &a.acc_stride}, {a.raised, a.ksk, a.acc});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    const uint64_t rows = (uint64_t)a.g.rows();
    if (rg.bx > 0x7fffffffull || rows > 65535)
        return set_error(MFHE_EINVAL, "ksk_inner_product: too large for one launch");
    const KsRuns run = ks_runs(a.npoly, rg.bx, rows, kKsipMinRun);   // a thread keeps its key slice across a run
    a.prun = run.prun;
    const KsipKernel k = a.galois_elt ? (wide ? pick_ksip<2, true>(a.ndigits) : pick_ksip<1, true>(a.ndigits))
                                      : (wide ? pick_ksip<2, false>(a.ndigits) : pick_ksip<1, false>(a.ndigits));
    hipLaunchKernelGGL(k, dim3((uint32_t)rg.bx, (uint32_t)rows, (uint32_t)run.runs), dim3(rg.block), 0, st, a,
                       (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("ksk_inner_product_kernel");
    return MFHE_OK;
}

// [key_level] P mod q_r, cached per (key_level, special range); built and uploaded on first use
int ksk_pmod_table(mfhe_ctx* c, int key_level, int sp, int nsp, const uint64_t** tab) {
    std::lock_guard<std::mutex> lock(c->bconv_mu);
    for (const auto& e : c->ksk_tabs)
        if (e.key_level == key_level && e.special_start == sp && e.nspecial == nsp) {
            *tab = e.d_pmod;
            return MFHE_OK;
        }
    std::vector<uint64_t> h(key_level);
    for (int r = 0; r < key_level; ++r) {
        const uint64_t q = c->moduli[r];
        uint64_t v = 1 % q;
        for (int k = 0; k < nsp; ++k) v = hm::mulmod(v, c->moduli[sp + k] % q, q);
        h[r] = v;
    }
    void* d = nullptr;
    MFHE_HIP(hipMalloc(&d, h.size() * 8));
    hipError_t e = hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_error(e, "hipMemcpy (switching key table)");
    }
    c->allocs.push_back(d);
    c->ksk_tabs.push_back({key_level, sp, nsp, (uint64_t*)d});
    *tab = (const uint64_t*)d;
    return MFHE_OK;
}

// ---- argument checks (nothing here touches the device) ----
int ks_check_ctx(const mfhe_ctx* c) {
    if (!c) return set_error(MFHE_EINVAL, "null ctx");
    if (!(c->conv & MFHE_CONV_PHANTOM)) return set_error(MFHE_ENOTREADY, "context was created without MFHE_CONV_PHANTOM");
    return MFHE_OK;
}

int ks_check_geom(const mfhe_ctx* c, const KsGeom& g, const char* what) {
    const std::string w(what);
    if (g.nspecial < 1) return set_error(MFHE_EINVAL, w + ": nspecial < 1");
    if (g.key_level < 1 || g.key_level > c->L) return set_error(MFHE_EINVAL, w + ": key_level outside the context");
    if (g.level < 1) return set_error(MFHE_EINVAL, w + ": level < 1");
    if (g.level > g.key_level) return set_error(MFHE_EINVAL, w + ": level > key_level");
    if (g.special_start < g.key_level) return set_error(MFHE_EINVAL, w + ": special limbs overlap [0, key_level)");
    if (g.special_start > c->L || g.nspecial > c->L - g.special_start)
        return set_error(MFHE_EINVAL, w + ": special limbs outside the context");
    return MFHE_OK;
}

int ks_check_galois(const mfhe_ctx* c, int galois_elt, const char* what) {
    if (galois_elt < 1 || !(galois_elt & 1) || (uint64_t)galois_elt >= 2 * (uint64_t)c->N)
        return set_error(MFHE_EINVAL, std::string(what) + ": Galois element is not an odd integer in [1, 2 N)");
    return MFHE_OK;
}

int ks_check_digits(const mfhe_ctx* c, int alpha, const KsGeom& g, const char* what) {
    if (alpha < 1) return set_error(MFHE_EINVAL, std::string(what) + ": alpha < 1");
    return ks_check_geom(c, g, what);
}

int ks_check_overlap(const std::string& w, const KsRange* in, size_t nin, const KsRange* out, size_t nout) {
    const int o = ks_find_overlap(in, nin, out, nout);
    if (o == kKsNoOverlap) return MFHE_OK;
    return set_error(MFHE_EINVAL, w + (o == kKsInputOverlap ? ": an input overlaps an output" : ": the outputs overlap"));
}

// ---- tables and workspace ----
static int ks_tables(mfhe_ctx* c, const KsGeom& g, int alpha, KsTables& t) {
    t.beta = ks_beta(g.level, alpha);
    t.plan.assign(t.beta, ModUpPlan{});
    t.tab.assign((size_t)3 * t.beta, nullptr);
    for (int j = 0; j < t.beta; ++j) {
        const int ds = j * alpha, dc = g.level - ds < alpha ? g.level - ds : alpha;
        RC(check_modup(c, g.level, ds, dc, g.special_start, g.nspecial, t.plan[j]));
        RC(ntt_modup_tables(c, ds, dc, t.plan[j], &t.tab[(size_t)3 * j]));
    }
    return bconv_table(c, g.special_start, g.nspecial, 0, g.level, &t.down);
}

int ks_prepare(mfhe_ctx* c, const KsGeom& g, int alpha, int extra, size_t ws_words, KsTables& t) {
    RC(ks_tables(c, g, alpha, t));
    if (extra & kKsRescale) RC(bconv_table(c, g.level - 1, 1, 0, g.level - 1, &t.rescale));
    if (extra & kKsPmod) RC(ksk_pmod_table(c, g.key_level, g.special_start, g.nspecial, &t.pmod));
    return grow_ws(c, ws_words * 8);
}

int ks_reserve(mfhe_ctx* c, size_t npoly, const KsGeom& g, int alpha, const char* what) {
    RC(ks_check_ctx(c));
    RC(ks_check_digits(c, alpha, g, what));
    KsTables t;
    return ks_prepare(c, g, alpha, 0, ks_ws_words(npoly, ks_beta(g.level, alpha), (size_t)g.rows(), c->N), t);
}

// ---- the pipeline ----
int raise_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, uint64_t* raised, size_t digit_stride,
               size_t poly_stride, size_t npoly, const KsGeom& g, int alpha, const KsTables& t, uint64_t* scratch,
               hipStream_t st) {
    for (int j = 0; j < t.beta; ++j) {
        const int ds = j * alpha, dc = g.level - ds < alpha ? g.level - ds : alpha;
        RC(ntt_modup_body(c, d_in, in_stride, raised + (size_t)j * digit_stride, poly_stride, npoly, ds, dc, t.plan[j],
                          &t.tab[(size_t)3 * j], scratch, st));
    }
    return MFHE_OK;
}

int ks_raise_ws(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, size_t npoly, const KsGeom& g, int alpha,
                const KsTables& t, hipStream_t st) {
    const size_t pw = (size_t)g.rows() * c->N;
    const KsWs w = ks_ws(npoly, t.beta, (size_t)g.rows(), c->N);
    uint64_t* ws = (uint64_t*)c->ws;
    return raise_body(c, d_in, in_stride, ws + w.raised, npoly * pw, pw, npoly, g, alpha, t, ws + w.scratch, st);
}

int ks_inner_product(mfhe_ctx* c, const KsRaised& x, const uint64_t* d_ksk, uint64_t* d_acc, size_t acc_stride,
                     size_t npoly, int ndigits, const KsGeom& g, uint32_t galois_elt, hipStream_t st) {
    KsipArgs a{};
    a.raised = x.p; a.ksk = d_ksk; a.acc = d_acc;
    a.digit_stride = x.digit_stride; a.poly_stride = x.poly_stride; a.acc_stride = acc_stride;
    a.ncoeff = c->N; a.npoly = npoly; a.ndigits = ndigits; a.g = g; a.galois_elt = galois_elt;
    return launch_ksk_inner_product(c, a, st);
}

int ks_moddown_pair(mfhe_ctx* c, const uint64_t* acc, uint64_t* scratch, const KsOut& o, size_t npoly, const KsGeom& g,
                    const KsTables& t, hipStream_t st) {
    const size_t pw = (size_t)g.rows() * c->N, lw = (size_t)g.level * c->N;
    const uint64_t* cen = nullptr;
    RC(ntt_moddown_center(c, acc, pw, 2 * npoly, g.level, g.special_start, g.nspecial, t.down, scratch, &cen, st));
    uint64_t* outs[2] = {o.out0, o.out1};
    for (int k = 0; k < 2; ++k)
        RC(launch_sub_scale(c, acc + (size_t)k * pw, 2 * pw, cen + (size_t)k * lw, 2 * lw, outs[k], o.stride,
                            (o.add >> k & 1) ? outs[k] : nullptr, npoly, g.level, g.nspecial, t.down, st));
    return MFHE_OK;
}

int ks_apply_raised(mfhe_ctx* c, const KsRaised& x, const uint64_t* d_ksk, const KsOut& o, size_t npoly,
                    const KsGeom& g, const KsTables& t, uint32_t galois_elt, hipStream_t st) {
    const size_t pw = (size_t)g.rows() * c->N;
    const KsWs w = ks_ws(npoly, t.beta, (size_t)g.rows(), c->N);
    uint64_t* ws = (uint64_t*)c->ws;
    RC(ks_inner_product(c, x, d_ksk, ws + w.acc, 2 * pw, npoly, t.beta, g, galois_elt, st));
    return ks_moddown_pair(c, ws + w.acc, ws + w.scratch, o, npoly, g, t, st);
}

int ks_switch_body(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, const uint64_t* d_ksk, const KsOut& o,
                   size_t npoly, const KsGeom& g, int alpha, const KsTables& t, hipStream_t st) {
    RC(ks_raise_ws(c, d_in, in_stride, npoly, g, alpha, t, st));
    return ks_apply_raised(c, ks_ws_raised(c, npoly, g), d_ksk, o, npoly, g, t, 0, st);
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_ksk_assemble(mfhe_ctx* c, const uint64_t* d_s_from, const uint64_t* d_s_to, const uint64_t* d_a,
                                 const uint64_t* d_e, uint64_t* d_ksk, int key_level, int alpha, int special_start,
                                 int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_s_from || !d_s_to || !d_a || !d_e || !d_ksk) return set_error(MFHE_EINVAL, "ksk_assemble: null pointer");
    const KsGeom g{key_level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "ksk_assemble"));
    const uint64_t* pmod = nullptr;
    RC(ksk_pmod_table(c, key_level, special_start, nspecial, &pmod));
    const uint64_t total = (uint64_t)ks_beta(key_level, alpha) * g.key_rows() * c->N;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) return set_error(MFHE_EINVAL, "ksk_assemble: too many coefficients for one launch");
    hipLaunchKernelGGL(ksk_assemble_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)s, d_s_from, d_s_to, d_a,
                       d_e, d_ksk, key_level, g.key_rows(), alpha, special_start, c->logN, pmod,
                       (const uint64_t*)c->d_dmod, total);
    MFHE_CHECK_LAUNCH("ksk_assemble_kernel");
    return MFHE_OK;
}

// galois_elt 0: the plain product; else the raised digits are gathered through pi_g
static int ksk_inner_product_checked(mfhe_ctx* c, const uint64_t* d_raised, size_t digit_stride, size_t poly_stride,
                                     const uint64_t* d_ksk, uint64_t* d_acc, size_t acc_poly_stride, size_t npoly,
                                     int ndigits, int level, int key_level, int special_start, int nspecial,
                                     uint32_t galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_raised || !d_ksk || !d_acc) return set_error(MFHE_EINVAL, "ksk_inner_product: null pointer");
    if (ndigits < 1) return set_error(MFHE_EINVAL, "ksk_inner_product: ndigits < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_geom(c, g, "ksk_inner_product"));
    const size_t N = c->N, rows = (size_t)g.rows();
    if (poly_stride / N < rows || acc_poly_stride / N < 2 * rows)
        return set_error(MFHE_EINVAL, "ksk_inner_product: poly stride smaller than rows * N");
    if (npoly && digit_stride < ks_span(npoly, poly_stride, rows * N))
        return set_error(MFHE_EINVAL, "ksk_inner_product: digit stride smaller than the polynomials of a digit");
    return ks_inner_product(c, {d_raised, digit_stride, poly_stride}, d_ksk, d_acc, acc_poly_stride, npoly, ndigits, g,
                            galois_elt, (hipStream_t)s);
}

extern "C" int mfhe_ksk_inner_product(mfhe_ctx* c, const uint64_t* d_raised, size_t digit_stride, size_t poly_stride,
                                      const uint64_t* d_ksk, uint64_t* d_acc, size_t acc_poly_stride, size_t npoly,
                                      int ndigits, int level, int key_level, int special_start, int nspecial,
                                      mfhe_stream_t s) {
    return ksk_inner_product_checked(c, d_raised, digit_stride, poly_stride, d_ksk, d_acc, acc_poly_stride, npoly,
                                     ndigits, level, key_level, special_start, nspecial, 0, s);
}

extern "C" int mfhe_ksk_inner_product_galois(mfhe_ctx* c, const uint64_t* d_raised, size_t digit_stride,
                                             size_t poly_stride, const uint64_t* d_ksk, uint64_t* d_acc,
                                             size_t acc_poly_stride, size_t npoly, int ndigits, int level,
                                             int key_level, int special_start, int nspecial, int galois_elt,
                                             mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    RC(ks_check_galois(c, galois_elt, "ksk_inner_product_galois"));
    return ksk_inner_product_checked(c, d_raised, digit_stride, poly_stride, d_ksk, d_acc, acc_poly_stride, npoly,
                                     ndigits, level, key_level, special_start, nspecial, (uint32_t)galois_elt, s);
}

extern "C" int mfhe_keyswitch_reserve(mfhe_ctx* c, size_t npoly, int level, int key_level, int alpha,
                                      int special_start, int nspecial) {
    return ks_reserve(c, npoly, {level, key_level, special_start, nspecial}, alpha, "keyswitch_reserve");
}

extern "C" int mfhe_keyswitch(mfhe_ctx* c, const uint64_t* d_in, size_t in_stride, const uint64_t* d_ksk,
                              uint64_t* d_out0, uint64_t* d_out1, size_t out_stride, size_t npoly, int level,
                              int key_level, int alpha, int special_start, int nspecial, int flags, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_in || !d_ksk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "keyswitch: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "keyswitch"));
    if (flags & ~MFHE_KS_ADD) return set_error(MFHE_EINVAL, "keyswitch: unknown flag");
    const size_t N = c->N, lw = (size_t)level * N;
    if (in_stride < lw || out_stride < lw) return set_error(MFHE_EINVAL, "keyswitch: poly stride smaller than level * N");
    const size_t isp = ks_span(npoly, in_stride, lw), osp = ks_span(npoly, out_stride, lw);
    RC(ks_check_overlap("keyswitch", {{d_in, isp}}, {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    // every table and the workspace before the first launch (nothing to do after mfhe_keyswitch_reserve)
    KsTables t;
    RC(ks_prepare(c, g, alpha, 0, ks_ws_words(npoly, ks_beta(level, alpha), (size_t)g.rows(), N), t));
    const KsOut out{d_out0, d_out1, out_stride, (flags & MFHE_KS_ADD) ? 3 : 0};
    return ks_switch_body(c, d_in, in_stride, d_ksk, out, npoly, g, alpha, t, (hipStream_t)s);
}

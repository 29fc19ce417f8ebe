// lintrans.hip -- encrypted linear transforms for gfx950: a plaintext matrix applied to an encrypted vector by
// baby-step giant-step over hoisted rotations (include/mfhe.h mfhe_lt_baby_step, mfhe_lt_pt_mac, mfhe_lt_apply,
// mfhe_lt_reserve).
//
// Everything is in the evaluation domain (phantom NTT) and canonical, on the geometry of keyswitch.hip: a
// (level + K)-row block has modulus limb r on row r < level, else limb special_start + r - level.
//
//   baby step : a rotated ciphertext left in Q u P and scaled by P,
//               u[p][c][r][i] = sum_j raised[j][p][r][pi_g(i)] gk[j][c][keyrow(r)][i] + [c == 0, r < level] (P mod q_r)
//               c0[p][r][pi_g(i)]: the gathered inner product of keyswitch.hip straight into u, then lt_c0_kernel adds
//               the c0 term.  No ModDown: u0 + u1 s = P sigma_g(c0 + c1 s) + small.
//   pt_mac    : acc[p][c][r] = sum_t pt[term_pt[t]][ptrow(r)] u[term_u[t]][p][c][r] mod q_r, one launch
//   apply     : raise c1 once, every baby step, then per giant step one pt_mac, one ModDown of both components and one
//               rotation (raise, gathered inner product, ModDown); the additions into `out` ride in ModDown's tail and
//               in lt_c0_kernel (its multiplier-1 form is an accumulating automorphism)
//
// pt_mac design, as the inner product of keyswitch.hip: one thread owns one (row, coefficient) -- two adjacent
// coefficients with 16-byte accesses when the layout allows -- loads its slice of every plaintext of the sum once
// (nterms <= kLtUnroll; longer sums re-read it per output, from the cache) and walks a run of (polynomial, component)
// pairs.  The sum is an unreduced u128 (16 products of canonical residues below 2^62 fit; longer sums fold every 16
// terms) and ends in one 128-bit Barrett reduction.  The row is the grid's y index, so the modulus constants are scalar
// loads; the term index arrays are kernel arguments, so nothing is copied to the device.
#include "lintrans.hpp"

#include <hip/hip_runtime.h>

#include "bconv.hpp"
#include "galois.hpp"
#include "mod128.hpp"

namespace mfhe {

// largest term count whose plaintext slices stay in registers (DESIGN.md §3.11 has the resource table behind it)
constexpr int kLtUnroll = 8;
// Shortest run of (polynomial, component) pairs one thread walks with its plaintext slices (the whole batch when it is
// smaller): two polynomials.  The slices cost nterms loads against nterms + 1 accesses per pair, and they are shared by
// every polynomial of the batch, so a re-read is a cache hit; a short minimum keeps small batches on many workgroups.
constexpr uint64_t kLtMinRun = 4;

// NT: terms (template-unrolled, the plaintext slices in registers) or 0 (generic loop over a.nterms); V: coefficients
// per thread.  dmod is indexed by the block's row: scalar loads, as are the term indices (kernel arguments).
template <int NT, int V>
__global__ __launch_bounds__(256) void lt_pt_mac_kernel(LtMacArgs a, const uint64_t* __restrict__ dmod) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= a.ncoeff) return;
    const int r = blockIdx.y;
    const int level = a.level, rows = level + a.nspecial;
    const int limb = r < level ? r : a.special_start + r - level;
    const int prow = r < level ? r : a.pt_level + r - level;
    const uint64_t q = dmod[3 * limb], r0 = dmod[3 * limb + 1], r1 = dmod[3 * limb + 2];
    const T* pp = (const T*)a.pt + (uint64_t)prow * a.ncoeff + c;
    const T* up = (const T*)a.u + (uint64_t)r * a.ncoeff + c;
    T* op = (T*)a.acc + (uint64_t)r * a.ncoeff + c;
    const uint64_t cstride = (uint64_t)rows * a.ncoeff;   // one component
    const uint64_t pc0 = blockIdx.z * a.prun;
    const uint64_t pc1 = pc0 + a.prun < a.npairs ? pc0 + a.prun : a.npairs;

    if (NT) {
        constexpr int NK = NT ? NT : 1;
        uint64_t w[NK][V];
#pragma unroll
        for (int t = 0; t < NK; ++t) Lane<V>::load(pp + (uint64_t)a.term_pt[t] * a.pt_stride, w[t]);
        for (uint64_t pc = pc0; pc < pc1; ++pc) {
            const uint64_t p = pc >> 1, off = (pc & 1) * cstride;
            uint64_t x[NK][V];
#pragma unroll
            for (int t = 0; t < NK; ++t)
                Lane<V>::load(up + (uint64_t)a.term_u[t] * a.slot_stride + p * a.poly_stride + off, x[t]);
            u128 s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = 0;
#pragma unroll
            for (int t = 0; t < NK; ++t)
#pragma unroll
                for (int k = 0; k < V; ++k) s[k] += (u128)x[t][k] * w[t][k];
            uint64_t o[V];
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = barrett128(s[k], q, r0, r1);
            Lane<V>::store(op + p * a.acc_stride + off, o);
        }
    } else {
        for (uint64_t pc = pc0; pc < pc1; ++pc) {
            const uint64_t p = pc >> 1, off = (pc & 1) * cstride;
            uint64_t o[V];
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = 0;
            for (int t0 = 0; t0 < a.nterms; t0 += 16) {   // 16 products < 2^124 and a residue < 2^62 fit a u128
                u128 s[V];
#pragma unroll
                for (int k = 0; k < V; ++k) s[k] = o[k];
                const int t1 = t0 + 16 < a.nterms ? t0 + 16 : a.nterms;
                for (int t = t0; t < t1; ++t) {
                    uint64_t x[V], w[V];
                    Lane<V>::load(up + (uint64_t)a.term_u[t] * a.slot_stride + p * a.poly_stride + off, x);
                    Lane<V>::load(pp + (uint64_t)a.term_pt[t] * a.pt_stride, w);
#pragma unroll
                    for (int k = 0; k < V; ++k) s[k] += (u128)x[k] * w[k];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = barrett128(s[k], q, r0, r1);
            }
            Lane<V>::store(op + p * a.acc_stride + off, o);
        }
    }
}

// One thread per element (V words) of row blockIdx.y, walking the polynomials blockIdx.z, blockIdx.z + gridDim.z, ...
// Rows r < level: x = src[p][r][pi_g(i)] (no gather for galois_elt <= 1), m = pmod[r] (1 when pmod is null);
// ADD: u[p][r][i] = (m x + u[p][r][i]) mod q_r, else u[p][r][i] = m x mod q_r.  Rows r >= level (the store form
// alone is launched over them): u[p][r][i] = 0.  q and its constants are scalar loads per row; limb r is row r here.
template <int V, bool ADD>
__global__ __launch_bounds__(256) void lt_c0_kernel(const void* __restrict__ src, void* u, uint64_t src_stride,
                                                    uint64_t u_stride, uint64_t ncoeff, uint64_t npoly, int level,
                                                    const uint64_t* __restrict__ pmod,
                                                    const uint64_t* __restrict__ dmod, uint32_t galois_elt, int log_n) {
    using T = typename Lane<V>::T;
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c >= ncoeff) return;
    const int r = blockIdx.y;
    T* up = (T*)u + (uint64_t)r * ncoeff + c;
    if (r >= level) {
        const uint64_t zero[V] = {};
        for (uint64_t p = blockIdx.z; p < npoly; p += gridDim.z) Lane<V>::store(up + p * u_stride, zero);
        return;
    }
    uint64_t cs = c;
    bool swap = false;
    if (galois_elt > 1u) {
        const uint32_t s = galois_perm_index((uint32_t)c * V, galois_elt, log_n);
        cs = V == 2 ? s >> 1 : s;
        swap = V == 2 && (s & 1u);
    }
    const uint64_t q = dmod[3 * r], r0 = dmod[3 * r + 1], r1 = dmod[3 * r + 2];
    const uint64_t m = pmod ? pmod[r] : 1;
    const T* sp = (const T*)src + (uint64_t)r * ncoeff + cs;
    for (uint64_t p = blockIdx.z; p < npoly; p += gridDim.z) {
        uint64_t x[V], o[V];
        Lane<V>::load(sp + p * src_stride, x);
        if (V == 2 && swap) {
            const uint64_t t = x[0];
            x[0] = x[V - 1];
            x[V - 1] = t;
        }
        if (ADD) Lane<V>::load(up + p * u_stride, o);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = barrett128((u128)m * x[k] + (ADD ? o[k] : 0), q, r0, r1);
        Lane<V>::store(up + p * u_stride, o);
    }
}

using LtMacKernel = void (*)(LtMacArgs, const uint64_t*);

template <int V>
static LtMacKernel pick_lt_mac(int nt) {
    switch (nt) {
        case 1: return lt_pt_mac_kernel<1, V>;
        case 2: return lt_pt_mac_kernel<2, V>;
        case 3: return lt_pt_mac_kernel<3, V>;
        case 4: return lt_pt_mac_kernel<4, V>;
        case 5: return lt_pt_mac_kernel<5, V>;
        case 6: return lt_pt_mac_kernel<6, V>;
        case 7: return lt_pt_mac_kernel<7, V>;
        case 8: return lt_pt_mac_kernel<8, V>;
        default: return lt_pt_mac_kernel<0, V>;
    }
}
static_assert(kLtUnroll == 8, "pick_lt_mac lists the unrolled term counts");

int launch_lt_pt_mac(mfhe_ctx* c, LtMacArgs a, size_t npoly, hipStream_t st) {
    if (npoly == 0 || a.ncoeff == 0) return MFHE_OK;
    const bool wide = ks_wide({&a.ncoeff, &a.slot_stride, &a.poly_stride, &a.pt_stride, &a.acc_stride},
                              {a.u, a.pt, a.acc});
    const KsRowGrid rg = ks_row_grid(a.ncoeff);
    const uint64_t rows = (uint64_t)(a.level + a.nspecial);
    if (rg.bx > 0x7fffffffull || rows > 65535) return set_error(MFHE_EINVAL, "lt_pt_mac: too large for one launch");
    a.npairs = 2 * (uint64_t)npoly;
    const KsRuns run = ks_runs(a.npairs, rg.bx, rows, kLtMinRun);   // a thread keeps its plaintext slices across a run
    a.prun = run.prun;
    const LtMacKernel k = wide ? pick_lt_mac<2>(a.nterms) : pick_lt_mac<1>(a.nterms);
    hipLaunchKernelGGL(k, dim3((uint32_t)rg.bx, (uint32_t)rows, (uint32_t)run.runs), dim3(rg.block), 0, st, a,
                       (const uint64_t*)c->d_dmod);
    MFHE_CHECK_LAUNCH("lt_pt_mac_kernel");
    return MFHE_OK;
}

int launch_lt_c0(mfhe_ctx* c, const uint64_t* src, size_t src_stride, uint64_t* u, size_t u_stride, size_t npoly,
                 int level, int nrows, const uint64_t* pmod, uint32_t galois_elt, bool add, hipStream_t st) {
    uint64_t ncoeff = c->N;
    if (npoly == 0 || nrows == 0) return MFHE_OK;
    const bool wide = ks_wide({&ncoeff, &src_stride, &u_stride}, {src, u});
    const KsRowGrid rg = ks_row_grid(ncoeff);
    if (rg.bx > 0x7fffffffull || nrows > 65535) return set_error(MFHE_EINVAL, "lt_baby_step: too large for one launch");
    const dim3 grid((uint32_t)rg.bx, (uint32_t)nrows, (uint32_t)(npoly < 65535 ? npoly : 65535));
    auto k = wide ? (add ? lt_c0_kernel<2, true> : lt_c0_kernel<2, false>)
                  : (add ? lt_c0_kernel<1, true> : lt_c0_kernel<1, false>);
    hipLaunchKernelGGL(k, grid, dim3(rg.block), 0, st, (const void*)src, (void*)u, (uint64_t)src_stride,
                       (uint64_t)u_stride, ncoeff, (uint64_t)npoly, level, pmod, (const uint64_t*)c->d_dmod, galois_elt,
                       c->logN);
    MFHE_CHECK_LAUNCH("lt_c0_kernel");
    return MFHE_OK;
}

// words of mfhe_lt_apply's block of the workspace: the key switch's block, n_baby baby slots and one accumulator of
// [npoly][2][rows][N] each, and (w0, w1) of [npoly][level][N] each
static size_t lt_ws_words(size_t npoly, int beta, size_t rows, int level, size_t N, int n_baby) {
    return ks_ws_words(npoly, beta, rows, N) + (2 * (size_t)n_baby + 2) * npoly * rows * N + 2 * npoly * (size_t)level * N;
}

// The baby step of d_u (arguments checked, tables built): with a key, the gathered inner product into u and the c0
// term added; without (g = 1), u = (P c0, P c1) on the Q rows and 0 on the special rows, x1 = c1.
static int baby_body(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const KsRaised& x1, const uint64_t* d_gk,
                     uint64_t* d_u, size_t u_stride, size_t npoly, const KsGeom& g, int beta, const uint64_t* pmod,
                     uint32_t galois_elt, hipStream_t st) {
    const size_t pw = (size_t)g.rows() * c->N;
    if (!d_gk) {
        RC(launch_lt_c0(c, d_c0, in_stride, d_u, u_stride, npoly, g.level, g.rows(), pmod, 0, false, st));
        return launch_lt_c0(c, x1.p, in_stride, d_u + pw, u_stride, npoly, g.level, g.rows(), pmod, 0, false, st);
    }
    RC(ks_inner_product(c, x1, d_gk, d_u, u_stride, npoly, beta, g, galois_elt, st));
    return launch_lt_c0(c, d_c0, in_stride, d_u, u_stride, npoly, g.level, g.level, pmod, galois_elt, true, st);
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_lt_baby_step(mfhe_ctx* c, const uint64_t* d_c0, size_t in_stride, const uint64_t* d_raised,
                                 size_t digit_stride, size_t poly_stride, const uint64_t* d_gk, uint64_t* d_u,
                                 size_t u_stride, size_t npoly, int level, int key_level, int alpha, int special_start,
                                 int nspecial, int galois_elt, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_raised || !d_u) return set_error(MFHE_EINVAL, "lt_baby_step: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "lt_baby_step"));
    RC(ks_check_galois(c, galois_elt, "lt_baby_step"));
    if (!d_gk && galois_elt != 1) return set_error(MFHE_EINVAL, "lt_baby_step: null key for a Galois element other than 1");
    const size_t N = c->N, pw = (size_t)g.rows() * N, lw = (size_t)level * N;
    const int beta = ks_beta(level, alpha);
    if (in_stride < lw) return set_error(MFHE_EINVAL, "lt_baby_step: input poly stride smaller than level * N");
    if (u_stride / N < 2 * (size_t)g.rows()) return set_error(MFHE_EINVAL, "lt_baby_step: u poly stride smaller than 2 rows * N");
    const size_t isp = ks_span(npoly, in_stride, lw), usp = ks_span(npoly, u_stride, 2 * pw);
    size_t rsp = isp;   // without a key d_raised is c1, laid out as c0
    if (d_gk) {
        if (poly_stride < pw) return set_error(MFHE_EINVAL, "lt_baby_step: raised poly stride smaller than rows * N");
        const size_t dsp = ks_span(npoly, poly_stride, pw);
        if (npoly && digit_stride < dsp)
            return set_error(MFHE_EINVAL, "lt_baby_step: digit stride smaller than the polynomials of a digit");
        rsp = ks_span(beta, digit_stride, dsp);
    }
    RC(ks_check_overlap("lt_baby_step",
                        {{d_c0, isp}, {d_raised, rsp}, {d_gk, d_gk ? (size_t)beta * 2 * g.key_rows() * N : 0}},
                        {{d_u, usp}}));
    if (npoly == 0) return MFHE_OK;
    const uint64_t* pmod = nullptr;
    RC(ksk_pmod_table(c, key_level, special_start, nspecial, &pmod));
    return baby_body(c, d_c0, in_stride, {d_raised, digit_stride, poly_stride}, d_gk, d_u, u_stride, npoly, g, beta,
                     pmod, (uint32_t)galois_elt, (hipStream_t)s);
}

extern "C" int mfhe_lt_pt_mac(mfhe_ctx* c, const uint64_t* d_u, size_t slot_stride, size_t poly_stride, int nslots,
                              const uint64_t* d_pt, size_t pt_stride, int npt, int pt_level, uint64_t* d_acc,
                              size_t acc_stride, const int* term_u, const int* term_pt, int nterms, size_t npoly,
                              int level, int special_start, int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_u || !d_pt || !d_acc || !term_u || !term_pt) return set_error(MFHE_EINVAL, "lt_pt_mac: null pointer");
    if (nterms < 1 || nterms > kLtMaxTerms) return set_error(MFHE_EINVAL, "lt_pt_mac: nterms outside [1, 64]");
    if (nslots < 1 || npt < 1) return set_error(MFHE_EINVAL, "lt_pt_mac: nslots or npt < 1");
    if (pt_level < level) return set_error(MFHE_EINVAL, "lt_pt_mac: pt_level < level");
    const KsGeom g{level, pt_level, special_start, nspecial};   // a plaintext is laid out as a key made at pt_level
    RC(ks_check_geom(c, g, "lt_pt_mac"));
    for (int t = 0; t < nterms; ++t)
        if (term_u[t] < 0 || term_u[t] >= nslots || term_pt[t] < 0 || term_pt[t] >= npt)
            return set_error(MFHE_EINVAL, "lt_pt_mac: a term index is out of range");
    const size_t N = c->N, pw = (size_t)g.rows() * N, ptw = (size_t)g.key_rows() * N;
    if (poly_stride / N < 2 * (size_t)g.rows() || acc_stride / N < 2 * (size_t)g.rows())
        return set_error(MFHE_EINVAL, "lt_pt_mac: poly stride smaller than 2 rows * N");
    const size_t ssp = ks_span(npoly, poly_stride, 2 * pw);
    if (npoly && slot_stride < ssp) return set_error(MFHE_EINVAL, "lt_pt_mac: slot stride smaller than the polynomials of a slot");
    if (pt_stride < ptw) return set_error(MFHE_EINVAL, "lt_pt_mac: pt stride smaller than (pt_level + K) * N");
    const size_t asp = ks_span(npoly, acc_stride, 2 * pw);
    RC(ks_check_overlap("lt_pt_mac", {{d_u, ks_span(nslots, slot_stride, ssp)}, {d_pt, ks_span(npt, pt_stride, ptw)}},
                        {{d_acc, asp}}));
    LtMacArgs a{};
    a.u = d_u; a.pt = d_pt; a.acc = d_acc;
    a.slot_stride = slot_stride; a.poly_stride = poly_stride; a.pt_stride = pt_stride; a.acc_stride = acc_stride;
    a.ncoeff = N; a.nterms = nterms; a.level = level; a.pt_level = pt_level; a.special_start = special_start;
    a.nspecial = nspecial;
    for (int t = 0; t < nterms; ++t) {
        a.term_u[t] = term_u[t];
        a.term_pt[t] = term_pt[t];
    }
    return launch_lt_pt_mac(c, a, npoly, (hipStream_t)s);
}

extern "C" int mfhe_lt_reserve(mfhe_ctx* c, size_t npoly, int level, int key_level, int alpha, int special_start,
                               int nspecial, int n_baby) {
    RC(ks_check_ctx(c));
    if (alpha < 1) return set_error(MFHE_EINVAL, "lt_reserve: alpha < 1");
    if (n_baby < 1) return set_error(MFHE_EINVAL, "lt_reserve: n_baby < 1");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_geom(c, g, "lt_reserve"));
    KsTables t;
    return ks_prepare(c, g, alpha, kKsPmod,
                      lt_ws_words(npoly, ks_beta(level, alpha), (size_t)g.rows(), level, c->N, n_baby), t);
}

extern "C" int mfhe_lt_apply(mfhe_ctx* c, const mfhe_lt_plan* plan, const uint64_t* d_c0, const uint64_t* d_c1,
                             size_t in_stride, const uint64_t* d_pt, size_t pt_stride, int pt_level, uint64_t* d_out0,
                             uint64_t* d_out1, size_t out_stride, size_t npoly, int level, int key_level, int alpha,
                             int special_start, int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!plan || !d_c0 || !d_c1 || !d_pt || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "lt_apply: null pointer");
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "lt_apply"));
    if (pt_level < level) return set_error(MFHE_EINVAL, "lt_apply: pt_level < level");
    RC(ks_check_geom(c, KsGeom{level, pt_level, special_start, nspecial}, "lt_apply (plaintexts)"));
    std::vector<LtGroup> groups;
    std::vector<char> baby_used;
    if (const int e = lt_plan_validate(plan, c->N, groups, baby_used))
        return set_error(MFHE_EINVAL, std::string("lt_apply: ") + lt_plan_error_text(e));
    const size_t N = c->N, rows = (size_t)g.rows(), pw = rows * N, lw = (size_t)level * N;
    const size_t ptw = ((size_t)pt_level + nspecial) * N, kw = 2 * (size_t)g.key_rows() * N;
    const int beta = ks_beta(level, alpha);
    if (in_stride < lw || out_stride < lw) return set_error(MFHE_EINVAL, "lt_apply: poly stride smaller than level * N");
    if (pt_stride < ptw) return set_error(MFHE_EINVAL, "lt_apply: pt stride smaller than (pt_level + K) * N");
    const size_t isp = ks_span(npoly, in_stride, lw), osp = ks_span(npoly, out_stride, lw);
    std::vector<KsRange> in{{d_c0, isp}, {d_c1, isp}, {d_pt, ks_span(plan->nterms, pt_stride, ptw)}};
    for (int b = 1; b < plan->n_baby; ++b)   // and every key that is read
        if (baby_used[b]) in.push_back({plan->d_gk_baby[b], beta * kw});
    for (const LtGroup& gr : groups)
        if (gr.giant) in.push_back({plan->d_gk_giant[gr.giant], beta * kw});
    const KsRange out[2] = {{d_out0, osp}, {d_out1, osp}};
    RC(ks_check_overlap("lt_apply", in.data(), in.size(), out, 2));
    if (npoly == 0) return MFHE_OK;
    // every table and the workspace before the first launch (nothing to do after mfhe_lt_reserve)
    KsTables t;
    RC(ks_prepare(c, g, alpha, kKsPmod, lt_ws_words(npoly, beta, rows, level, N, plan->n_baby), t));
    hipStream_t st = (hipStream_t)s;
    const KsWs w = ks_ws(npoly, beta, rows, N);                // the key switch's block, then
    const KsRaised raised = ks_ws_raised(c, npoly, g);
    uint64_t* scratch = (uint64_t*)c->ws + w.scratch;
    uint64_t* U = (uint64_t*)c->ws + w.end;                    // [n_baby][npoly][2][rows][N]
    uint64_t* A = U + (size_t)plan->n_baby * 2 * npoly * pw;   // [npoly][2][rows][N]
    uint64_t* w0 = A + 2 * npoly * pw;                         // [npoly][level][N]
    uint64_t* w1 = w0 + npoly * lw;                            // [npoly][level][N]
    const size_t slot = 2 * npoly * pw;

    bool keyed = false;
    for (int b = 1; b < plan->n_baby; ++b) keyed = keyed || baby_used[b];
    if (keyed) RC(ks_raise_ws(c, d_c1, in_stride, npoly, g, alpha, t, st));
    for (int b = 0; b < plan->n_baby; ++b) {
        if (!baby_used[b]) continue;
        if (b == 0)
            RC(baby_body(c, d_c0, in_stride, {d_c1, 0, 0}, nullptr, U, 2 * pw, npoly, g, beta, t.pmod, 1, st));
        else
            RC(baby_body(c, d_c0, in_stride, raised, plan->d_gk_baby[b], U + (size_t)b * slot, 2 * pw, npoly, g, beta,
                         t.pmod, (uint32_t)plan->baby_elt[b], st));
    }
    bool started = false;   // `out` holds a partial sum
    for (const LtGroup& gr : groups) {
        LtMacArgs m{};
        m.u = U; m.pt = d_pt; m.acc = A;
        m.slot_stride = slot; m.poly_stride = 2 * pw; m.pt_stride = pt_stride; m.acc_stride = 2 * pw;
        m.ncoeff = N; m.nterms = gr.count; m.level = level; m.pt_level = pt_level; m.special_start = special_start;
        m.nspecial = nspecial;
        for (int k = 0; k < gr.count; ++k) {
            m.term_u[k] = plan->term_baby[gr.first + k];
            m.term_pt[k] = gr.first + k;
        }
        RC(launch_lt_pt_mac(c, m, npoly, st));
        if (gr.giant == 0) {
            RC(ks_moddown_pair(c, A, scratch, {d_out0, d_out1, out_stride, started ? 3 : 0}, npoly, g, t, st));
            started = true;
            continue;
        }
        RC(ks_moddown_pair(c, A, scratch, {w0, w1, lw, 0}, npoly, g, t, st));
        // the rotation of (w0, w1), added into out: out0 (+)= sigma(w0), then the key switch of sigma(w1) with out as
        // the addend of ModDown's tails
        const uint32_t ge = (uint32_t)plan->giant_elt[gr.giant];
        RC(ks_raise_ws(c, w1, lw, npoly, g, alpha, t, st));
        if (started)
            RC(launch_lt_c0(c, w0, lw, d_out0, out_stride, npoly, level, level, nullptr, ge, true, st));
        else
            RC(launch_automorphism(c, w0, lw, d_out0, out_stride, npoly, level, ge, st));
        RC(ks_apply_raised(c, raised, plan->d_gk_giant[gr.giant], {d_out0, d_out1, out_stride, started ? 3 : 1}, npoly,
                           g, t, ge, st));
        started = true;
    }
    return MFHE_OK;
}

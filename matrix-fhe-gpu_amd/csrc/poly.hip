// poly.hip -- encrypted polynomial evaluation for gfx950: the plan object around poly_plan.hpp and the driver that
// runs its nodes (include/mfhe.h mfhe_poly_plan_*, mfhe_poly_reserve, mfhe_poly_apply).
//
// A node is a ciphertext product (ctmul.hip: tensor sum and relinearisation, not rescaled) into t, one scalar sum
// (lincomb.hip) of t and registers into reg[dst], and the rescale of reg[dst] in place (ctmul.hip's); the last node's
// rescale writes the caller's outputs instead.  Registers and t live behind the product's block of the workspace as
// slots [2][npoly][level][N] at one stride, so a slot is a source of the sum by its index, both components of a slot
// are one batch of the rescale, and a register at a lower level is the first rows of its slot.
#include <hip/hip_runtime.h>

#include <map>

#include "ctmul.hpp"
#include "lincomb.hpp"
#include "poly_plan.hpp"

struct mfhe_poly_plan {
    mfhe::PolyPlan p;
    std::vector<uint64_t> ctx_moduli;   // every modulus of the context the plan was made for
    uint64_t* d_k = nullptr;            // [nconst][level]
};

namespace mfhe {

static size_t poly_ctmul_words(size_t npoly, int level, int alpha, int nspecial, size_t N) {
    return ks_ws_words(npoly, ks_beta(level, alpha), (size_t)(level + nspecial), N) + npoly * (size_t)level * N;
}
// words of mfhe_poly_apply's block of the workspace
static size_t poly_ws_words(const PolyPlan& p, size_t npoly, int alpha, int nspecial, size_t N) {
    return poly_ctmul_words(npoly, p.level, alpha, nspecial, N) + 2 * ((size_t)p.nreg + 1) * npoly * (size_t)p.level * N;
}

static int poly_check_plan(const mfhe_ctx* c, const mfhe_poly_plan* plan, const char* what) {
    if (!plan) return set_error(MFHE_EINVAL, std::string(what) + ": null plan");
    if (plan->ctx_moduli != c->moduli)
        return set_error(MFHE_EINVAL, std::string(what) + ": the plan was made for a context of other moduli");
    return MFHE_OK;
}

// every table of every level the plan's nodes run at, and the workspace
static int poly_prepare(mfhe_ctx* c, const PolyPlan& p, size_t npoly, const KsGeom& g, int alpha,
                        std::map<int, KsTables>& tabs) {
    const size_t words = poly_ws_words(p, npoly, alpha, g.nspecial, c->N);
    for (const PolyNode& n : p.nodes)
        if (!tabs.count(n.level))
            RC(ks_prepare(c, KsGeom{n.level, g.key_level, g.special_start, g.nspecial}, alpha, kKsRescale, words,
                          tabs[n.level]));
    return MFHE_OK;
}

}  // namespace mfhe

using namespace mfhe;

extern "C" int mfhe_poly_plan_create(mfhe_ctx* c, const double* coeffs, int degree, int basis, double in_scale,
                                     int level, mfhe_poly_plan** out) {
    RC(ks_check_ctx(c));
    if (!coeffs || !out) return set_error(MFHE_EINVAL, "poly_plan_create: null pointer");
    *out = nullptr;
    if (level < 1 || level > c->L) return set_error(MFHE_EINVAL, "poly_plan_create: level outside the context");
    mfhe_poly_plan* pl = new (std::nothrow) mfhe_poly_plan;
    if (!pl) return set_error(MFHE_ENOMEM, "poly_plan_create: host allocation failed");
    if (const int e = poly_plan_build(coeffs, degree, basis, in_scale, level, c->moduli.data(), pl->p)) {
        delete pl;
        return set_error(MFHE_EINVAL, std::string("poly_plan_create: ") + poly_plan_error_text(e));
    }
    pl->ctx_moduli = c->moduli;
    const std::vector<uint64_t> res = poly_plan_residues(pl->p);
    hipError_t e = hipMalloc((void**)&pl->d_k, res.size() * 8);
    if (e == hipSuccess) e = hipMemcpy(pl->d_k, res.data(), res.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (pl->d_k) (void)hipFree(pl->d_k);
        delete pl;
        return hip_error(e, "poly_plan_create: the constants' table");
    }
    *out = pl;
    return MFHE_OK;
}

extern "C" int mfhe_poly_plan_destroy(mfhe_poly_plan* plan) {
    if (!plan) return MFHE_OK;
    if (plan->d_k) (void)hipFree(plan->d_k);
    delete plan;
    return MFHE_OK;
}

extern "C" int mfhe_poly_plan_info(const mfhe_poly_plan* plan, mfhe_poly_info* info) {
    if (!plan || !info) return set_error(MFHE_EINVAL, "poly_plan_info: null pointer");
    const PolyPlan& p = plan->p;
    info->basis = p.basis; info->degree = p.degree; info->level = p.level;
    info->nnodes = (int)p.nodes.size(); info->nreg = p.nreg; info->nconst = (int)p.consts.size(); info->nmul = p.nmul;
    info->depth = p.depth; info->out_level = p.out_level; info->out_reg = p.out_reg;
    info->in_scale = p.in_scale; info->out_scale = p.out_scale;
    return MFHE_OK;
}

extern "C" int mfhe_poly_plan_node(const mfhe_poly_plan* plan, int i, mfhe_poly_node* node) {
    if (!plan || !node) return set_error(MFHE_EINVAL, "poly_plan_node: null pointer");
    if (i < 0 || i >= (int)plan->p.nodes.size()) return set_error(MFHE_EINVAL, "poly_plan_node: index out of range");
    const PolyNode& n = plan->p.nodes[(size_t)i];
    *node = mfhe_poly_node{};
    node->dst = n.dst; node->level = n.level;
    node->mul_a = n.mul_a; node->mul_b = n.mul_b; node->k_mul = n.k_mul;
    node->nterms = (int)n.src.size(); node->addend_k = n.addend_k;
    for (size_t j = 0; j < n.src.size(); ++j) {
        node->term_src[j] = n.src[j];
        node->term_k[j] = n.k[j];
        node->term_coef[j] = n.coef[j];
    }
    node->addend_coef = n.addend_coef;
    node->scale_in = n.scale_in; node->scale_out = n.scale_out;
    return MFHE_OK;
}

extern "C" int mfhe_poly_plan_constant(const mfhe_poly_plan* plan, int i, int* negative, uint64_t* mag_lo,
                                       uint64_t* mag_hi) {
    if (!plan || !negative || !mag_lo || !mag_hi) return set_error(MFHE_EINVAL, "poly_plan_constant: null pointer");
    if (i < 0 || i >= (int)plan->p.consts.size())
        return set_error(MFHE_EINVAL, "poly_plan_constant: index out of range");
    const PolyConst& k = plan->p.consts[(size_t)i];
    *negative = k.negative ? 1 : 0;
    *mag_lo = (uint64_t)k.mag;
    *mag_hi = (uint64_t)(k.mag >> 64);
    return MFHE_OK;
}

extern "C" int mfhe_poly_plan_table(const mfhe_poly_plan* plan, const uint64_t** d_k) {
    if (!plan || !d_k) return set_error(MFHE_EINVAL, "poly_plan_table: null pointer");
    *d_k = plan->d_k;
    return MFHE_OK;
}

extern "C" int mfhe_poly_reserve(mfhe_ctx* c, const mfhe_poly_plan* plan, size_t npoly, int key_level, int alpha,
                                 int special_start, int nspecial) {
    RC(ks_check_ctx(c));
    RC(poly_check_plan(c, plan, "poly_reserve"));
    const KsGeom g{plan->p.level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "poly_reserve"));
    std::map<int, KsTables> tabs;
    return poly_prepare(c, plan->p, npoly, g, alpha, tabs);
}

extern "C" int mfhe_poly_apply(mfhe_ctx* c, const mfhe_poly_plan* plan, const uint64_t* d_c0, const uint64_t* d_c1,
                               size_t in_poly_stride, const uint64_t* d_rlk, uint64_t* d_out0, uint64_t* d_out1,
                               size_t out_poly_stride, size_t npoly, int key_level, int alpha, int special_start,
                               int nspecial, mfhe_stream_t s) {
    RC(ks_check_ctx(c));
    if (!d_c0 || !d_c1 || !d_rlk || !d_out0 || !d_out1) return set_error(MFHE_EINVAL, "poly_apply: null pointer");
    RC(poly_check_plan(c, plan, "poly_apply"));
    const PolyPlan& p = plan->p;
    const int level = p.level;
    const KsGeom g{level, key_level, special_start, nspecial};
    RC(ks_check_digits(c, alpha, g, "poly_apply"));
    const size_t N = c->N, lw = (size_t)level * N, ow = (size_t)p.out_level * N;
    if (in_poly_stride < lw) return set_error(MFHE_EINVAL, "poly_apply: input poly stride smaller than level * N");
    if (out_poly_stride < ow) return set_error(MFHE_EINVAL, "poly_apply: output poly stride smaller than out_level * N");
    const size_t isp = ks_span(npoly, in_poly_stride, lw), osp = ks_span(npoly, out_poly_stride, ow);
    RC(ks_check_overlap("poly_apply",
                        {{d_c0, isp},
                         {d_c1, isp},
                         {d_rlk, (size_t)ks_beta(level, alpha) * 2 * g.key_rows() * N},
                         {plan->d_k, p.consts.size() * (size_t)level}},
                        {{d_out0, osp}, {d_out1, osp}}));
    if (npoly == 0) return MFHE_OK;
    // every table and the workspace before the first launch (nothing to do after mfhe_poly_reserve)
    std::map<int, KsTables> tabs;
    RC(poly_prepare(c, p, npoly, g, alpha, tabs));
    hipStream_t st = (hipStream_t)s;
    const size_t comp = npoly * lw, slot = 2 * comp;   // one component of a slot; a slot
    uint64_t* R = (uint64_t*)c->ws + poly_ctmul_words(npoly, level, alpha, nspecial, N);   // [nreg + 1][2][npoly][level][N]
    const int tslot = p.nreg;
    auto reg = [&](int r, int cpt) { return R + (size_t)r * slot + (size_t)cpt * comp; };

    RC(launch_copy_rows(d_c0, in_poly_stride, reg(0, 0), lw, npoly, lw, st));
    RC(launch_copy_rows(d_c1, in_poly_stride, reg(0, 1), lw, npoly, lw, st));
    for (size_t i = 0; i < p.nodes.size(); ++i) {
        const PolyNode& n = p.nodes[i];
        const KsGeom gl{n.level, key_level, special_start, nspecial};
        const KsTables& t = tabs[n.level];
        LincombArgs a{};
        if (n.mul_a >= 0) {
            // mfhe_ctmul_apply without the rescale, into t
            CtmulArgs m{};
            const bool sq = n.mul_a == n.mul_b;
            m.a0 = reg(n.mul_a, 0); m.a1 = reg(n.mul_a, 1);
            m.b0 = sq ? nullptr : reg(n.mul_b, 0); m.b1 = sq ? nullptr : reg(n.mul_b, 1);
            m.d0 = reg(tslot, 0); m.d1 = reg(tslot, 1); m.d2 = ctmul_d2(c, npoly, t.beta, gl);
            m.a_term = 0; m.a_poly = lw; m.b_term = 0; m.b_poly = sq ? 0 : lw;
            m.d01_poly = lw; m.d2_poly = (size_t)n.level * N;
            m.ncoeff = N; m.npoly = npoly; m.nterms = 1; m.level = n.level;
            RC(launch_ctmul_tensor(c, m, st));
            RC(ctmul_relin_rescale(c, d_rlk, reg(tslot, 0), reg(tslot, 1), lw, npoly, gl, alpha, t, 0, st));
            a.term_x[a.nterms] = tslot;
            a.term_k[a.nterms++] = n.k_mul;
        }
        for (size_t j = 0; j < n.src.size(); ++j) {
            a.term_x[a.nterms] = n.src[j];
            a.term_k[a.nterms++] = n.k[j];
        }
        a.x0 = reg(0, 0); a.x1 = reg(0, 1); a.k = plan->d_k; a.o0 = reg(n.dst, 0); a.o1 = reg(n.dst, 1);
        a.src_stride = slot; a.x_poly = lw; a.o_poly = lw; a.k_stride = (uint64_t)level;
        a.ncoeff = N; a.level = n.level; a.addend_k = n.addend_k;
        RC(launch_ct_lincomb(c, a, npoly, st));
        if (i + 1 < p.nodes.size()) {
            RC(ctmul_rescale(c, reg(n.dst, 0), reg(n.dst, 1), lw, npoly, gl, t, st));
            continue;
        }
        // the last rescale: the centred conversion of both components as one batch, then one tail per component into
        // the caller's outputs
        const int keep = n.level - 1;
        const size_t kw = (size_t)keep * N;
        const uint64_t* cen = nullptr;
        RC(ntt_moddown_center(c, reg(n.dst, 0), lw, 2 * npoly, keep, keep, 1, t.rescale, (uint64_t*)c->ws, &cen, st));
        RC(launch_sub_scale(c, reg(n.dst, 0), lw, cen, kw, d_out0, out_poly_stride, nullptr, npoly, keep, 1, t.rescale,
                            st));
        RC(launch_sub_scale(c, reg(n.dst, 1), lw, cen + npoly * kw, kw, d_out1, out_poly_stride, nullptr, npoly, keep, 1,
                            t.rescale, st));
    }
    return MFHE_OK;
}

// Prints the plans of the polynomial planner (csrc/poly_plan.hpp, included alone) for both bases at degrees 1, 2, 3, 4,
// 7, 8, 15, 16, 31, 63 and 127 with seeded coefficients in [-1, 1], some exactly zero, one degree-15 case whose upper
// half is zero, and the code of every rejection.  One record per line, the first word its kind, doubles as hex floats:
//   plan <id> basis degree level in_scale nnodes nreg nk nmul depth out_reg out_level out_scale
//   mod  <id> q_0 .. q_(level-1)
//   coef <id> a_0 .. a_degree
//   node <id> i dst level mul_a mul_b k_mul addend_k addend_coef scale_in scale_out nterms {src k coef}
//   const <id> i negative mag_hi mag_lo
//   res  <id> i residues mod q_0 .. q_(level-1)
//   reject <name> code
// tests/test_poly_plan_cpu.py builds this with the host compiler under the address and undefined-behaviour sanitizers
// and checks every line.  No GPU, no libmfhe.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "poly_plan.hpp"

using namespace mfhe;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double next_coef() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t v = g_state >> 11;
    if (v % 5 == 0) return 0.0;
    return (double)v / 9007199254740992.0 * 2.0 - 1.0;
}

static std::vector<uint64_t> moduli(int level) {
    // odd values near 2^45, descending: the planner reads them as numbers only
    std::vector<uint64_t> q;
    for (int r = 0; r < level; ++r) q.push_back((1ull << 45) - 2 * (uint64_t)(r * r * 977 + 3 * r) - 229);
    return q;
}

static int emit(int id, const std::vector<double>& a, int basis, double scale, int level) {
    const std::vector<uint64_t> q = moduli(level);
    PolyPlan p;
    const int rc = poly_plan_build(a.data(), (int)a.size() - 1, basis, scale, level, q.data(), p);
    if (rc) {
        std::printf("failed %d %d\n", id, rc);
        return 1;
    }
    std::printf("plan %d %d %d %d %a %zu %d %zu %d %d %d %d %a\n", id, p.basis, p.degree, p.level, p.in_scale,
                p.nodes.size(), p.nreg, p.consts.size(), p.nmul, p.depth, p.out_reg, p.out_level, p.out_scale);
    std::printf("mod %d", id);
    for (uint64_t v : q) std::printf(" %llu", (unsigned long long)v);
    std::printf("\ncoef %d", id);
    for (double v : a) std::printf(" %a", v);
    std::printf("\n");
    for (size_t i = 0; i < p.nodes.size(); ++i) {
        const PolyNode& n = p.nodes[i];
        std::printf("node %d %zu %d %d %d %d %d %d %a %a %a %zu", id, i, n.dst, n.level, n.mul_a, n.mul_b, n.k_mul,
                    n.addend_k, n.addend_coef, n.scale_in, n.scale_out, n.src.size());
        for (size_t j = 0; j < n.src.size(); ++j) std::printf(" %d %d %a", n.src[j], n.k[j], n.coef[j]);
        std::printf("\n");
    }
    const std::vector<uint64_t> res = poly_plan_residues(p);
    for (size_t i = 0; i < p.consts.size(); ++i) {
        const PolyConst& k = p.consts[i];
        std::printf("const %d %zu %d %llu %llu\n", id, i, k.negative ? 1 : 0, (unsigned long long)(k.mag >> 64),
                    (unsigned long long)k.mag);
        std::printf("res %d %zu", id, i);
        for (int r = 0; r < p.level; ++r) std::printf(" %llu", (unsigned long long)res[i * (size_t)p.level + r]);
        std::printf("\n");
    }
    return 0;
}

static void reject(const char* name, const std::vector<double>& a, int degree, int basis, double scale, int level) {
    const std::vector<uint64_t> q = moduli(level > 0 ? level : 1);
    PolyPlan p;
    std::printf("reject %s %d\n", name, poly_plan_build(a.data(), degree, basis, scale, level, q.data(), p));
}

int main() {
    const double scale = std::ldexp(1.0, 45);
    const int level = 10;
    int id = 0, bad = 0;
    for (int basis : {kPolyMonomial, kPolyChebyshev})
        for (int d : {1, 2, 3, 4, 7, 8, 15, 16, 31, 63, 127}) {
            std::vector<double> a((size_t)d + 1);
            for (double& v : a) v = next_coef();
            if (a[(size_t)d] == 0.0) a[(size_t)d] = 0.625;   // the degree is the stated one
            bad += emit(id++, a, basis, scale, level);
        }
    for (int basis : {kPolyMonomial, kPolyChebyshev}) {
        std::vector<double> a(16, 0.0);
        for (int i = 0; i < 8; ++i) a[(size_t)i] = next_coef();
        a[7] = -0.75;
        bad += emit(id++, a, basis, scale, level);
    }

    const std::vector<double> ok(129, 0.5);
    reject("degree-0", ok, 0, kPolyMonomial, scale, level);
    reject("degree-128", ok, 128, kPolyMonomial, scale, level);
    reject("basis", ok, 7, 2, scale, level);
    reject("levels", ok, 7, kPolyMonomial, scale, 4);      // degree 7 takes 4 levels: needs level >= 5
    reject("levels-cheb", ok, 7, kPolyChebyshev, scale, 4);
    reject("level-0", ok, 7, kPolyMonomial, scale, 0);
    std::vector<double> nan = ok, inf = ok, big = ok, flat(8, 0.0);
    nan[3] = std::numeric_limits<double>::quiet_NaN();
    inf[0] = std::numeric_limits<double>::infinity();
    big[2] = 1e30;   // k = a S / D is near 1e30 2^45 > 2^126
    flat[0] = 0.25;
    reject("nan-coefficient", nan, 7, kPolyMonomial, scale, level);
    reject("inf-coefficient", inf, 7, kPolyChebyshev, scale, level);
    reject("nan-scale", ok, 7, kPolyMonomial, std::numeric_limits<double>::quiet_NaN(), level);
    reject("inf-scale", ok, 7, kPolyMonomial, std::numeric_limits<double>::infinity(), level);
    reject("zero-scale", ok, 7, kPolyMonomial, 0.0, level);
    reject("constant-too-large", big, 7, kPolyMonomial, scale, level);
    reject("constant-polynomial", flat, 7, kPolyMonomial, scale, level);
    return bad ? 1 : 0;
}

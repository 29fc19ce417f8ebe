// poly_plan.hpp -- the host planner of encrypted polynomial evaluation (poly.hip, include/mfhe.h mfhe_poly_plan_*): a
// coefficient vector in the monomial or the Chebyshev basis becomes a baby-step giant-step (Paterson-Stockmeyer) list
// of nodes with exact scale and level bookkeeping.  Standard library only, no HIP dependency
// (tests/cpp/poly_plan_main.cpp includes this file with a host compiler alone).
//
// Every node has one form, on registers that hold ciphertexts (register 0 is the input, x or T_1):
//   t        = reg[mul_a] reg[mul_b], relinearised, not rescaled          (optional)
//   y        = k_mul t + sum_j k_j reg[src_j] + k_0                       (at the node's level l, scale S)
//   reg[dst] = ModDown(y) by limb l - 1                                   (level l - 1, scale S / q_(l-1))
// A constant is the integer rint(a S / D), a the real coefficient and D the tracked scale of the term's register (1 for
// k_0), so no two scales ever have to match: a mismatch is absorbed by an integer near the scale, whose rounding costs
// about 1 / scale relative.  With a product S = D_a D_b and k_mul is 1 or 2; without, S = D_in q_(l-1), which keeps
// the result near the input's scale.
//
//   power    : x^(a+b) = x^a x^b, T_(a+b) = 2 T_a T_b - T_(a-b), a = ceil(j / 2), b = floor(j / 2): a - b is 0 (the
//              addend -rint(S)) or 1 (the term -rint(S / D_1) T_1)
//   leaf     : a polynomial of degree < m in the baby powers 1 .. m - 1, no product
//   giant    : quotient x giant + remainder, the giants m 2^i; monomial p = x^g q + r, Chebyshev q = a_g +
//              sum_(i>g) 2 a_i T_(i-g), r = sum_(i<g) a_i T_i - sum_(i>g) a_i T_(2g-i), recursing on the top giant
//              g <= deg < 2g
// m = 2^ceil(e / 2), e = ceil(log2(d + 1)) for the effective degree d (trailing zero coefficients dropped).  Powers
// nobody reads are not computed, a zero constant is not a term, a polynomial that is one power with coefficient 1 is
// that power's register, and a constant quotient makes the giant step a sum without a product.  The levels consumed
// are at most ceil(log2(d + 1)) + 1: a power j sits ceil(log2 j) below the input, a leaf one below its powers, and a
// giant step of span m 2^i one below the deeper of its quotient and its giant.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace mfhe {

using pp_u128 = unsigned __int128;

constexpr int kPolyMaxDegree = 127;
constexpr int kPolyMaxTerms = 64;   // terms of one node's sum, the product's among them (mfhe_ct_lincomb's limit)
enum { kPolyMonomial = 0, kPolyChebyshev = 1 };

// Why a plan was refused; poly_plan_main prints these.
enum PolyPlanError {
    kPolyPlanOk = 0,
    kPolyPlanNull = 10,        // null coefficients or moduli
    kPolyPlanDegree = 11,      // degree outside [1, 127]
    kPolyPlanBasis = 12,       // unknown basis
    kPolyPlanNotFinite = 13,   // a coefficient or the scale is not finite, or the scale is not positive
    kPolyPlanConstant = 14,    // every coefficient above a_0 is zero: nothing to evaluate
    kPolyPlanLevels = 15,      // the plan needs more levels than level - 1
    kPolyPlanOverflow = 16,    // a constant of magnitude >= 2^126
    kPolyPlanTerms = 17,       // more than 64 terms in one node
};

inline const char* poly_plan_error_text(int e) {
    switch (e) {
        case kPolyPlanOk: return "ok";
        case kPolyPlanNull: return "null coefficients or moduli";
        case kPolyPlanDegree: return "degree outside [1, 127]";
        case kPolyPlanBasis: return "unknown basis";
        case kPolyPlanNotFinite: return "a coefficient or the scale is not finite, or the scale is not positive";
        case kPolyPlanConstant: return "every coefficient above a_0 is zero";
        case kPolyPlanLevels: return "the plan needs more levels than level - 1";
        case kPolyPlanOverflow: return "a constant of magnitude >= 2^126";
        case kPolyPlanTerms: return "more than 64 terms in one node";
        default: return "unknown";
    }
}

struct PolyConst {
    bool negative;
    pp_u128 mag;
};

struct PolyNode {
    int dst = 0, level = 0;          // reg[dst] is written at level - 1
    int mul_a = -1, mul_b = -1;      // registers of the product, -1: none
    int k_mul = -1;                  // constant index of the product's multiplier (1 or 2)
    std::vector<int> src, k;         // the other terms: register and constant index
    std::vector<double> coef;        // their real coefficients
    int addend_k = -1;               // constant index of k_0, -1: none
    double addend_coef = 0.0;
    double scale_in = 0.0, scale_out = 0.0;   // S and S / q_(level-1)
};

struct PolyPlan {
    int basis = 0, degree = 0, level = 0;
    int nreg = 0, nmul = 0, depth = 0, out_reg = 0, out_level = 0;
    double in_scale = 0.0, out_scale = 0.0;
    std::vector<PolyNode> nodes;
    std::vector<PolyConst> consts;
    std::vector<uint64_t> moduli;    // limbs [0, level)
};

// the integer mantissa and exponent of a positive finite double: v = m 2^e, m < 2^53
inline void pp_split(double v, uint64_t& m, int& e) {
    int ex;
    const double f = std::frexp(v, &ex);
    m = (uint64_t)std::ldexp(f, 53);
    e = ex - 53;
}

// rint(|a| s / d) for finite a and positive finite s, d, in integers: within max(1, 2^-70 of the result) of the exact
// quotient of the three doubles.  False when the result reaches 2^126.
inline bool pp_scaled_constant(double a, double s, double d, pp_u128& mag) {
    mag = 0;
    if (a == 0.0) return true;
    uint64_t ma, ms, md;
    int ea, es, ed;
    pp_split(std::fabs(a), ma, ea);
    pp_split(s, ms, es);
    pp_split(d, md, ed);
    pp_u128 num = (pp_u128)ma * ms;   // < 2^106
    int sh = ea + es - ed;
    if (sh <= 0) {
        const pp_u128 n = -sh >= 128 ? 0 : num >> -sh;
        mag = (n + md / 2) / md;
        return (mag >> 126) == 0;
    }
    int lz = 0;
    while (!((num << lz) >> 127)) ++lz;
    const int s1 = sh < lz ? sh : lz;
    num <<= s1;
    sh -= s1;
    const pp_u128 qd = num / md, rem = num % md;
    if (sh == 0) {
        mag = qd + (2 * rem >= md ? 1 : 0);
        return (mag >> 126) == 0;
    }
    // num >= 2^127 and md < 2^53: qd >= 2^74, so what the shift drops is below 2^-74 of the result
    if (sh >= 126 - 74) return false;
    if ((qd >> (126 - sh)) != 0) return false;
    mag = qd << sh;
    return true;
}

class PolyPlanner {
  public:
    PolyPlanner(PolyPlan& p) : p_(p) {}

    int build(const double* coeffs, int degree, int basis, double in_scale, int level, const uint64_t* moduli) {
        p_ = PolyPlan{};
        if (!coeffs || !moduli) return kPolyPlanNull;
        if (degree < 1 || degree > kPolyMaxDegree) return kPolyPlanDegree;
        if (basis != kPolyMonomial && basis != kPolyChebyshev) return kPolyPlanBasis;
        if (!std::isfinite(in_scale) || in_scale <= 0.0) return kPolyPlanNotFinite;
        for (int i = 0; i <= degree; ++i)
            if (!std::isfinite(coeffs[i])) return kPolyPlanNotFinite;
        if (level < 1) return kPolyPlanLevels;
        p_.basis = basis; p_.degree = degree; p_.level = level; p_.in_scale = in_scale;
        p_.moduli.assign(moduli, moduli + level);
        std::vector<double> c(coeffs, coeffs + degree + 1);
        const int d = eff_degree(c);
        if (d == 0) return kPolyPlanConstant;
        int e = 0;
        while ((1 << e) < d + 1) ++e;
        m_ = 1 << ((e + 1) / 2);
        regs_.push_back({level, in_scale});
        pow_[1] = 0;
        const Val v = eval(c);
        if (err_) return err_;
        p_.out_reg = v.reg;
        p_.out_level = regs_[v.reg].level;
        p_.out_scale = regs_[v.reg].scale;
        p_.depth = level - p_.out_level;
        reuse_registers();
        return kPolyPlanOk;
    }

  private:
    struct Reg {
        int level;
        double scale;
    };
    struct Val {
        bool is_const;
        double c;
        int reg;
    };

    static int eff_degree(const std::vector<double>& c) {
        int d = (int)c.size() - 1;
        while (d > 0 && c[d] == 0.0) --d;
        return d;
    }

    int constant(bool neg, pp_u128 mag) {
        for (size_t i = 0; i < p_.consts.size(); ++i)
            if (p_.consts[i].mag == mag && p_.consts[i].negative == neg) return (int)i;
        p_.consts.push_back({neg, mag});
        return (int)p_.consts.size() - 1;
    }
    // index of rint(a s / d), or -1: zero (not a term) or an error (err_ set)
    int scaled(double a, double s, double d) {
        pp_u128 mag;
        if (!pp_scaled_constant(a, s, d, mag)) {
            err_ = kPolyPlanOverflow;
            return -1;
        }
        return mag == 0 ? -1 : constant(a < 0.0, mag);
    }

    // the node's level from its registers; 0 with err_ set when no limb would be left
    int node_level(const PolyNode& n) {
        int l = p_.level;
        if (n.mul_a >= 0) l = std::min(l, std::min(regs_[n.mul_a].level, regs_[n.mul_b].level));
        for (int s : n.src) l = std::min(l, regs_[s].level);
        if (l < 2) {
            err_ = kPolyPlanLevels;
            return 0;
        }
        return l;
    }

    // appends the node (level, registers and real coefficients set, scale_in = S): constants, terms, destination
    int finish(PolyNode n, const std::vector<int>& src, const std::vector<double>& coef, double addend) {
        const double S = n.scale_in;
        for (size_t j = 0; j < src.size(); ++j) {
            const int k = scaled(coef[j], S, regs_[src[j]].scale);
            if (err_) return 0;
            if (k < 0) continue;
            n.src.push_back(src[j]);
            n.k.push_back(k);
            n.coef.push_back(coef[j]);
        }
        if (addend != 0.0) {
            n.addend_k = scaled(addend, S, 1.0);
            n.addend_coef = n.addend_k < 0 ? 0.0 : addend;
            if (err_) return 0;
        }
        if ((int)n.src.size() + (n.mul_a >= 0 ? 1 : 0) > kPolyMaxTerms) {
            err_ = kPolyPlanTerms;
            return 0;
        }
        if (n.src.empty() && n.mul_a < 0) {   // every constant rounded to zero: nothing of the input is left
            err_ = kPolyPlanConstant;
            return 0;
        }
        n.scale_out = S / (double)p_.moduli[n.level - 1];
        n.dst = (int)regs_.size();
        regs_.push_back({n.level - 1, n.scale_out});
        if (n.mul_a >= 0) ++p_.nmul;
        p_.nodes.push_back(n);
        return n.dst;
    }

    // y = kmul reg[a] reg[b] + sum coef_j reg[src_j] + addend at S = D_a D_b
    int emit_mul(int a, int b, int kmul, std::vector<int> src, std::vector<double> coef, double addend) {
        PolyNode n;
        n.mul_a = a; n.mul_b = b;
        n.src = src;
        n.level = node_level(n);
        n.src.clear();
        if (err_) return 0;
        n.scale_in = regs_[a].scale * regs_[b].scale;
        n.k_mul = constant(false, (pp_u128)kmul);
        return finish(n, src, coef, addend);
    }
    // y = sum coef_j reg[src_j] + addend at S = D_in q_(l-1)
    int emit_lin(std::vector<int> src, std::vector<double> coef, double addend) {
        PolyNode n;
        n.src = src;
        n.level = node_level(n);
        n.src.clear();
        if (err_) return 0;
        n.scale_in = p_.in_scale * (double)p_.moduli[n.level - 1];
        return finish(n, src, coef, addend);
    }

    int power(int j) {
        const auto it = pow_.find(j);
        if (it != pow_.end()) return it->second;
        const int a = (j + 1) / 2, b = j / 2;
        const int ra = power(a), rb = power(b);
        if (err_) return 0;
        int r;
        if (p_.basis == kPolyMonomial)
            r = emit_mul(ra, rb, 1, {}, {}, 0.0);
        else if (a == b)
            r = emit_mul(ra, rb, 2, {}, {}, -1.0);        // - T_0
        else
            r = emit_mul(ra, rb, 2, {0}, {-1.0}, 0.0);    // - T_1
        pow_[j] = r;
        return r;
    }

    Val eval(const std::vector<double>& c) {
        const int deg = eff_degree(c);
        if (err_) return {true, 0.0, 0};
        if (deg == 0) return {true, c[0], 0};
        if (deg < m_) {
            std::vector<int> src;
            std::vector<double> coef;
            for (int j = 1; j <= deg; ++j)
                if (c[j] != 0.0) {
                    src.push_back(power(j));
                    coef.push_back(c[j]);
                }
            if (err_) return {true, 0.0, 0};
            // one power with coefficient 1 is that power's register (not the input's: a plan has a node)
            if (src.size() == 1 && src[0] != 0 && coef[0] == 1.0 && c[0] == 0.0) return {false, 0.0, src[0]};
            return {false, 0.0, emit_lin(src, coef, c[0])};
        }
        int g = m_;
        while (2 * g <= deg) g *= 2;
        std::vector<double> q((size_t)(deg - g + 1)), r(c.begin(), c.begin() + g);
        if (p_.basis == kPolyMonomial) {
            for (int i = g; i <= deg; ++i) q[(size_t)(i - g)] = c[i];
        } else {
            q[0] = c[g];
            for (int i = g + 1; i <= deg; ++i) {
                q[(size_t)(i - g)] = 2.0 * c[i];
                r[(size_t)(2 * g - i)] -= c[i];
            }
        }
        const Val vq = eval(q), vr = eval(r);
        const int rg = power(g);
        if (err_) return {true, 0.0, 0};
        std::vector<int> src;
        std::vector<double> coef;
        if (vq.is_const) {
            src.push_back(rg);
            coef.push_back(vq.c);
        }
        if (!vr.is_const) {
            src.push_back(vr.reg);
            coef.push_back(1.0);
        }
        const double addend = vr.is_const ? vr.c : 0.0;
        const int dst = vq.is_const ? emit_lin(src, coef, addend) : emit_mul(vq.reg, rg, 1, src, coef, addend);
        return {false, 0.0, dst};
    }

    // Registers are renamed so that one whose last reader has run is written again (register 0, the input, and the
    // result excepted).  A node's destination is never one of its own registers: the sum is written there.
    void reuse_registers() {
        const int nv = (int)regs_.size();
        std::vector<int> last(nv, -1), phys(nv, -1);
        for (size_t i = 0; i < p_.nodes.size(); ++i) {
            const PolyNode& n = p_.nodes[i];
            if (n.mul_a >= 0) last[n.mul_a] = last[n.mul_b] = (int)i;
            for (int s : n.src) last[s] = (int)i;
        }
        last[0] = last[p_.out_reg] = (int)p_.nodes.size();
        std::vector<int> free_list;
        int next = 1;
        phys[0] = 0;
        for (size_t i = 0; i < p_.nodes.size(); ++i) {
            PolyNode& n = p_.nodes[i];
            int d;
            if (free_list.empty())
                d = next++;
            else {
                d = free_list.back();
                free_list.pop_back();
            }
            phys[n.dst] = d;
            std::vector<int> reads = n.src;
            if (n.mul_a >= 0) {
                reads.push_back(n.mul_a);
                if (n.mul_b != n.mul_a) reads.push_back(n.mul_b);
            }
            for (size_t x = 0; x < reads.size(); ++x) {
                bool seen = false;
                for (size_t y = 0; y < x; ++y) seen = seen || reads[y] == reads[x];
                if (!seen && last[reads[x]] == (int)i) free_list.push_back(phys[reads[x]]);
            }
            if (last[n.dst] < 0) free_list.push_back(d);   // never read (cannot happen: every node is read or the result)
            n.dst = d;
            if (n.mul_a >= 0) {
                n.mul_a = phys[n.mul_a];
                n.mul_b = phys[n.mul_b];
            }
            for (int& s : n.src) s = phys[s];
        }
        p_.out_reg = phys[p_.out_reg];
        p_.nreg = next;
    }

    PolyPlan& p_;
    std::vector<Reg> regs_;
    std::map<int, int> pow_;
    int m_ = 2;
    int err_ = 0;
};

inline int poly_plan_build(const double* coeffs, int degree, int basis, double in_scale, int level,
                           const uint64_t* moduli, PolyPlan& out) {
    PolyPlanner b(out);
    return b.build(coeffs, degree, basis, in_scale, level, moduli);
}

// constant i mod q, canonical
inline uint64_t poly_plan_residue(const PolyConst& k, uint64_t q) {
    const uint64_t r = (uint64_t)(k.mag % q);
    return k.negative && r ? q - r : r;
}

// the table [nk][level] the nodes' sums read
inline std::vector<uint64_t> poly_plan_residues(const PolyPlan& p) {
    std::vector<uint64_t> t(p.consts.size() * (size_t)p.level);
    for (size_t i = 0; i < p.consts.size(); ++i)
        for (int r = 0; r < p.level; ++r) t[i * (size_t)p.level + r] = poly_plan_residue(p.consts[i], p.moduli[r]);
    return t;
}

}  // namespace mfhe

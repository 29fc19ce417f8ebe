// lintrans.hpp -- encrypted linear transforms by baby-step giant-step (lintrans.hip): the host-side validation of a
// transform plan, and the kernel arguments and launchers of the two kernels.  The validation is plain integer code
// with no HIP dependency (tests/cpp/lt_plan_main.cpp includes this file with a host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mfhe.h"

namespace mfhe {

// most terms of one multiply-accumulate (one giant step of a plan): the index arrays travel in the kernel arguments
constexpr int kLtMaxTerms = 64;

// Why a plan was rejected; lt_plan_main exits with these.
enum LtPlanError {
    kLtPlanOk = 0,
    kLtPlanNull = 10,         // null plan or a null array
    kLtPlanCounts = 11,       // n_baby, n_giant or nterms < 1
    kLtPlanBabyFirst = 12,    // baby_elt[0] != 1
    kLtPlanGiantFirst = 13,   // giant_elt[0] != 1
    kLtPlanElement = 14,      // an element that is even, < 1 or >= 2 N
    kLtPlanTermIndex = 15,    // term_baby or term_giant out of range
    kLtPlanUnsorted = 16,     // term_giant decreases
    kLtPlanTooManyTerms = 17, // more than kLtMaxTerms terms in one giant step
    kLtPlanNullKey = 18,      // a step that is used (other than step 0) has no key
};

inline const char* lt_plan_error_text(int e) {
    switch (e) {
        case kLtPlanOk: return "ok";
        case kLtPlanNull: return "null plan or null array";
        case kLtPlanCounts: return "n_baby, n_giant and nterms must be >= 1";
        case kLtPlanBabyFirst: return "baby_elt[0] != 1";
        case kLtPlanGiantFirst: return "giant_elt[0] != 1";
        case kLtPlanElement: return "a Galois element is not an odd integer in [1, 2 N)";
        case kLtPlanTermIndex: return "a term index is out of range";
        case kLtPlanUnsorted: return "term_giant is not non-decreasing";
        case kLtPlanTooManyTerms: return "more than 64 terms in one giant step";
        case kLtPlanNullKey: return "a used step has a null key";
        default: return "unknown";
    }
}

// The terms of one giant step: terms [first, first + count) of the plan (term_giant is sorted, so they are a run).
struct LtGroup {
    int giant, first, count;
};

// Checks a plan for ring degree n and groups its terms by giant step (only the giants that have terms, in order);
// baby_used[b] = some term reads baby step b.  Nothing is written on failure but the two vectors may be partly filled.
inline int lt_plan_validate(const mfhe_lt_plan* pl, uint64_t n, std::vector<LtGroup>& groups,
                            std::vector<char>& baby_used) {
    groups.clear();
    baby_used.clear();
    if (!pl) return kLtPlanNull;
    if (pl->n_baby < 1 || pl->n_giant < 1 || pl->nterms < 1) return kLtPlanCounts;
    if (!pl->baby_elt || !pl->giant_elt || !pl->d_gk_baby || !pl->d_gk_giant || !pl->term_giant || !pl->term_baby)
        return kLtPlanNull;
    if (pl->baby_elt[0] != 1) return kLtPlanBabyFirst;
    if (pl->giant_elt[0] != 1) return kLtPlanGiantFirst;
    auto elt_ok = [n](int g) { return g >= 1 && (g & 1) && (uint64_t)g < 2 * n; };
    for (int b = 0; b < pl->n_baby; ++b)
        if (!elt_ok(pl->baby_elt[b])) return kLtPlanElement;
    for (int a = 0; a < pl->n_giant; ++a)
        if (!elt_ok(pl->giant_elt[a])) return kLtPlanElement;
    baby_used.assign((size_t)pl->n_baby, 0);
    for (int t = 0; t < pl->nterms; ++t) {
        const int a = pl->term_giant[t], b = pl->term_baby[t];
        if (a < 0 || a >= pl->n_giant || b < 0 || b >= pl->n_baby) return kLtPlanTermIndex;
        if (t && a < pl->term_giant[t - 1]) return kLtPlanUnsorted;
        if (groups.empty() || groups.back().giant != a) groups.push_back({a, t, 0});
        if (++groups.back().count > kLtMaxTerms) return kLtPlanTooManyTerms;
        baby_used[(size_t)b] = 1;
    }
    for (int b = 1; b < pl->n_baby; ++b)
        if (baby_used[(size_t)b] && !pl->d_gk_baby[b]) return kLtPlanNullKey;
    for (const LtGroup& g : groups)
        if (g.giant != 0 && !pl->d_gk_giant[g.giant]) return kLtPlanNullKey;
    return kLtPlanOk;
}

}  // namespace mfhe

#if defined(__HIPCC__)
#include "keyswitch.hpp"

namespace mfhe {

// Kernel arguments of the plaintext multiply-accumulate.  Strides and ncoeff in units of V words (V = 1 scalar, V = 2
// the 16-byte form).  u [nslots][npoly][2][rows][ncoeff], pt [npt][pt_level + K][ncoeff], acc [npoly][2][rows][ncoeff].
struct LtMacArgs {
    const void* u;
    const void* pt;
    void* acc;
    uint64_t slot_stride, poly_stride, pt_stride, acc_stride;
    uint64_t ncoeff;        // elements per row
    uint64_t npairs, prun;  // (polynomial, component) pairs = 2 npoly; pairs one thread walks (grid z = ceil(npairs / prun))
    int nterms, level, pt_level, special_start, nspecial;
    int term_u[kLtMaxTerms], term_pt[kLtMaxTerms];   // slot and plaintext of term t, by value: nothing is copied
};

// One launch: acc[p][c][r] = sum_t pt[term_pt[t]][ptrow(r)] u[term_u[t]][p][c][r] mod q_r.  Strides and ncoeff given in
// words; the 16-byte form is chosen here when ncoeff and every stride are even and the three buffers 16-byte aligned.
// Arguments already checked.
int launch_lt_pt_mac(mfhe_ctx* c, LtMacArgs a, size_t npoly, hipStream_t st);

// One launch over rows [0, nrows) of one component of npoly polynomials: with ADD, u[p][r][i] += pmod[r] src[p][r][pi_g(i)]
// on nrows = level rows; without, u[p][r][i] = pmod[r] src[p][r][i] on the first `level` rows and 0 on the rest of
// nrows = level + K.  galois_elt 0 or 1: no gather.  pmod: [level] P mod q_r (ksk_pmod_table).
int launch_lt_c0(mfhe_ctx* c, const uint64_t* src, size_t src_stride, uint64_t* u, size_t u_stride, size_t npoly,
                 int level, int nrows, const uint64_t* pmod, uint32_t galois_elt, bool add, hipStream_t st);

}  // namespace mfhe
#endif

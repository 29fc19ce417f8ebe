// Runs the host-side validation of a linear-transform plan (csrc/lintrans.hpp lt_plan_validate):
//   lt_plan_main <N> <baby_elt> <giant_elt> <baby keys> <giant keys> <term_giant> <term_baby>
// Every list is comma-separated integers, "-" for an empty list, "null:<count>" for a null array that claims <count>
// entries ("noplan" as baby_elt: a null plan); a key list holds 0 (null key) or 1 per step.  Exit status 0 and, on
// stdout, one line "group <giant> <first> <count>" per giant step that has terms and one line "used <b> ..." with the
// baby steps in use; or the LtPlanError of the rejection (10 .. 18); 2 for a malformed command line.  tests/test_lintrans_cpu.py builds this with the host compiler under the address and
// undefined-behaviour sanitizers.  No GPU, no libmfhe.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lintrans.hpp"

static bool parse(const char* s, std::vector<int>& out, int& null_count) {
    out.clear();
    null_count = -1;   // not a null array
    if (std::strcmp(s, "noplan") == 0) null_count = 0;
    if (std::strncmp(s, "null:", 5) == 0) null_count = std::atoi(s + 5);
    if (null_count >= 0 || std::strcmp(s, "-") == 0) return true;
    const char* p = s;
    while (*p) {
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p || v < -2147483647L || v > 2147483647L) return false;
        out.push_back((int)v);
        p = end;
        if (*p == ',') ++p;
        else if (*p) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s N baby_elt giant_elt baby_keys giant_keys term_giant term_baby\n", argv[0]);
        return 2;
    }
    const unsigned long long n = std::strtoull(argv[1], nullptr, 10);
    std::vector<int> v[6];
    int nc[6];
    bool null[6];
    size_t len[6];
    for (int k = 0; k < 6; ++k) {
        if (!parse(argv[2 + k], v[k], nc[k])) return 2;
        null[k] = nc[k] >= 0;
        len[k] = null[k] ? (size_t)nc[k] : v[k].size();
    }
    static const uint64_t some_key = 0;
    std::vector<const uint64_t*> kb, kg;
    for (int f : v[2]) kb.push_back(f ? &some_key : nullptr);
    for (int f : v[3]) kg.push_back(f ? &some_key : nullptr);
    if (len[2] != len[0] || len[3] != len[1] || len[4] != len[5]) return 2;
    // exact-size heap copies, so that a read past an array is the sanitizer's to catch
    mfhe_lt_plan pl{};
    pl.n_baby = (int)len[0];
    pl.n_giant = (int)len[1];
    pl.nterms = (int)len[4];
    pl.baby_elt = null[0] ? nullptr : v[0].data();
    pl.giant_elt = null[1] ? nullptr : v[1].data();
    pl.d_gk_baby = null[2] ? nullptr : kb.data();
    pl.d_gk_giant = null[3] ? nullptr : kg.data();
    pl.term_giant = null[4] ? nullptr : v[4].data();
    pl.term_baby = null[5] ? nullptr : v[5].data();
    std::vector<mfhe::LtGroup> groups;
    std::vector<char> used;
    const int e = mfhe::lt_plan_validate(std::strcmp(argv[2], "noplan") == 0 ? nullptr : &pl, n, groups, used);
    if (e) {
        std::fprintf(stderr, "rejected: %s\n", mfhe::lt_plan_error_text(e));
        return e;
    }
    for (const mfhe::LtGroup& g : groups) std::printf("group %d %d %d\n", g.giant, g.first, g.count);
    std::printf("used");
    for (size_t b = 0; b < used.size(); ++b)
        if (used[b]) std::printf(" %zu", b);
    std::printf("\n");
    return 0;
}

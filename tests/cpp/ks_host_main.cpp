// Prints the host arithmetic of the key switch and its drivers (csrc/ks_host.hpp), one line per case:
//   grid <ncoeff> <block> <bx>
//   wide <case> <wide> <the strides afterwards>
//   runs <n> <bx> <rows> <min_run> <prun> <runs>
//   fold <rows> <npoly> <gy> <gz>
//   ws <npoly> <beta> <rows> <N> <raised> <acc> <scratch> <end> <ks_ws_words>
//   span <npoly> <stride> <words> <span>
//   overlap <case> <ks_find_overlap>
// tests/test_ks_host_cpu.py builds this with the host compiler under the address and undefined-behaviour sanitizers and
// compares every line with a Python restatement of the rule.  No GPU, no libmfhe.
#include <cinttypes>
#include <cstdio>

#include "ks_host.hpp"

using namespace mfhe;

static void wide_case(const char* name, uint64_t ncoeff, uint64_t s0, uint64_t s1, const void* p0, const void* p1) {
    const bool w = ks_wide({&ncoeff, &s0, &s1}, {p0, p1});
    std::printf("wide %s %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", name, (int)w, ncoeff, s0, s1);
}

static void overlap_case(const char* name, std::initializer_list<KsRange> in, std::initializer_list<KsRange> out) {
    std::printf("overlap %s %d\n", name, ks_find_overlap(in.begin(), in.size(), out.begin(), out.size()));
}

int main() {
    for (uint64_t n : {1ull, 2ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1ull << 15}) {
        const KsRowGrid g = ks_row_grid(n);
        std::printf("grid %" PRIu64 " %" PRIu32 " %" PRIu64 "\n", n, g.block, g.bx);
    }

    alignas(16) static uint64_t buf[64];
    wide_case("even-aligned", 16, 32, 48, buf, buf + 2);
    wide_case("odd-stride", 16, 33, 48, buf, buf + 2);
    wide_case("pointer-off-8", 16, 32, 48, buf, buf + 3);
    wide_case("odd-ncoeff", 15, 32, 48, buf, buf + 2);

    const uint64_t runs_n[] = {0, 1, 3, 4, 2340, 2341, 3001};
    for (uint64_t n : runs_n) {
        const KsRuns r = ks_runs(n, 1, 7, 4);
        std::printf("runs %" PRIu64 " 1 7 4 %" PRIu64 " %" PRIu64 "\n", n, r.prun, r.runs);
    }
    // the longest grid z the rule can give: one block column of one row, a batch far beyond 65535 runs of 4
    const KsRuns big = ks_runs(1ull << 40, 1, 1, 4);
    std::printf("runs %" PRIu64 " 1 1 4 %" PRIu64 " %" PRIu64 "\n", 1ull << 40, big.prun, big.runs);

    const uint64_t fold[][2] = {{3, 21845}, {3, 21846}, {1, 65543}};
    for (const auto& f : fold) {
        const KsFold k = ks_fold(f[0] * f[1]);
        std::printf("fold %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", f[0], f[1], k.gy, k.gz);
    }

    const size_t ws[][4] = {{1, 1, 2, 2}, {3, 3, 7, 16}, {0, 2, 7, 16}};
    for (const auto& s : ws) {
        const KsWs w = ks_ws(s[0], (int)s[1], s[2], s[3]);
        std::printf("ws %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s[0], s[1], s[2], s[3], w.raised, w.acc, w.scratch, w.end,
                    ks_ws_words(s[0], (int)s[1], s[2], s[3]));
    }

    const size_t span[][3] = {{0, 10, 4}, {1, 10, 4}, {3, 10, 4}};
    for (const auto& s : span) std::printf("span %zu %zu %zu %zu\n", s[0], s[1], s[2], ks_span(s[0], s[1], s[2]));

    overlap_case("disjoint", {{buf, 8}}, {{buf + 16, 8}});
    overlap_case("touching", {{buf, 8}}, {{buf + 8, 8}});
    overlap_case("one-word-shared", {{buf, 9}}, {{buf + 8, 8}});
    overlap_case("empty-input-inside-output", {{buf + 4, 0}}, {{buf, 8}});
    overlap_case("empty-output-inside-input", {{buf, 8}}, {{buf + 4, 0}});
    overlap_case("output-against-output", {{buf, 8}}, {{buf + 16, 8}, {buf + 23, 8}});
    overlap_case("second-output-against-input", {{buf, 8}, {buf + 40, 8}}, {{buf + 16, 8}, {buf + 47, 8}});
    return 0;
}

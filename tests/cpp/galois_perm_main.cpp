// Prints the evaluation-domain gather of a Galois automorphism (csrc/galois.hpp galois_perm_index):
//   galois_perm_main <log_n> <g>
// One source index per line, for i = 0 .. 2^log_n - 1.  tests/test_galois_cpu.py builds this with the host compiler
// under the address and undefined-behaviour sanitizers and compares every line with the Python model.  No GPU, no
// libmfhe.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "galois.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s log_n g\n", argv[0]);
        return 2;
    }
    const int log_n = std::atoi(argv[1]);
    const unsigned long long g = std::strtoull(argv[2], nullptr, 10);
    if (log_n < 1 || log_n > 30) return 3;
    if (!(g & 1ull) || g >= (2ull << log_n)) return 3;
    const uint32_t n = 1u << log_n;
    std::vector<uint32_t> pi(n);
    for (uint32_t i = 0; i < n; ++i) pi[i] = mfhe::galois_perm_index(i, (uint32_t)g, log_n);
    for (uint32_t i = 0; i < n; ++i) std::printf("%" PRIu32 "\n", pi[i]);
    return 0;
}

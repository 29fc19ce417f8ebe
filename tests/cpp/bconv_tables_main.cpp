// Prints the RNS basis conversion tables (csrc/host_math.hpp bconv_tables) for moduli given on the command line:
//   bconv_tables_main <ns> <s_0> .. <s_(ns-1)> <d_0> .. <d_(nd-1)>
// One value per line; tests/test_bconv_cpu.py builds this with the host compiler under the address and
// undefined-behaviour sanitizers and compares every line with Python integers.  No GPU, no libmfhe.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_math.hpp"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s ns s_0 .. s_(ns-1) d_0 ..\n", argv[0]);
        return 2;
    }
    const int ns = std::atoi(argv[1]);
    if (ns < 1 || ns > argc - 2) return 2;
    std::vector<uint64_t> src, dst;
    for (int i = 2; i < argc; ++i) (i < 2 + ns ? src : dst).push_back(std::strtoull(argv[i], nullptr, 10));
    const int nd = (int)dst.size();
    mfhe::hm::BconvTables t;
    if (!mfhe::hm::bconv_tables(src.data(), ns, dst.data(), nd, t)) return 3;
    for (int i = 0; i < ns; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &t.sinv[i], 8);
        std::printf("inv %d %" PRIu64 " %" PRIu64 "\n", i, t.inv[i], t.inv_shoup[i]);
        std::printf("sinv %d %" PRIu64 "\n", i, bits);
    }
    for (int j = 0; j < nd; ++j) {
        for (int i = 0; i < ns; ++i) std::printf("c %d %d %" PRIu64 "\n", j, i, t.c[(size_t)j * ns + i]);
        std::printf("smod %d %" PRIu64 "\n", j, t.smod[j]);
        std::printf("pinv %d %" PRIu64 " %" PRIu64 "\n", j, t.pinv[j], t.pinv_shoup[j]);
    }
    return 0;
}

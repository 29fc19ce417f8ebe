// slot_geom_main -- prints what csrc/slot.hpp computes on the host (no HIP): built by tests/test_slot_cpu.py with a
// host compiler alone, under the address and undefined-behaviour sanitizers.
//   slot_geom_main geom LOG_N NPOLY ROWS   ->  "ln whole l1 l2 lcA lcB lcW ws_words"
//   slot_geom_main jinv LOG_N              ->  the N / 2 entries of jinv, one line
//   slot_geom_main consts                  ->  "threads tile_log whole_max_log"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slot.hpp"

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "consts")) {
        std::printf("%d %d %d\n", mfhe::kSlotThreads, mfhe::kSlotTileLog, mfhe::kSlotWholeMaxLog);
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "geom")) {
        const int log_n = std::atoi(argv[2]);
        const size_t npoly = std::strtoull(argv[3], nullptr, 10), rows = std::strtoull(argv[4], nullptr, 10);
        const mfhe::SlotGeom g = mfhe::slot_geom(log_n, npoly);
        std::printf("%d %d %d %d %d %d %d %zu\n", g.ln, (int)g.whole, g.l1, g.l2, g.lcA, g.lcB, g.lcW,
                    mfhe::slot_ws_words(log_n, npoly, rows));
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "jinv")) {
        const int log_n = std::atoi(argv[2]);
        std::vector<uint32_t> t((size_t)1 << (log_n - 1));
        mfhe::slot_jinv_table(log_n, t.data());
        for (uint32_t v : t) std::printf("%u ", v);
        std::printf("\n");
        return 0;
    }
    return 2;
}

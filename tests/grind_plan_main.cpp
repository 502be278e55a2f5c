// Prints the batches of csrc/grind_plan.h for every input line (tests/test_cpu_grind.py):
//   B kind start n_max          "base:count base:count ..." — the first n_max launches of a search from `start` that finds nothing,
//                               by grind_begin / grind_next as the two library entries call them, then " exhausted" if the next
//                               grind_next found no batch left
//   C                           the header's constants
// kind: 0 Blake2s, 1 Poseidon252.  Numbers are decimal and 64 bits wide.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "grind_plan.h"

using namespace tstwo;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "C") {
            std::printf("%" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIu64 "\n", kGrindNone, kGrindLanes, kGrindBlake2sSmall,
                        kGrindBlake2sSmallSpan, kGrindBlake2sLarge, kGrindP252First, kGrindP252GrowLog, kGrindP252Max);
            continue;
        }
        int kind = 0;
        uint64_t start = 0, n_max = 0;
        if (!(in >> kind >> start >> n_max)) {
            std::printf("error: bad line\n");
            continue;
        }
        GrindSearch s = grind_begin((GrindKind)kind, start);
        bool first = true;
        for (uint64_t k = 0;; k++) {
            if (!grind_next(s)) {
                std::printf("%sexhausted", first ? "" : " ");
                break;
            }
            if (k == n_max) break;
            std::printf("%s%" PRIu64 ":%" PRIu64, first ? "" : " ", s.base, s.batch);
            first = false;
        }
        std::printf("\n");
    }
    return 0;
}

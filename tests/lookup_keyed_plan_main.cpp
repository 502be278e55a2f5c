// Prints the keyed plan of csrc/lookup_plan.h, in the format of tests/lookup_keyed_plan.py::render, for every input line
// "log_range order n_groups  { n_limbs weight_addr len  addr_0 bits_0 ... addr_{n_limbs-1} bits_{n_limbs-1} } per group"
// (tests/test_cpu_lookup_keyed_plan.py); "error: <reason>" for an input without a plan.  At most 4 limbs are stored per group;
// n_limbs itself is passed on as given, so that the plan refuses it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lookup_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t log_range, order;
        uint64_t n_groups;
        if (!(in >> log_range >> order >> n_groups)) continue;
        std::vector<tstwo::LookupKeyedGroup> groups;
        for (uint64_t g = 0; g < n_groups; g++) {
            tstwo::LookupKeyedGroup G = {};
            uint64_t len;
            if (!(in >> G.n_limbs >> G.weight >> len)) break;
            G.len = (size_t)len;
            for (uint32_t j = 0; j < G.n_limbs; j++) {
                uint64_t addr;
                uint32_t bits;
                if (!(in >> addr >> bits)) break;
                if (j < tstwo::kLookupMaxLimbs) {
                    G.limbs[j] = addr;
                    G.bits[j] = bits;
                }
            }
            groups.push_back(G);
        }
        tstwo::LookupKeyedPlan p;
        if (const char *why = tstwo::lookup_keyed_plan(groups.data(), groups.size(), log_range, order, p)) {
            std::printf("error: %s\n", why);
            continue;
        }
        std::printf("%s %s %u %u %u %llu %llx %u\n", p.branch == tstwo::LookupPlan::LDS ? "LDS" : "GLOBAL", p.acc64 ? "acc64" : "acc32",
                    p.threads, p.grid_x, p.grid_y, (unsigned long long)p.wrap, (unsigned long long)p.vec, p.combine);
    }
    return 0;
}

// Prints the plan of csrc/lookup_plan.h, in the format of tests/lookup_plan.py::render, for every input line
// "log_range order addr_0 len_0 addr_1 len_1 ..." (tests/test_cpu_lookup_plan.py); "error: <reason>" for an input without a plan.
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
        if (!(in >> log_range >> order)) continue;
        std::vector<uint64_t> addrs;
        std::vector<size_t> lens;
        uint64_t a, n;
        while (in >> a >> n) {
            addrs.push_back(a);
            lens.push_back((size_t)n);
        }
        tstwo::LookupPlan p;
        if (const char *why = tstwo::lookup_plan(addrs.data(), lens.data(), lens.size(), log_range, order, p)) {
            std::printf("error: %s\n", why);
            continue;
        }
        std::printf("%s %u %u %u %llu %llx\n", p.branch == tstwo::LookupPlan::LDS ? "LDS" : "GLOBAL", p.threads, p.grid_x, p.grid_y,
                    (unsigned long long)p.wrap, (unsigned long long)p.vec);
    }
    return 0;
}

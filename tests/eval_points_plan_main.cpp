// Prints the plan of csrc/poly_eval_plan.h, in the format of tests/eval_points_plan.py::render, for every input line
// "log cols points aligned" (tests/test_cpu_eval_points_plan.py); "error: <reason>" for a group without a plan.  A line
// "results n" prints whether n results go into the page-locked page.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "poly_eval_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (line.rfind("results", 0) == 0) {
            std::string word;
            uint64_t n;
            if (in >> word >> n) std::printf("%d\n", (int)tstwo::eval_points_result_pinned((size_t)n));
            continue;
        }
        uint32_t log, points;
        uint64_t cols;
        int aligned;
        if (!(in >> log >> cols >> points >> aligned)) continue;
        tstwo::EvalPointsPlan p;
        if (const char *why = tstwo::eval_points_plan(log, (size_t)cols, points, aligned != 0, p)) {
            std::printf("error: %s\n", why);
            continue;
        }
        std::printf("%u %u %u %u %u %d %llu %llu %u %llu %llu %llu\n", p.sweeps, p.k_full, p.k_last, p.g, p.chunk_log, (int)p.fast,
                    (unsigned long long)p.chunks, (unsigned long long)p.groups1, p.levels, (unsigned long long)p.slabs,
                    (unsigned long long)p.slab_cols, (unsigned long long)p.scratch_qm31);
    }
    return 0;
}

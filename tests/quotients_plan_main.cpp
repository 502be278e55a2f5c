// Prints the launch plan of csrc/quotients_plan.h, in the names of tests/saturation.py::quotient_kernels, for every input line
// "log_size out_aligned n_union count_0 count_1 ..." (tests/test_cpu_saturation.py::test_quotient_plan_matches_the_library).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "quotients_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned log_size, aligned;
        size_t n_union, n;
        std::vector<size_t> counts;
        if (!(in >> log_size >> aligned >> n_union)) continue;
        while (in >> n) counts.push_back(n);
        tstwo::QuotientPlan plan;
        if (!tstwo::quotients_plan(log_size, counts, n_union, aligned != 0, plan)) {
            std::puts("error");
            continue;
        }
        const char *tf[2] = {"false", "true"};
        for (const tstwo::QuotientLaunch &q : plan.launches) {
            if (q.kind == tstwo::QuotientLaunch::ROW) std::printf("row ");
            else if (q.kind == tstwo::QuotientLaunch::Q8) std::printf("q8<%s,%s> ", tf[q.single], tf[q.lazy]);
            else std::printf("%s<%d,%s>@%zu ", q.kind == tstwo::QuotientLaunch::RP ? "rp" : "multi", q.nb, tf[q.accum], q.first);
        }
        std::printf("\n");
    }
    return 0;
}

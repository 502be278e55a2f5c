// Prints the plan of csrc/mle_eval_plan.h, in the format of tests/mle_eval_plan.py::render, for every input line
// "log_n n_mles is_secure aligned" (tests/test_cpu_mle_eval_plan.py); "error: <reason>" for an input without a plan.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "mle_eval_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t log_n;
        uint64_t n_mles;
        int secure, aligned;
        if (!(in >> log_n >> n_mles >> secure >> aligned)) continue;
        tstwo::MleEvalPlan p;
        if (const char *why = tstwo::mle_eval_plan(log_n, (size_t)n_mles, secure != 0, aligned != 0, p)) {
            std::printf("error: %s\n", why);
            continue;
        }
        std::printf("%u %u %d %u %u %u %u %llu\n", p.groups, p.chunk_log, (int)p.fast, p.chunks, p.grid_y, p.passes, p.blocks,
                    (unsigned long long)p.scratch_qm31);
    }
    return 0;
}

// Prints the schedule of csrc/fri_plan.h, in the format of tests/fri_plan.py::render, for every input line
// "log_last_layer_size col_log_0 col_log_1 ..." (tests/test_cpu_fri_plan.py); "error: <reason>" for an input without a schedule.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fri_plan.h"

int main() {
    static const char *const names[] = {"FIRST_TREE", "CIRCLE_WRITE", "COMMIT", "FOLD_COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "TAIL"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t last, c;
        std::vector<uint32_t> col_logs;
        if (!(in >> last)) continue;
        while (in >> c) col_logs.push_back(c);
        std::vector<tstwo::FriStep> steps;
        if (const char *why = tstwo::fri_plan(col_logs.data(), col_logs.size(), last, steps)) {
            std::printf("error: %s\n", why);
            continue;
        }
        for (size_t i = 0; i < steps.size(); i++) {
            const tstwo::FriStep &s = steps[i];
            std::printf("%s%s:%u:%u:%u:%u:%u:%u:%d", i ? " " : "", names[s.kind], s.layer, s.log, s.column, s.alpha_in, s.alpha_out, s.n_layers, (int)s.pre);
        }
        std::printf("\n");
    }
    return 0;
}

// Prints kP252CoopMaxLog (csrc/poseidon_plan.h) on the first line, then the UNFUSED schedule of csrc/fri_plan.h (fused = false: what
// tstwo_fri_commit_layers_poseidon252 runs) for every input line "log_last_layer_size col_log_0 col_log_1 ...", as
// "KIND:layer:log:column:alpha_in:alpha_out" words, or "error: <reason>" (tests/test_cpu_fri_plan_poseidon.py).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fri_plan.h"
#include "poseidon_plan.h"

int main() {
    static const char *const names[] = {"FIRST_TREE", "CIRCLE_WRITE", "COMMIT", "FOLD_COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "TAIL"};
    std::printf("kP252CoopMaxLog %d\n", tstwo::kP252CoopMaxLog);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t last, c;
        std::vector<uint32_t> col_logs;
        if (!(in >> last)) continue;
        while (in >> c) col_logs.push_back(c);
        std::vector<tstwo::FriStep> steps;
        if (const char *why = tstwo::fri_plan(col_logs.data(), col_logs.size(), last, steps, false)) {
            std::printf("error: %s\n", why);
            continue;
        }
        for (size_t i = 0; i < steps.size(); i++) {
            const tstwo::FriStep &s = steps[i];
            std::printf("%s%s:%u:%u:%u:%u:%u", i ? " " : "", names[s.kind], s.layer, s.log, s.column, s.alpha_in, s.alpha_out);
        }
        std::printf("\n");
    }
    return 0;
}

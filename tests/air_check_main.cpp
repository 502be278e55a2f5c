// What csrc/air_codegen.h's check_assert_program says about a program (tests/test_cpu_air_check.py): the validator of
// tstwo_air_check_constraints on its own, host only.  Every input line is "n_cols n_constraints w0 w1 w0 w1 ..." (decimal
// words); the answer to a line is "error: <reason>" or "ok <n_regs>".  With the argument "acc" the line goes to
// check_acc_program instead, so that the test can hold the two validators' reasons side by side.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "air_codegen.h"

int main(int argc, char **argv) {
    const bool acc = argc > 1 && !std::strcmp(argv[1], "acc");
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        size_t n_cols, n_constraints;
        if (!(in >> n_cols >> n_constraints)) continue;
        std::vector<uint32_t> words;
        uint64_t w;
        while (in >> w) words.push_back((uint32_t)w);
        uint32_t n_regs = 0;
        const char *why = acc ? tstwo::check_acc_program(words.data(), words.size() / 2, n_cols, n_constraints, n_regs)
                              : tstwo::check_assert_program(words.data(), words.size() / 2, n_cols, n_constraints, n_regs);
        if (why) std::printf("error: %s\n", why);
        else std::printf("ok %u\n", n_regs);
    }
    return 0;
}

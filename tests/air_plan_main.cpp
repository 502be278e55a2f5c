// Prints what csrc/air_plan.h and the marker of csrc/air_codegen.h give for every input line (tests/test_cpu_air_plan.py):
//   P entry kind log log_expand n_cols n_terminal program_len n_regs aligned n_cus
//         "w threads grid stride lds_bytes tally_word upload_words coeff_word cols_by_value out_by_value capturable", or
//         "error: <the entry's prefix><reason>" for an input air_refuse turns down
//   M n_constraints n_cols w0 w1 w0 w1 ...
//         the words mark_last_acc writes for the program, or "error: <reason>" when check_assert_program refuses it
//   C     the header's constants
// entry: the AirEntry in the header's order.  Numbers are decimal.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "air_codegen.h"
#include "air_plan.h"

using namespace tstwo;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "C") {
            std::printf("%u %u %u %u %u %u %u %zu %zu\n", kAirMaxLog, kAirMaxLogExpand, kAirMaxConstraints, kAirWideThreads, kAirWideCapPerCu, kAirWaveThreads,
                        kAirWaveCapPerCu, kAirTableByValue, kAirMaxUploadWords);
        } else if (what == "P") {
            AirInput i = {};
            uint32_t entry = 0, aligned = 0;
            if (!(in >> entry >> i.kind >> i.log >> i.log_expand >> i.n_cols >> i.n_terminal >> i.program_len >> i.n_regs >> aligned >> i.n_cus) || entry >= kAirEntries) {
                std::printf("error: bad line\n");
                continue;
            }
            i.entry = (AirEntry)entry, i.aligned = aligned != 0;
            if (const char *why = air_refuse(i)) {
                std::printf("error: %s%s\n", air_prefix(i.entry), why);
                continue;
            }
            const AirPlan p = air_plan(i);
            std::printf("%u %u %u %u %u %u %u %u %d %d %d\n", p.w, p.threads, p.grid, p.stride, p.lds_bytes, p.tally_word, p.upload_words, p.coeff_word,
                        (int)p.cols_by_value, (int)p.out_by_value, (int)p.capturable);
        } else if (what == "M") {
            size_t n_constraints = 0, n_cols = 0;
            in >> n_constraints >> n_cols;
            std::vector<uint32_t> words;
            for (uint32_t w; in >> w;) words.push_back(w);
            uint32_t n_regs = 0;
            if (const char *why = check_assert_program(words.data(), words.size() / 2, n_cols, n_constraints, n_regs)) {
                std::printf("error: %s\n", why);
                continue;
            }
            std::vector<uint32_t> marked(words.size());
            mark_last_acc(words.data(), words.size() / 2, marked.data());
            for (size_t k = 0; k < marked.size(); k++) std::printf("%s%u", k ? " " : "", marked[k]);
            std::printf("\n");
        } else {
            std::printf("error: bad line\n");
        }
    }
    return 0;
}

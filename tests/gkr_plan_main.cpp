// Prints the schedule csrc/gkr_plan.h makes, one line per batch, in the format of tests/gkr_plan.py render().
// stdin: one batch per line, "kind:log_n kind:log_n ..." (an empty line = an empty batch).
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gkr_plan.h"

using namespace tstwo;

static char fold_char(GkrFold f) { return f == GKR_NO_FOLD ? 'S' : f == GKR_FOLD_IN_PLACE ? 'I' : f == GKR_FOLD_NEW ? 'N' : 'B'; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<uint32_t> kinds, logs;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            unsigned k = 0, l = 0;
            if (sscanf(tok.c_str(), "%u:%u", &k, &l) != 2) return 2;
            kinds.push_back(k);
            logs.push_back(l);
        }
        GkrPlan p;
        if (const char *why = gkr_plan(kinds.data(), logs.data(), kinds.size(), p)) {
            printf("error: %s\n", why);
            continue;
        }
        printf("layers=%u block=%u pool=%" PRIu64 " off=%u,%u,%u,%u,%u,%u,%u,%u gen=", p.n_layers, p.block_words, p.pool_words, p.state_off,
               p.sums_off, p.ctv_off, p.out_off, p.ood_off[0], p.ood_off[1], p.inv_off, p.final_ood);
        for (size_t i = 0; i < p.inst.size(); i++) printf("%s%" PRIu64 "/%u", i ? "," : "", p.inst[i].gen_off, p.inst[i].gen_cols);
        for (uint32_t L = 0; L < p.n_layers; L++) {
            const GkrPlanLayer &lay = p.layers[L];
            printf(" | L%u:%u:%" PRIx64 ":%" PRIx64 ":%u:%u", L, lay.n_rounds, lay.enter, lay.active, lay.poly_off, lay.mask_off);
            for (uint32_t rem = L; rem >= 1; rem--) {
                const uint64_t lanes = gkr_round_lanes(p, L, rem);
                printf(" r%u=%" PRIx64 "/", rem, lanes);
                uint32_t j = 0;
                for (const GkrPlanInst &q : p.inst) {
                    const int n_v = gkr_n_v(q, L);
                    if (n_v < 0) continue;
                    const bool act = (lanes >> j++) & 1;
                    printf("%u%c", (uint32_t)n_v < rem ? (uint32_t)n_v : rem, act ? fold_char(gkr_round_fold(p, q, L, rem)) : '-');
                }
            }
            printf(" last=");
            for (const GkrPlanInst &q : p.inst) {
                const int n_v = gkr_n_v(q, L);
                if (n_v < 0) continue;
                putchar(n_v >= 1 ? fold_char(gkr_last_fold(p, q, L)) : '-');
            }
        }
        printf("\n");
    }
    return 0;
}

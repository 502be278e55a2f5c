// Prints the plan of csrc/cfft_plan.h, in the format of tests/cfft_plan.py::render, for every input line
// "entry ext n n_cols n_cus kb ka_max logta" (tests/test_cpu_cfft_plan.py); "error: <reason>" for an input without a plan.
// With the argument "table": the supported shapes instead, one "kind K LOGT knob_only" per line.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "cfft_plan.h"

int main(int argc, char **argv) {
    using namespace tstwo;
    static const char *const routes[] = {"small", "generic", "tiled", "fallback"};
    static const char *const kinds[] = {"whole", "bottom", "bottom_stream", "bottom_oop", "strided", "strided_stream", "strided_ext"};
    if (argc > 1 && !std::strcmp(argv[1], "table")) {
        for (const CfftShape &s : kCfftShapes)
            for (uint32_t k = s.k_lo; k <= s.k_hi; k++) std::printf("%s %u %u %d\n", kinds[s.kind], k, (unsigned)s.logt, (int)s.knob_only);
        return 0;
    }
    unsigned entry, ext, n, n_cus, kb, ka, logta;
    uint64_t n_cols;
    while (std::scanf("%u %u %u %" SCNu64 " %u %u %u %u", &entry, &ext, &n, &n_cols, &n_cus, &kb, &ka, &logta) == 8) {
        CfftPlan plan;
        if (const char *why = cfft_plan((CfftEntry)entry, ext, n, n_cols, n_cus, {kb, ka, logta}, plan)) {
            std::printf("error: %s\n", why);
            continue;
        }
        std::printf("%s:%u:%u", routes[plan.route], plan.cols_per_wg, plan.blocks);
        for (uint32_t i = 0; i < plan.n_passes; i++) {
            const CfftPass &s = plan.pass[i];
            std::printf(" %s:%u:%u:%u:%u:%u:%u:%d", kinds[s.kind], s.lo, s.k, s.logt, s.threads, s.lds_bytes, s.tiles, (int)s.scale);
        }
        std::printf("\n");
    }
    return 0;
}

// quotients_plan.h — which launches tstwo_quotients_accumulate takes for an input (host only: no HIP, no context).
// tests/saturation.py::quotient_kernels restates this in Python; tests/test_cpu_saturation.py compiles this header and compares.
#pragma once
#include <cstddef>
#include <vector>

namespace tstwo {

struct QuotientLaunch {
    enum Kind { ROW, Q8, MULTI, RP } kind;          // k_quotients_row, k_quotients8, k_quotients8_multi, k_quotients_rp
    int nb;                     // MULTI, RP: batches of this sweep (the template parameter NB)
    bool single, lazy;          // Q8: one batch in all; some batch has more than 4 column entries
    bool accum;                 // MULTI, RP: the sweep continues from the rows an earlier one wrote
    size_t first;               // first batch of the launch
};
struct QuotientPlan {
    // k >= 2 batches whose column lists overlap take the shared-load kernels, which read ONE list, the union of the batches' columns.
    // Taken when the batches hold at least 1.4 entries per union column on average — below that the zero products (a batch that
    // does not sample a column) cost more than the shared loads save.  Decided for every input: the upload carries the list if set.
    bool shared_list;
    unsigned bsel;              // row bit that separates a lane's two quads (k_quotients8, _multi): 8 from 512 rows on, else 2
    std::vector<QuotientLaunch> launches;
};

// counts[b]: column entries of batch b; n_union: distinct columns over all batches.  False — on no input, by the arithmetic below —
// if a sweep over the shared list would hold a single batch: no kernel takes one.
inline bool quotients_plan(unsigned log_size, const std::vector<size_t> &counts, size_t n_union, bool out_aligned, QuotientPlan &plan) {
    const size_t n_batches = counts.size();
    size_t n_entries = 0;
    bool lazy = false;
    for (size_t n : counts) { n_entries += n; lazy = lazy || n > 4; }
    plan = {n_batches >= 2 && n_union > 0 && 10 * n_entries >= 14 * n_union, log_size >= 9 ? 8u : 2u, {}};
    if (log_size < 3 || log_size > 30 || !out_aligned)          // 8 rows per lane: 8 rows, 32-bit word offsets, 16-byte stores
        plan.launches.push_back({QuotientLaunch::ROW, 0, false, false, false, 0});
    else if (!plan.shared_list)
        plan.launches.push_back({QuotientLaunch::Q8, 0, n_batches == 1, lazy, false, 0});
    else
        // sweeps: 2 batches -> k_quotients8_multi<2>; 3 or 4 -> the row-pair kernel k_quotients_rp<3 | 4> (log_size >= 9); more -> 4
        // (or 3) at a time, the later sweeps continuing from the rows the earlier ones wrote (5 = 3 + 2, 6 = 3 + 3, 7 = 4 + 3); below
        // log 9, 3 (or 2) at a time.  No sweep leaves a single batch behind.
        for (size_t done = 0, left; (left = n_batches - done) > 0;) {
            if (left < 2) return false;
            const bool rp = log_size >= 9 && left >= 3;
            const int nb = rp ? ((left == 3 || left == 5 || left == 6) ? 3 : 4) : ((left == 2 || left == 4) ? 2 : 3);
            plan.launches.push_back({rp ? QuotientLaunch::RP : QuotientLaunch::MULTI, nb, false, false, done != 0, done});
            done += (size_t)nb;
        }
    return true;
}

}  // namespace tstwo

// poly_eval_plan.h — how tstwo_eval_at_points launches for one group of its call (host only: no HIP, no context).
// tests/eval_points_plan.py restates this in Python; tests/test_cpu_eval_points_plan.py compiles this header and compares.
//
// A group is `cols` columns of 2^log coefficients, every one sampled at the same `points` (1..16) points.
//   sweeps   k_eval_coeffs_pts<.., K> reads every coefficient once for K <= kEvalPtsMaxK points, so a group is swept
//            ceil(points / kEvalPtsMaxK) times: every sweep but the last takes kEvalPtsMaxK points, the last one `k_last`.
//   G        64 coefficients per lane (G = 4, a chunk of 2^14) when the grid then still has kEvalPtsMinWorkgroups workgroups,
//            else 16 (G = 1, 2^12): the rule of the one-point entries, with the CU count of an MI355X as a constant so that
//            the plan is a pure function of its arguments.
//   fast     16-byte loads: every column of the group is 16-byte aligned and the polynomial has a whole chunk.  Otherwise the
//            guarded word loads, which read nothing past 2^log (log 0, the constant polynomial, included).
//   levels   1 (one chunk), 2 (up to 4096 chunks: one k_eval_partials_pts launch) or 3 (more: two).  Three levels begin at
//            2^27 coefficients (G = 4 there for any column count).
//   slabs    a launch takes at most kEvalPtsSlabCols columns (grid y, and cols x K rows in grid y x z of the later levels);
//            a larger group runs slab after slab.
//   scratch  QM31 slots for the partials of ONE sweep of one slab.  Launches of one stream run in order, so every sweep of
//            every group of a call uses the same slots; the call needs the largest figure among its groups, plus the result
//            region when that is not the page-locked page (eval_points_result_pinned).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tstwo {

constexpr uint32_t kEvalPtsMaxPoints = 16;                    // TSTWO_EVAL_MAX_POINTS
constexpr uint32_t kEvalPtsMaxK = 4;                          // points per sweep (resource figures per K)
constexpr uint32_t kEvalPtsMaxLog = 31;
constexpr uint32_t kEvalPtsMinWorkgroups = 256;
constexpr size_t kEvalPtsSlabCols = 8192;
constexpr size_t kEvalPtsPinnedBytes = 64 * 1024;             // = kPinnedBytes (common.h; poly_eval.hip asserts it)

struct EvalPointsPlan {
    uint32_t sweeps;              // ceil(points / kEvalPtsMaxK)
    uint32_t k_full;              // K of every sweep but the last (kEvalPtsMaxK; 0 with one sweep)
    uint32_t k_last;              // K of the last sweep, 1..kEvalPtsMaxK
    uint32_t g;                   // 1 or 4 groups of 4096 coefficients per workgroup
    uint32_t chunk_log;           // 12 or 14
    bool fast;
    uint64_t chunks;              // grid x of the first level = partials per (column, point)
    uint64_t groups1;             // partials per (column, point) after the second level (1 unless levels == 3)
    uint32_t levels;              // 1..3
    size_t slabs;
    size_t slab_cols;             // columns of every slab but the last
    size_t scratch_qm31;
};

// Returns the reason (the text behind "eval_at_points: ") for a group without a plan.
inline const char *eval_points_plan(uint32_t log, size_t cols, uint32_t points, bool aligned, EvalPointsPlan &p) {
    p = {};
    if (cols == 0) return "a group without columns";
    if (points < 1 || points > kEvalPtsMaxPoints) return "1 to 16 points per group";
    if (log > kEvalPtsMaxLog) return "log size out of range";
    p.sweeps = (points + kEvalPtsMaxK - 1) / kEvalPtsMaxK;
    p.k_full = p.sweeps > 1 ? kEvalPtsMaxK : 0;
    p.k_last = points - (p.sweeps - 1) * kEvalPtsMaxK;
    bool wide = false;
    if (log >= 14) {
        const uint32_t sh = log - 14;                         // cols << sh >= 256, without overflow
        wide = sh >= 8 || cols >= (kEvalPtsMinWorkgroups >> sh);
    }
    p.g = wide ? 4 : 1;
    p.chunk_log = wide ? 14 : 12;
    p.fast = aligned && log >= p.chunk_log;
    p.chunks = log > p.chunk_log ? 1ull << (log - p.chunk_log) : 1;
    p.groups1 = p.chunks > 4096 ? p.chunks / 4096 : 1;
    p.levels = p.chunks == 1 ? 1 : p.chunks <= 4096 ? 2 : 3;
    p.slabs = (cols + kEvalPtsSlabCols - 1) / kEvalPtsSlabCols;
    p.slab_cols = cols < kEvalPtsSlabCols ? cols : kEvalPtsSlabCols;
    const uint32_t kmax = p.sweeps > 1 ? kEvalPtsMaxK : p.k_last;
    p.scratch_qm31 = p.levels == 1 ? 0 : p.slab_cols * kmax * (size_t)(p.chunks + (p.levels == 3 ? p.groups1 : 0));
    return nullptr;
}

// Whether the results of a call (one QM31 per (group, column, point)) go straight into the page-locked page.
inline bool eval_points_result_pinned(size_t results) { return results <= kEvalPtsPinnedBytes / 16; }

}  // namespace tstwo

// mle_eval_plan.h — how tstwo_mle_eval_at_point_{base,secure} launch for an input (host only: no HIP, no context).
// tests/mle_eval_plan.py restates this in Python; tests/test_cpu_mle_eval_plan.py compiles this header and compares.
//
// Pass 1 (k_mle_first, csrc/mle_eval.hip): grid (chunks, n_mles), 256 lanes.  A workgroup owns 2^chunk_log consecutive values of
// one MLE — the last chunk_log variables of the point — and leaves one QM31 partial.
//   base    16 values per lane per group, `groups` groups of 4096 values per workgroup: 4 (chunk_log 14) when that still leaves
//           kMleMinWorkgroups workgroups in the grid, else 1 (chunk_log 12).
//   secure  the 4 groups are the 4 coordinate columns at the same 4096 positions (chunk_log 12): 64 KiB per workgroup either way.
//   fast    16-byte loads: every column of the call is 16-byte aligned and the MLE has a whole chunk.  Otherwise the guarded
//           word loads, which read nothing past 2^log_n (the missing high positions count as zero).
// Pass 2 (k_mle_partials), only when chunks > 1: grid (1, n_mles).  One workgroup per MLE folds its `chunks` partials, 256 per
// block, `blocks` = ceil(chunks / 256) blocks one after the other: at most 2^16 partials (log_n 28), a MiB, so no third pass and
// no launch whose shape appears only above 2^24 values.  Every shape of this plan is reached by an input of at most 2^22 values
// (tests/mle_eval_plan.py: gpu_shapes, branches).
//
// kMleMinWorkgroups is a constant (the CU count of an MI355X), not a query of the device, so that the plan is a pure function of
// its arguments and the Python model reproduces it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tstwo {

constexpr uint32_t kMleEvalMaxLog = 28;                       // word offsets inside a column stay below 2^30
constexpr size_t kMleEvalMaxMles = 32768;                     // gridDim.y
constexpr uint32_t kMleGroupLog = 12;                         // 256 lanes x 16 values
constexpr uint32_t kMleMinWorkgroups = 256;
constexpr uint32_t kMleFoldBlock = 256;                       // partials per block of pass 2: one per lane

struct MleEvalPlan {
    uint32_t groups;              // 1 or 4
    uint32_t chunk_log;           // 12 or 14
    bool fast;                    // pass 1 takes 16-byte loads
    uint32_t chunks;              // grid x of pass 1 = partials per MLE
    uint32_t grid_y;              // n_mles, both passes
    uint32_t passes;              // 1 or 2
    uint32_t blocks;              // pass 2: blocks of 256 partials per workgroup (0: no pass 2)
    size_t scratch_qm31;          // QM31 slots of device scratch: the partials, then the results
};

// Returns the reason (the text behind "mle eval_at_point: ") for an input without a plan.
inline const char *mle_eval_plan(uint32_t log_n, size_t n_mles, bool is_secure, bool aligned, MleEvalPlan &p) {
    p = {};
    if (n_mles == 0) return "no MLE given";
    if (n_mles > kMleEvalMaxMles) return "more than 32768 MLEs in one call";
    if (log_n > kMleEvalMaxLog) return "more than 28 variables";
    const bool wide = !is_secure && log_n >= kMleGroupLog + 2 && (((uint64_t)n_mles << (log_n - kMleGroupLog - 2)) >= kMleMinWorkgroups);
    p.groups = (is_secure || wide) ? 4 : 1;
    p.chunk_log = kMleGroupLog + (wide ? 2 : 0);
    p.fast = aligned && log_n >= p.chunk_log;
    p.chunks = log_n > p.chunk_log ? 1u << (log_n - p.chunk_log) : 1u;
    p.grid_y = (uint32_t)n_mles;
    p.passes = p.chunks > 1 ? 2 : 1;
    p.blocks = p.chunks > 1 ? (p.chunks + kMleFoldBlock - 1) / kMleFoldBlock : 0;
    p.scratch_qm31 = n_mles * ((size_t)(p.chunks > 1 ? p.chunks : 0) + 1);
    return nullptr;
}

}  // namespace tstwo

// lookup_plan.h — how tstwo_lookup_multiplicities launches for an input (host only: no HIP, no context).
// tests/lookup_plan.py restates this in Python; tests/test_cpu_lookup_plan.py compiles this header and compares.
//
// One launch counts every column: blockIdx.y is the column, blockIdx.x strides over the column's UNITS of kLookupUnit = 4
// consecutive words, one unit per lane per step.  A unit is one 16-byte load where the column's `vec` bit is set (its address is
// 16-byte aligned, and it has a whole unit) and the unit lies wholly inside the column; the last, partial unit of such a column
// and every unit of a column without the bit are read word by word.  So a lane's stride in VALUES is the same on both paths and
// the grid wraps at one point per launch: `wrap` values of one column are covered by one pass of the grid's x extent.
//
// Two branches, by the size of the table:
//   LDS     log_range <= kLookupLdsMaxLog = 14.  A workgroup of 1024 lanes (16 waves) keeps a private histogram of 2^log_range
//           words in a 64 KiB LDS array, zeroes and flushes only those words, and adds to `out` once per non-zero bin.
//           Why 64 KiB and 1024 lanes: two such workgroups fill a CU's 2048 lanes (8 waves per SIMD, the most there is) and take
//           128 of its 160 KiB, so the histogram costs no occupancy, and tables of 2^13 and 2^14 bins stay off the global
//           branch, which takes 5 to 6 times as long on them (308 and 317 us against 50 and 67 for 2 x 2^22 uniform values;
//           all figures here: profiles/lookup_plan_sweep.jsonl, HIP events, median of 15).
//           The price is the flush: every workgroup adds each of its non-zero bins to the same 2^log_range words, so a word
//           takes one add per workgroup and these serialise.  Hence few workgroups: at most 64 in all.  Measured at 2 x 2^22
//           values with caps of 512 / 256 / 128 / 64 / 32 / 16: 171 / 93 / 57 / 46 / 46 / 62 us at 2^10 bins and
//           215 / 152 / 96 / 67 / 66 / 85 us at 2^14; at 2 x 2^20 values 166 / 91 / 54 / 38 / 30 / 29 and 86 / 77 / 66 / 54 /
//           48 / 51.  (A table of 2 bins alone prefers many workgroups, 35 us at 512 against 79 at 64: there the LDS adds
//           themselves collide.  A cap that depends on the table size was not tried.)
//   GLOBAL  above that: the range check, then one global add per value.  256 lanes, at most 2048 workgroups (eight per CU:
//           all 32 wave slots), no LDS.  This cap has not been measured against another.
//
// The caps are constants, not a query of the device, so that the Python model reproduces the grid.  They are shared by the
// columns of a call: a column gets cap / n_cols workgroups, at least one.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tstwo {

constexpr uint32_t kLookupMaxCols = 64, kLookupMaxLog = 28;
constexpr uint64_t kLookupMaxValues = (1ull << 31) - 2;      // every count is a canonical M31 value without a reduction
constexpr uint32_t kLookupUnit = 4;                          // words per lane per step
constexpr uint32_t kLookupLdsMaxLog = 14;                    // 2^14 words = 64 KiB
constexpr uint32_t kLookupLdsThreads = 1024, kLookupLdsCap = 64;
constexpr uint32_t kLookupGlobalThreads = 256, kLookupGlobalCap = 2048;

struct LookupPlan {
    enum Branch { LDS, GLOBAL } branch;
    uint32_t threads;
    uint32_t grid_x, grid_y;        // grid_x = 0: no value at all, nothing is launched (the entry only zeroes)
    uint64_t wrap;                  // values of one column per pass of the grid at its cap: beyond it lanes take a second unit
    uint64_t vec;                   // bit c: column c takes 16-byte loads for its whole units
};

// addrs: the columns' device addresses as integers.  Returns the reason (the text behind "lookup: ") for an input without a plan.
inline const char *lookup_plan(const uint64_t *addrs, const size_t *lens, size_t n_cols, uint32_t log_range, uint32_t order,
                               LookupPlan &p) {
    p = {};
    if (log_range < 1 || log_range > kLookupMaxLog) return "log_range must be 1 to 28";
    if (n_cols < 1 || n_cols > kLookupMaxCols) return "1 to 64 columns";
    if (order > 1) return "order must be 0 (natural) or 1 (coset)";
    uint64_t total = 0, max_units = 0;
    for (size_t c = 0; c < n_cols; c++) {
        if (lens[c] > kLookupMaxValues) return "more than 2^31 - 2 values";
        total += lens[c];
        const uint64_t units = ((uint64_t)lens[c] + kLookupUnit - 1) / kLookupUnit;
        if (units > max_units) max_units = units;
        if (addrs[c] % 16 == 0 && lens[c] >= kLookupUnit) p.vec |= 1ull << c;
    }
    if (total > kLookupMaxValues) return "more than 2^31 - 2 values";
    const bool lds = log_range <= kLookupLdsMaxLog;
    p.branch = lds ? LookupPlan::LDS : LookupPlan::GLOBAL;
    p.threads = lds ? kLookupLdsThreads : kLookupGlobalThreads;
    const uint32_t cap = (lds ? kLookupLdsCap : kLookupGlobalCap) / (uint32_t)n_cols;
    const uint32_t cap_x = cap ? cap : 1;
    p.wrap = (uint64_t)cap_x * p.threads * kLookupUnit;
    const uint64_t need = (max_units + p.threads - 1) / p.threads;
    p.grid_x = (uint32_t)(need < cap_x ? need : cap_x);
    p.grid_y = (uint32_t)n_cols;
    return nullptr;
}

}  // namespace tstwo

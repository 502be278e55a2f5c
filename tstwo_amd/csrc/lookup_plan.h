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

// ---------------------------------------------------------------------------------------------------------------------------
// tstwo_lookup_multiplicities_keyed: keys joined from up to 4 limb columns, rows weighed by a column.  tests/lookup_keyed_plan.py
// restates this; tests/test_cpu_lookup_keyed_plan.py compiles it (tests/lookup_keyed_plan_main.cpp) and compares.
//
// The launch keeps the shape above: blockIdx.y is the GROUP, blockIdx.x strides over the group's units of 4 consecutive ROWS,
// the caps are shared by the groups of a call, and `wrap` is again the number of rows of one group per pass of a capped grid.
// What differs, each with its reason:
//   vec      a unit takes 16-byte loads only where EVERY column of its group (the limbs in use, and the weight column if there
//            is one) is 16-byte aligned and the group has a whole unit: one bit per group, not per column, because a lane forms
//            its four keys from the same four rows of every column and a mixed unit would need both code paths per limb.
//   acc64    no weight column in the whole call: 32-bit counters straight into `out`, which sum(len) <= 2^31 - 2 keeps
//            canonical, exactly as above.  Any weight column: 64-bit accumulators for every group of the call (sum(len) rows of
//            weight < 2^32 stay below 2^63), kept in a scratch of 8 bytes per bin from the library's allocator, and a second
//            kernel reduces them mod P into out[place(k)].  The scratch is allocated before anything is zeroed or launched: a
//            table too large for it fails the call with the allocator's error (TSTWO_ERR_HIP, "hipMalloc ...") and `out` untouched.
//   LDS      a 64-bit histogram has half the bins in the same 64 KiB: the weighted LDS branch ends at 2^13 bins
//            (kLookupKeyedLdsMaxLog64).  Taking more than 64 KiB would leave one workgroup of 1024 lanes per CU (160 KiB),
//            half the waves, for the one table size 2^14; that trade has not been measured, so the occupancy argument above
//            is kept and 2^14 weighted bins go to the global branch.
//   combine  before a wave adds, lanes that hold the key of the wave's first pending lane are peeled off: their weights are summed
//            into that lane and they drop out (readlane + compare + ballot + a masked wave sum, only when more than one lane
//            matches).  At most `combine` such rounds per row of the unit; then every lane that still holds a weight issues its
//            own add, all in ONE atomic instruction, so peeling never turns one 64-lane instruction into several 1-lane ones.
//            GLOBAL: kLookupKeyedCombineGlobal = 8 rounds, because equal keys serialise on one word of memory (88 adds per us:
//            95 ms for 2^23 equal values).  2 x 2^22 rows into 2^16 bins, HIP events, median of 10, bounds 0 / 2 / 4 / 8: all
//            rows equal 95.2 / 1.59 / 1.58 / 1.60 ms, half the rows equal 47.7 / 12.7 / 4.32 / 1.80 ms (a wave whose first
//            `combine` pending lanes all miss the common key adds it lane by lane: one wave in 2^combine), uniform keys
//            434 / 432 / 403 / 438 us, which is what two runs of one library differ by.  More than 8 was not measured.
//            (Every one of these, bound 0 included, was 62 to 86 us behind the parent's old entry in the same runs: about 40 us
//            of that because the keyed path was always the one timed right after the host path, and some 20 us per call,
//            in LDS and on the global branch alike, whose cause was not found.  The rounds are not that gap.  DESIGN.md 4.10 (a)
//            has the comparison with the order of the paths drawn per round.)
//            LDS: kLookupKeyedCombineLds = 0.  A ds_add whose lanes collide costs 1.3 to 1.7 times the uniform time; 4 rounds
//            bring all-equal rows from 190 to 133 us (2^8 bins) and 199 to 139 us (2^14) but cost uniform keys 111 -> 194 and
//            149 -> 250 us, and uniform keys decide.  (profiles/bench_lookup_keyed.jsonl; DESIGN.md 4.10 has the table.)
constexpr uint32_t kLookupMaxGroups = 64, kLookupMaxLimbs = 4;
constexpr uint32_t kLookupKeyedLdsMaxLog32 = kLookupLdsMaxLog;           // 2^14 counters of 4 bytes = 64 KiB
constexpr uint32_t kLookupKeyedLdsMaxLog64 = kLookupLdsMaxLog - 1;       // 2^13 accumulators of 8 bytes = 64 KiB
constexpr uint32_t kLookupKeyedCombineGlobal = 8, kLookupKeyedCombineLds = 0;

struct LookupKeyedGroup {           // one tstwo_lookup_group with its device addresses as integers (0 = NULL)
    uint64_t limbs[kLookupMaxLimbs];
    uint32_t bits[kLookupMaxLimbs];
    uint32_t n_limbs;
    uint64_t weight;
    size_t len;
};

struct LookupKeyedPlan {
    LookupPlan::Branch branch;
    bool acc64;                     // 64-bit accumulators in a scratch and the reducing kernel; else 32-bit counters in `out`
    uint32_t threads;
    uint32_t grid_x, grid_y;        // grid_x = 0: no row at all, nothing is launched (the entry only zeroes)
    uint64_t wrap;                  // rows of one group per pass of the grid at its cap
    uint64_t vec;                   // bit g: group g takes 16-byte loads for its whole units
    uint32_t combine;               // peeling rounds per row before the atomic
};

// Returns the reason (the text behind "lookup: ") for an input without a plan.
inline const char *lookup_keyed_plan(const LookupKeyedGroup *groups, size_t n_groups, uint32_t log_range, uint32_t order,
                                     LookupKeyedPlan &p) {
    p = {};
    if (log_range < 1 || log_range > kLookupMaxLog) return "log_range must be 1 to 28";
    if (n_groups < 1 || n_groups > kLookupMaxGroups) return "1 to 64 groups";
    if (order > 1) return "order must be 0 (natural) or 1 (coset)";
    uint64_t total = 0, max_units = 0;
    for (size_t g = 0; g < n_groups; g++) {
        const LookupKeyedGroup &G = groups[g];
        if (G.n_limbs < 1 || G.n_limbs > kLookupMaxLimbs) return "1 to 4 limbs per group";
        uint64_t sum = 0;
        bool aligned = G.weight % 16 == 0;                   // 0 (no weight column) counts as aligned
        for (uint32_t j = 0; j < G.n_limbs; j++) {
            if (G.bits[j] < 1) return "every limb needs at least 1 bit";
            if (!G.limbs[j]) return "null device pointer among the limbs";
            sum += G.bits[j];
            aligned = aligned && G.limbs[j] % 16 == 0;
        }
        if (sum != log_range) return "the bits of every group must add up to log_range";
        if (G.len > kLookupMaxValues) return "more than 2^31 - 2 rows";
        total += G.len;
        const uint64_t units = ((uint64_t)G.len + kLookupUnit - 1) / kLookupUnit;
        if (units > max_units) max_units = units;
        if (aligned && G.len >= kLookupUnit) p.vec |= 1ull << g;
        if (G.weight) p.acc64 = true;
    }
    if (total > kLookupMaxValues) return "more than 2^31 - 2 rows";
    const bool lds = log_range <= (p.acc64 ? kLookupKeyedLdsMaxLog64 : kLookupKeyedLdsMaxLog32);
    p.branch = lds ? LookupPlan::LDS : LookupPlan::GLOBAL;
    p.threads = lds ? kLookupLdsThreads : kLookupGlobalThreads;
    p.combine = lds ? kLookupKeyedCombineLds : kLookupKeyedCombineGlobal;
    const uint32_t cap = (lds ? kLookupLdsCap : kLookupGlobalCap) / (uint32_t)n_groups;
    const uint32_t cap_x = cap ? cap : 1;
    p.wrap = (uint64_t)cap_x * p.threads * kLookupUnit;
    const uint64_t need = (max_units + p.threads - 1) / p.threads;
    p.grid_x = (uint32_t)(need < cap_x ? need : cap_x);
    p.grid_y = (uint32_t)n_groups;
    return nullptr;
}

}  // namespace tstwo

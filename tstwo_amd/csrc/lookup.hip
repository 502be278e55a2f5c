// lookup.hip — the multiplicity column of a lookup table, counted on the device (the host version is
// constraint_framework.range_check_multiplicities; tstwo_amd/logup.py lookup_multiplicities drives this one).
//
// tstwo_lookup_multiplicities: out[place(k)] = the number of words equal to k over all columns, a histogram of M31 columns into a
// column of 2^log_range words.  place is the identity (natural order: an MLE, the numerators of a GKR LogUpMultiplicities layer)
// or coset_pos (the storage order of a trace column on CanonicCoset(log_range), coset_order.cuh).  The launch comes from
// lookup_plan.h: one launch for all columns, the column on blockIdx.y, lanes striding over units of 4 words.
//   k_lookup<true, .>   the table fits LDS: a private histogram per workgroup (ds_add_u32), flushed bin by bin, non-zero bins only
//   k_lookup<false, .>  one global atomic add per value
// Counters are 32-bit integers, so the result does not depend on the order of arrival.  A word is compared with the range before
// it indexes anything; words outside are counted per lane and leave as one add per wave into *n_rejected.
// The column table (address, length, vec bit) travels through the small-upload ring and is read with scalar loads.
//
// tstwo_coset_iota: out[coset_pos(k)] = k, written position by position through the inverse map (coalesced stores).
#include <string>

#include "common.h"
#include "coset_order.cuh"
#include "lookup_plan.h"

using namespace tstwo;

namespace {

static_assert(kLookupMaxCols == TSTWO_LOOKUP_MAX_COLS && kLookupMaxLog == TSTWO_LOOKUP_MAX_LOG, "lookup_plan.h restates the header's limits");
static_assert(kLookupUnit == 4, "a unit is one 16-byte load");

// column descriptor as uploaded (u32 words): address (u64), length, vec
constexpr u32 kColWords = 4;
static_assert(kLookupMaxCols * kColWords * 4 <= kUpSlotBytes, "the column table must fit one upload slot");

typedef const u32 __attribute__((address_space(4))) *k32;
typedef const unsigned long long __attribute__((address_space(4))) *k64;

struct LookupArgs {
    const u32 *table;                // grid_y descriptors of kColWords
    u32 *out;                        // 2^log_range words, zeroed before the launch
    u32 *n_rejected;                 // zeroed before the launch, or nullptr
    u32 log_range;
};

template <bool COSET>
__device__ __forceinline__ u32 place(u32 k, u32 log_range) {
    if constexpr (COSET) return coset_pos(k, log_range - 1);
    else return k;
}

// the lane's units of its column, from unit u on, `stride` units apart: count(word) for every word
template <class F>
__device__ __forceinline__ void each_word(const u32 *col, u32 len, bool vec, u32 u, u32 stride, F count) {
    const u32 units = (len + kLookupUnit - 1) / kLookupUnit;           // len <= 2^31 - 2: 4 u < 2^31 + 4
    for (; u < units; u += stride) {
        const u32 w = u * kLookupUnit;
        if (vec && len - w >= kLookupUnit) {
            const uint4 v = gload4(col + w);
            count(v.x); count(v.y); count(v.z); count(v.w);
        } else {
            const u32 end = min(len, w + kLookupUnit);
            for (u32 i = w; i < end; i++) count(gload1(col + i));
        }
    }
}

__device__ __forceinline__ void add_rejected(u32 *n_rejected, u32 mine) {
    if (!n_rejected) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if (mine && (threadIdx.x & 63u) == 0) atomicAdd(n_rejected, mine);
}

template <bool LDS, bool COSET>
__global__ void __launch_bounds__(LDS ? kLookupLdsThreads : kLookupGlobalThreads) k_lookup(LookupArgs a) {
    constexpr u32 T = LDS ? kLookupLdsThreads : kLookupGlobalThreads;
    const u32 base = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.y * kColWords));
    const u32 *col = (const u32 *)((k64)a.table)[base >> 1];
    const u32 len = ((k32)a.table)[base + 2];
    const bool vec = ((k32)a.table)[base + 3] != 0;
    const u32 units = (len + kLookupUnit - 1) / kLookupUnit;
    if (blockIdx.x * T >= units) return;                               // the whole workgroup: a column shorter than the longest
    const u32 range = 1u << a.log_range;
    const u32 u0 = blockIdx.x * T + threadIdx.x, stride = gridDim.x * T;
    u32 rejected = 0;
    if constexpr (LDS) {
        __shared__ u32 hist[1u << kLookupLdsMaxLog];
        for (u32 i = threadIdx.x; i < range; i += T) hist[i] = 0;
        __syncthreads();
        each_word(col, len, vec, u0, stride, [&](u32 v) {
            if (v < range) atomicAdd(&hist[v], 1u);
            else rejected++;
        });
        __syncthreads();
        for (u32 i = threadIdx.x; i < range; i += T) {
            const u32 c = hist[i];
            if (c) atomicAdd(&a.out[place<COSET>(i, a.log_range)], c);
        }
    } else {
        each_word(col, len, vec, u0, stride, [&](u32 v) {
            if (v < range) atomicAdd(&a.out[place<COSET>(v, a.log_range)], 1u);
            else rejected++;
        });
    }
    add_rejected(a.n_rejected, rejected);
}

__global__ void __launch_bounds__(256) k_coset_iota(u32 *out, u32 log_size) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p < (1u << log_size)) gstore1(out, p, coset_row(p, log_size - 1));
}

int bad(const std::string &msg) { return set_error(TSTWO_ERR_BAD_ARG, "lookup: " + msg); }

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace

extern "C" {

int tstwo_lookup_multiplicities(const u32 *const *cols, const size_t *lens, size_t n_cols, u32 log_range, u32 order, u32 *out,
                                u32 *n_rejected) {
    TSTWO_REQUIRE_READY();
    if (!cols || !lens) return bad("null host argument");
    if (!out) return bad("null device pointer");
    if (n_cols < 1 || n_cols > kLookupMaxCols) return bad("1 to 64 columns");
    uint64_t addrs[kLookupMaxCols];
    for (size_t c = 0; c < n_cols; c++) {
        if (!cols[c]) return bad("null device pointer in the column table");
        addrs[c] = (uint64_t)(uintptr_t)cols[c];
    }
    LookupPlan plan;
    if (const char *why = lookup_plan(addrs, lens, n_cols, log_range, order, plan)) return bad(why);
    const size_t out_bytes = sizeof(u32) << log_range;
    for (size_t c = 0; c < n_cols; c++)
        if (cols[c] == out || overlap(cols[c], lens[c] * sizeof(u32), out, out_bytes)) return bad("out is one of the columns");
    if (n_rejected && overlap(n_rejected, sizeof(u32), out, out_bytes)) return bad("n_rejected lies inside out");
    // the column table travels through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the column table cannot be recorded)");
    TSTWO_HIP(hipMemsetAsync(out, 0, out_bytes, ctx().stream));
    if (n_rejected) TSTWO_HIP(hipMemsetAsync(n_rejected, 0, sizeof(u32), ctx().stream));
    if (plan.grid_x == 0) return TSTWO_OK;
    u32 staged[kLookupMaxCols * kColWords] = {};
    for (size_t c = 0; c < n_cols; c++) {
        u32 *w = staged + c * kColWords;
        w[0] = (u32)addrs[c];
        w[1] = (u32)(addrs[c] >> 32);
        w[2] = (u32)lens[c];
        w[3] = (u32)((plan.vec >> c) & 1u);
    }
    const size_t bytes = n_cols * kColWords * sizeof(u32);
    if (int rc = ensure_scratch(bytes)) return rc;
    if (int rc = small_h2d(ctx().scratch, staged, bytes)) return rc;
    LookupArgs a = {ctx().scratch, out, n_rejected, log_range};
    const dim3 grid(plan.grid_x, plan.grid_y), block(plan.threads);
    const bool coset = order == TSTWO_LOOKUP_ORDER_COSET;
    if (plan.branch == LookupPlan::LDS) {
        if (coset) hipLaunchKernelGGL((k_lookup<true, true>), grid, block, 0, ctx().stream, a);
        else hipLaunchKernelGGL((k_lookup<true, false>), grid, block, 0, ctx().stream, a);
    } else {
        if (coset) hipLaunchKernelGGL((k_lookup<false, true>), grid, block, 0, ctx().stream, a);
        else hipLaunchKernelGGL((k_lookup<false, false>), grid, block, 0, ctx().stream, a);
    }
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_coset_iota(u32 *out, u32 log_size) {
    TSTWO_REQUIRE_READY();
    if (!out) return bad("null device pointer");
    if (log_size < 1 || log_size > kLookupMaxLog) return bad("log_size must be 1 to 28");
    // a table column is built once, beside its multiplicities: like them it stays out of a recorded graph
    if (stream_is_capturing()) return bad("coset_iota during graph capture");
    hipLaunchKernelGGL(k_coset_iota, dim3(ceil_div((size_t)1 << log_size, 256)), dim3(256), 0, ctx().stream, out, log_size);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // extern "C"

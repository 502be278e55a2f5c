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
// tstwo_lookup_multiplicities_keyed: the same column where a key is joined from up to 4 limb columns, each limb checked against
// its own width before the limbs are joined, and a row adds its word of a weight column (0: the row is skipped unchecked).
//   k_lookup_keyed<LDS, W64, .>  W64 = false (no weight column in the call): 32-bit counters, into `out` as above;
//                                W64 = true: 64-bit accumulators (ds_add_u64 / global_atomic_add_x2) in a scratch, bin k at word k
//   k_lookup_keyed_reduce        out[p] = the accumulator of the bin stored at p, mod P
// Before a wave adds, lanes with the key of its first pending lane are summed into that lane (combine_equal_keys, the number
// of rounds from the plan).  Every device write is a vector store or a vector atomic.
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

// ---------------------------------------------------------------- keyed and weighted (tstwo_lookup_multiplicities_keyed)
// group descriptor as uploaded (u32 words): 4 limb addresses (u64), the weight address (u64, 0 = none), length,
// n_limbs | vec << 8, the limbs' bit widths and their shifts (one byte each), 2 words of padding
constexpr u32 kGroupWords = 16;
static_assert(kLookupMaxGroups == TSTWO_LOOKUP_MAX_GROUPS && kLookupMaxLimbs == TSTWO_LOOKUP_MAX_LIMBS, "lookup_plan.h restates the header's limits");
static_assert(kLookupMaxGroups * kGroupWords * 4 <= kUpSlotBytes, "the group table must fit one upload slot");

typedef unsigned long long u64acc;

struct KeyedArgs {
    const u32 *table;                // grid_y descriptors of kGroupWords
    void *acc;                       // W64: 2^log_range u64 accumulators (bin k at word k); else `out`; zeroed before the launch
    u32 *n_rejected;                 // zeroed before the launch, or nullptr
    u32 log_range;
    u32 combine;                     // peeling rounds per row (lookup_plan.h)
};

__device__ __forceinline__ u32 wave_sum(u32 x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// the sum of 64 weights of 32 bits (< 2^38); every lane of the wave calls it
__device__ __forceinline__ u64acc wave_sum_weights(u32 x) {
    if (!__ballot(x >> 26)) return wave_sum(x);                         // 64 words below 2^26: the sum fits a word
    return (u64acc)wave_sum(x & 0xFFFFu) + ((u64acc)wave_sum(x >> 16) << 16);
}

// What this lane adds to bin `key` after at most `rounds` rounds of peeling.  A round takes the wave's first pending lane (weight
// non-zero, not yet looked at), sums the weights of the pending lanes with ITS key into it and zeroes theirs.  w == 0 is a lane
// without a row to count (past the end, weight 0, rejected): never pending, so it neither leads nor joins a sum.  The whole wave
// must call this together.  ACC = u32: every pending lane weighs 1 and the sum is the number of matching lanes.
template <class ACC>
__device__ __forceinline__ ACC combine_equal_keys(u32 key, u32 w, u32 rounds, u32 lane) {
    ACC mine = w;
    bool pending = w != 0;
    for (u32 r = 0; r < rounds; r++) {
        const unsigned long long live = __ballot(pending);
        if (!live) break;
        const u32 first = (u32)__builtin_ctzll(live);
        const u32 lead = (u32)__builtin_amdgcn_readlane((int)key, (int)first);
        const bool match = pending && key == lead;
        const unsigned long long m = __ballot(match);
        if (__popcll(m) > 1) {
            ACC sum;
            if constexpr (sizeof(ACC) == 4) sum = (ACC)__popcll(m);
            else sum = wave_sum_weights(match ? w : 0u);
            mine = lane == first ? sum : match ? (ACC)0 : mine;
        }
        pending = pending && !match;
    }
    return mine;
}

__device__ __forceinline__ u32 reduce_m31(u64acc x) {                   // x < 2^63
    const u64acc s = (x & M31_P) + (x >> 31);                           // < 2^31 + 2^32
    u32 t = (u32)(s & M31_P) + (u32)(s >> 31);                          // < 2^31 + 3
    return t >= M31_P ? t - M31_P : t;
}

template <class ACC, u32 BINS>
__device__ __forceinline__ ACC *lds_histogram() {
    static_assert(sizeof(ACC) * BINS == 65536, "64 KiB: two workgroups of 1024 lanes per CU (lookup_plan.h)");
    __shared__ ACC hist[BINS];
    return hist;
}

template <bool LDS, bool W64, bool COSET>
__global__ void __launch_bounds__(LDS ? kLookupLdsThreads : kLookupGlobalThreads) k_lookup_keyed(KeyedArgs a) {
    constexpr u32 T = LDS ? kLookupLdsThreads : kLookupGlobalThreads;
    using acc_t = std::conditional_t<W64, u64acc, u32>;
    const u32 base = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.y * kGroupWords));
    const k64 t64 = (k64)a.table + (base >> 1);
    const k32 t32 = (k32)a.table + base;
    // every word of the descriptor is read here, once: a scalar load inside the loop over units would wait on lgkmcnt, the
    // counter the LDS adds of the units before it are still counted on
    const u32 *const limb[kLookupMaxLimbs] = {(const u32 *)t64[0], (const u32 *)t64[1], (const u32 *)t64[2], (const u32 *)t64[3]};
    const u32 *wcol = (const u32 *)t64[4];
    const u32 len = t32[10], flags = t32[11], bits_w = t32[12], shift_w = t32[13];
    const u32 n_limbs = flags & 7u;
    const bool vec = (flags >> 8) != 0;
    const u32 units = (len + kLookupUnit - 1) / kLookupUnit;
    if (blockIdx.x * T >= units) return;                               // the whole workgroup: a group shorter than the longest
    const u32 lane = threadIdx.x & 63u, stride = gridDim.x * T;
    acc_t *const acc = (acc_t *)a.acc;
    acc_t *hist = nullptr;
    const u32 range = 1u << a.log_range;
    if constexpr (LDS) {
        hist = lds_histogram<acc_t, 1u << (W64 ? kLookupKeyedLdsMaxLog64 : kLookupKeyedLdsMaxLog32)>();
        for (u32 i = threadIdx.x; i < range; i += T) hist[i] = 0;
        __syncthreads();
    }
    u32 rejected = 0;
    // ub, the unit of the wave's lane 0, is the same in every lane: the wave stays whole inside the loop (the rounds above use
    // ballots, readlane and shuffles), and a lane whose own unit lies past the end has rows = 0
    for (u32 ub = blockIdx.x * T + (threadIdx.x & ~63u); ub < units; ub += stride) {
        const u32 u = ub + lane;
        const u32 w0 = u * kLookupUnit;                                 // u < 2^29 + 64
        const u32 rows = u < units ? min(kLookupUnit, len - w0) : 0u;
        const bool whole = vec && rows == kLookupUnit;
        u32 wt[kLookupUnit], key[kLookupUnit] = {0, 0, 0, 0}, bad = 0;
        if (wcol) {
            if (whole) {
                const uint4 v = gload4(wcol + w0);
                wt[0] = v.x; wt[1] = v.y; wt[2] = v.z; wt[3] = v.w;
            } else {
#pragma unroll
                for (u32 i = 0; i < kLookupUnit; i++) wt[i] = i < rows ? gload1(wcol + w0 + i) : 0u;
            }
        } else {
#pragma unroll
            for (u32 i = 0; i < kLookupUnit; i++) wt[i] = i < rows ? 1u : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < kLookupMaxLimbs; j++) {
            if (j >= n_limbs) break;                                    // wave-uniform
            const u32 *col = limb[j];
            const u32 bits = (bits_w >> (8 * j)) & 0xFFu, shift = (shift_w >> (8 * j)) & 0xFFu;
            u32 v[kLookupUnit];
            if (whole) {
                const uint4 q = gload4(col + w0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (u32 i = 0; i < kLookupUnit; i++) v[i] = i < rows ? gload1(col + w0 + i) : 0u;
            }
#pragma unroll
            for (u32 i = 0; i < kLookupUnit; i++) {
                bad |= ((v[i] >> bits) != 0u ? 1u : 0u) << i;           // bits <= 28
                key[i] |= (v[i] & ((1u << bits) - 1u)) << shift;        // masked: a key is below the range whatever the limb holds
            }
        }
#pragma unroll
        for (u32 i = 0; i < kLookupUnit; i++) {
            if (wt[i] != 0u && ((bad >> i) & 1u)) {                     // weight 0 comes first: such a row is not checked at all
                rejected++;
                wt[i] = 0;
            }
            const acc_t add = combine_equal_keys<acc_t>(key[i], wt[i], a.combine, lane);
            if (add != 0) {
                if constexpr (LDS) atomicAdd(&hist[key[i]], add);
                else if constexpr (W64) atomicAdd(&acc[key[i]], add);
                else atomicAdd(&acc[place<COSET>(key[i], a.log_range)], add);
            }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (u32 i = threadIdx.x; i < range; i += T) {
            const acc_t c = hist[i];
            if (c != 0) atomicAdd(&acc[W64 ? i : place<COSET>(i, a.log_range)], c);
        }
    }
    add_rejected(a.n_rejected, rejected);
}

// out[p] = the accumulator of the bin stored at position p, mod P (coalesced stores through the inverse map, as k_coset_iota)
template <bool COSET>
__global__ void __launch_bounds__(256) k_lookup_keyed_reduce(const u64acc *acc, u32 *out, u32 log_range) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (1u << log_range)) return;
    const u32 k = COSET ? coset_row(p, log_range - 1) : p;
    gstore1(out, p, reduce_m31(acc[k]));
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

int tstwo_lookup_multiplicities_keyed(const tstwo_lookup_group *groups, size_t n_groups, u32 log_range, u32 order, u32 *out,
                                      u32 *n_rejected) {
    TSTWO_REQUIRE_READY();
    if (!groups) return bad("null host argument");
    if (!out) return bad("null device pointer");
    if (n_groups < 1 || n_groups > kLookupMaxGroups) return bad("1 to 64 groups");
    LookupKeyedGroup gs[kLookupMaxGroups];
    for (size_t g = 0; g < n_groups; g++) {
        LookupKeyedGroup &G = gs[g];
        G = {};
        G.n_limbs = groups[g].n_limbs;
        for (u32 j = 0; j < kLookupMaxLimbs; j++) {
            G.limbs[j] = (uint64_t)(uintptr_t)groups[g].limbs[j];
            G.bits[j] = groups[g].bits[j];
        }
        G.weight = (uint64_t)(uintptr_t)groups[g].weight;
        G.len = groups[g].len;
    }
    LookupKeyedPlan plan;
    if (const char *why = lookup_keyed_plan(gs, n_groups, log_range, order, plan)) return bad(why);
    const size_t out_bytes = sizeof(u32) << log_range;
    for (size_t g = 0; g < n_groups; g++) {
        const size_t col_bytes = gs[g].len * sizeof(u32);
        for (u32 j = 0; j <= gs[g].n_limbs; j++) {                       // the limbs in use, then the weight column
            const void *col = j < gs[g].n_limbs ? groups[g].limbs[j] : groups[g].weight;
            if (col && (col == out || overlap(col, col_bytes, out, out_bytes))) return bad("out overlaps a limb or weight column");
        }
    }
    if (n_rejected && overlap(n_rejected, sizeof(u32), out, out_bytes)) return bad("n_rejected lies inside out");
    // the group table travels through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the group table cannot be recorded)");
    const bool coset = order == TSTWO_LOOKUP_ORDER_COSET;
    if (plan.grid_x == 0) {
        TSTWO_HIP(hipMemsetAsync(out, 0, out_bytes, ctx().stream));
        if (n_rejected) TSTWO_HIP(hipMemsetAsync(n_rejected, 0, sizeof(u32), ctx().stream));
        return TSTWO_OK;
    }
    const size_t bytes = n_groups * kGroupWords * sizeof(u32);
    if (int rc = ensure_scratch(bytes)) return rc;
    void *acc = out;
    if (plan.acc64) {                                                   // before anything is zeroed: a failure leaves `out` as it was
        if (int rc = tstwo_malloc(&acc, sizeof(u64acc) << log_range)) return rc;
    }
    // everything below is enqueued on the one stream, so the block may go back to the allocator before the kernels have run
    struct Release { void *p; ~Release() { if (p) (void)tstwo_free(p); } } release = {plan.acc64 ? acc : nullptr};
    TSTWO_HIP(hipMemsetAsync(acc, 0, (plan.acc64 ? sizeof(u64acc) : sizeof(u32)) << log_range, ctx().stream));
    if (n_rejected) TSTWO_HIP(hipMemsetAsync(n_rejected, 0, sizeof(u32), ctx().stream));
    u32 staged[kLookupMaxGroups * kGroupWords] = {};
    for (size_t g = 0; g < n_groups; g++) {
        u32 *w = staged + g * kGroupWords;
        u32 shift = 0;
        for (u32 j = 0; j < gs[g].n_limbs; j++) {
            w[2 * j] = (u32)gs[g].limbs[j];
            w[2 * j + 1] = (u32)(gs[g].limbs[j] >> 32);
            w[12] |= gs[g].bits[j] << (8 * j);
            w[13] |= shift << (8 * j);
            shift += gs[g].bits[j];
        }
        w[8] = (u32)gs[g].weight;
        w[9] = (u32)(gs[g].weight >> 32);
        w[10] = (u32)gs[g].len;
        w[11] = gs[g].n_limbs | (u32)((plan.vec >> g) & 1u) << 8;
    }
    if (int rc = small_h2d(ctx().scratch, staged, bytes)) return rc;
    KeyedArgs a = {ctx().scratch, acc, n_rejected, log_range, plan.combine};
    const dim3 grid(plan.grid_x, plan.grid_y), block(plan.threads);
    const bool lds = plan.branch == LookupPlan::LDS;
    if (plan.acc64) {
        if (lds) hipLaunchKernelGGL((k_lookup_keyed<true, true, false>), grid, block, 0, ctx().stream, a);
        else hipLaunchKernelGGL((k_lookup_keyed<false, true, false>), grid, block, 0, ctx().stream, a);
        TSTWO_LAUNCH_CHECK();
        const dim3 rgrid(ceil_div((size_t)1 << log_range, 256));
        if (coset) hipLaunchKernelGGL(k_lookup_keyed_reduce<true>, rgrid, dim3(256), 0, ctx().stream, (const u64acc *)acc, out, log_range);
        else hipLaunchKernelGGL(k_lookup_keyed_reduce<false>, rgrid, dim3(256), 0, ctx().stream, (const u64acc *)acc, out, log_range);
    } else if (lds) {
        if (coset) hipLaunchKernelGGL((k_lookup_keyed<true, false, true>), grid, block, 0, ctx().stream, a);
        else hipLaunchKernelGGL((k_lookup_keyed<true, false, false>), grid, block, 0, ctx().stream, a);
    } else {
        if (coset) hipLaunchKernelGGL((k_lookup_keyed<false, false, true>), grid, block, 0, ctx().stream, a);
        else hipLaunchKernelGGL((k_lookup_keyed<false, false, false>), grid, block, 0, ctx().stream, a);
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

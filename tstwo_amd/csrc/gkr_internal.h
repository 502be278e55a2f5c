// gkr_internal.h — what the three GKR translation units share: gkr_ops.hip (the streaming ops), gkr_transcript.hip (the
// single-wave transcript kernels) and gkr_prove.hip (the one-call driver, which enqueues the launchers of the other two).
#pragma once
#include "common.h"

namespace tstwo {

constexpr unsigned kMaxSumBlocks = 1024;     // slab = kMaxSumBlocks x 8 words
constexpr u32 kMaxLog = 28;                  // word offsets of gload*/gstore* stay below 2^30
// gkr scratch layout (context scratch, >= 1 MiB): ticket word | result words (no result page) | slab | eq tables
constexpr size_t kTicketOff = 0, kResultOff = 256, kSlabOff = 1024, kTabOff = kSlabOff + kMaxSumBlocks * 8 * 4;
constexpr u32 kStatusDegenerate = 1u;        // the status word: an eq point at which the host path divides by zero

inline bool dev_scalar_ok(const void *p) { return p && aligned16(p); }

__device__ __forceinline__ qm31 q_of(uint4 v) { return {v.x, v.y, v.z, v.w}; }
// foldMleEvals (lookups/utils.ts:256): eval0 + r (eval1 - eval0)
__device__ __forceinline__ qm31 fold_q(qm31 r, qm31 lhs, qm31 rhs) { return qm31_add(lhs, qm31_mul(r, qm31_sub(rhs, lhs))); }
// A protocol scalar of a kernel: the argument `v`, or (dev non-null: it wins) the 4 device words at `dev` (16-byte aligned) that
// an earlier launch on the stream left there.  The same for every lane: one load, then scalar registers, so a kernel keeps the
// register budget it has with the scalar by value.
__device__ __forceinline__ qm31 scalar_q(qm31 v, const u32 *dev) {
    if (!dev) return v;
    const uint4 w = gload4(dev);
    return {(u32)__builtin_amdgcn_readfirstlane((int)w.x), (u32)__builtin_amdgcn_readfirstlane((int)w.y),
            (u32)__builtin_amdgcn_readfirstlane((int)w.z), (u32)__builtin_amdgcn_readfirstlane((int)w.w)};
}

#define TSTWO_INTERNAL __attribute__((visibility("hidden")))
// ---- gkr_ops.hip: checks + launches.  A scalar is host words or, where those are null, 4 device words.
// One sum (fold: the fused round, which first folds by r / r_dev); `out` = 8 device-visible words.
TSTWO_INTERNAL int gkr_sum(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const onum[4],
                           u32 *const oden[4], u32 n_vars, const u32 r[4], const u32 *r_dev, const u32 lambda[4], const u32 *lambda_dev,
                           u32 *out, bool fold);
// One fold; base: in[0] is the one M31 column.
TSTWO_INTERNAL int mle_fold(bool base, const u32 *const in[4], u32 log_n, const u32 r[4], const u32 *r_dev, u32 *const out[4]);
// The eq table of the n_y coordinates at y (4 words each) times v: all of them host words, or (dev) all of them device words.
TSTWO_INTERNAL int eq_evals(const u32 *y, u32 n_y, const u32 *v, bool dev, u32 *const out[4]);
// next_layer of a checked layer of log_n >= 1 variables; num / onum as far as the kind has them (base numerators: num[0])
TSTWO_INTERNAL int launch_next_layer(u32 kind, const u32 *const num[4], const u32 *const den[4], u32 log_n, u32 *const onum[4], u32 *const oden[4]);
// ---- gkr_transcript.hip
// dev: y, a, alpha are device words and a degenerate y sets a bit of *status; else host words, a degenerate y is refused, status is null
TSTWO_INTERNAL int round_finish(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 *y, const u32 *a,
                                const u32 *alpha, bool dev, u32 *round_poly_out, u32 *challenge_out, u32 *status);
TSTWO_INTERNAL int layer_begin(u32 *chan, const tstwo_gkr_lane *lanes, u32 n, const u32 *claims, u32 *out_claims, u32 *state, u32 *scalars,
                               const u32 *y_dev, u32 n_y, u32 *inv, u32 *status);
TSTWO_INTERNAL int layer_end(u32 *chan, const tstwo_gkr_lane *lanes, u32 n, u32 *masks, u32 *claims, u32 *ch_out);

}  // namespace tstwo

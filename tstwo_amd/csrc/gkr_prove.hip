// gkr_prove.hip — prove_batch in one call (gkr_prover.ts:440-580): the schedule of gkr_plan.h with every protocol scalar left in
// device words.  The ops of gkr_ops.hip read y, v, lambda and the challenges from memory, and the single-wave kernels of
// gkr_transcript.hip do what the host does around and between a layer's sum-check rounds, so that the whole proof is enqueued
// without a read-back and one block comes back at the end.
#include <vector>

#include "gkr_internal.h"
#include "gkr_plan.h"

using namespace tstwo;

namespace {

// One instance's layer as the kernels see it: 4 numerator pointers (a base column repeats its one pointer; null without
// numerators) and 4 denominator pointers.
struct LayerView {
    u32 kind;
    u32 *num[4], *den[4];
};
// generated layer k of instance p inside the pool: all LogUp kinds generate LogUpGeneric layers (numerators, then denominators)
LayerView generated_layer(u32 *pool, const GkrPlanInst &p, u32 k) {
    LayerView v{};
    v.kind = p.kind == kGkrGrandProduct ? kGkrGrandProduct : kGkrGeneric;
    u32 *base = pool + gkr_layer_off(p, k);
    const uint64_t w = gkr_col_words(k);
    for (int c = 0; c < 4; c++) {
        v.num[c] = p.gen_cols == 8 ? base + c * w : nullptr;
        v.den[c] = base + (p.gen_cols == 8 ? 4 + c : c) * w;
    }
    return v;
}
LayerView input_layer(const tstwo_gkr_instance &in) {
    LayerView v{};
    v.kind = in.kind;
    for (int c = 0; c < 4; c++) {
        // never written: the plan folds an input into the instance's own buffers (GKR_FOLD_NEW)
        v.num[c] = in.kind == kGkrGeneric ? (u32 *)in.num[c] : in.kind == kGkrMultiplicities ? (u32 *)in.num[0] : nullptr;
        v.den[c] = (u32 *)in.den[c];
    }
    return v;
}
void fill_lane_ptrs(const u32 *(&dst)[8], const LayerView &v) {
    for (int c = 0; c < 4; c++) { dst[c] = v.num[c]; dst[4 + c] = v.den[c]; }
}

int plan_of(const tstwo_gkr_instance *instances, size_t n, GkrPlan &pl) {
    if (n && !instances) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    u32 kinds[kGkrMaxInstances], logs[kGkrMaxInstances];
    for (size_t i = 0; i < n && i < kGkrMaxInstances; i++) { kinds[i] = instances[i].kind; logs[i] = instances[i].log_n; }
    if (const char *why = gkr_plan(kinds, logs, n, pl)) return set_error(TSTWO_ERR_BAD_ARG, why);
    return TSTWO_OK;
}

// Everything the call allocated goes back to the allocator on every way out, behind a synchronisation (launches may be in flight).
struct ProveBuffers {
    void *pool = nullptr, *block = nullptr, *lanes = nullptr;
    ~ProveBuffers() {
        (void)hipStreamSynchronize(ctx().stream);
        for (void *p : {pool, block, lanes}) if (p) tstwo_free(p);
    }
};

int prove_batch_run(const u32 chan[10], const tstwo_gkr_instance *instances, const GkrPlan &pl, u32 *block_host) {
    const u32 n = pl.n_inst, n_layers = pl.n_layers;
    ProveBuffers mem;
    if (int rc = tstwo_malloc(&mem.pool, pl.pool_words * 4)) return rc;
    if (int rc = tstwo_malloc(&mem.block, (size_t)pl.block_words * 4)) return rc;
    size_t n_lanes_total = 0;
    for (const GkrPlanLayer &l : pl.layers) n_lanes_total += l.n_active;
    if (int rc = tstwo_malloc(&mem.lanes, n_lanes_total * sizeof(tstwo_gkr_lane))) return rc;
    if (int rc = ensure_scratch(kTabOff + ((size_t)2 << (kMaxLog / 2 + 1)) * sizeof(qm31))) return rc;
    u32 *const pool = (u32 *)mem.pool, *const blk = (u32 *)mem.block;
    hipStream_t st = ctx().stream;

    // the layers of every instance: [0 .. log_n) generated, [log_n] the caller's
    std::vector<std::vector<LayerView>> lay(n);
    u32 widest = 0;                                      // an instance with n_layers variables: its dead layers hold the eq tables
    for (u32 i = 0; i < n; i++) {
        const GkrPlanInst &p = pl.inst[i];
        for (u32 k = 0; k < p.log_n; k++) lay[i].push_back(generated_layer(pool, p, k));
        lay[i].push_back(input_layer(instances[i]));
        if (p.log_n == n_layers && pl.inst[widest].log_n != n_layers) widest = i;
        for (u32 k = p.log_n; k >= 1; k--) {
            const LayerView &in = lay[i][k], &out = lay[i][k - 1];
            if (int rc = launch_next_layer(in.kind, in.num, in.den, k, out.num, out.den)) return rc;
        }
    }
    TSTWO_HIP(hipMemsetAsync(blk, 0, (size_t)pl.block_words * 4, st));
    TSTWO_HIP(hipMemcpyAsync(blk + pl.chan_off, chan, 10 * sizeof(u32), hipMemcpyHostToDevice, st));

    // the lanes of every layer, known before anything runs: where each mask will lie once the layer's folds are done
    std::vector<tstwo_gkr_lane> lanes(n_lanes_total);
    std::vector<size_t> lane0(n_layers);
    {
        size_t at = 0;
        for (u32 L = 0; L < n_layers; L++) {
            lane0[L] = at;
            for (u32 i = 0; i < n; i++) {
                const GkrPlanInst &p = pl.inst[i];
                const int n_v = gkr_n_v(p, L);
                if (n_v < 0) continue;
                tstwo_gkr_lane &ln = lanes[at++];
                ln = tstwo_gkr_lane{};
                const bool input = (u32)n_v + 1 == p.log_n;
                // the reduced layer ends as 2 points: in place for a generated layer, in the dead layer below for an input that
                // was folded (n_v >= 1), the input itself where it has one variable
                const LayerView &src = input && n_v >= 1 ? lay[i][p.log_n - 1] : lay[i][n_v + 1];
                const u32 kind = input ? (p.kind == kGkrMultiplicities ? kGkrGeneric : p.kind) : src.kind;
                fill_lane_ptrs(ln.src, src);
                ln.inst = i; ln.kind = kind; ln.shift = L - (u32)n_v; ln.enter = n_v == 0;
                fill_lane_ptrs(ln.out_src, lay[i][0]);
            }
        }
    }
    TSTWO_HIP(hipMemcpyAsync(mem.lanes, lanes.data(), n_lanes_total * sizeof(tstwo_gkr_lane), hipMemcpyHostToDevice, st));
    const tstwo_gkr_lane *lanes_dev = (const tstwo_gkr_lane *)mem.lanes;

    u32 *const status = blk + pl.status_off, *const chan_dev = blk + pl.chan_off;
    for (u32 L = 0; L < n_layers; L++) {
        const GkrPlanLayer &gl = pl.layers[L];
        u32 *const ood_cur = blk + pl.ood_off[L & 1], *const ood_next = blk + pl.ood_off[(L + 1) & 1];
        const tstwo_gkr_lane *ld = lanes_dev + lane0[L];
        if (int rc = layer_begin(chan_dev, ld, gl.n_active, blk + pl.ctv_off, blk + pl.out_off, blk + pl.state_off, blk + pl.alpha_off, ood_cur,
                                 L, blk + pl.inv_off, status))
            return rc;
        // EqEvals.generate(ood): eq((0, x), y) = genEqEvals(y[1:], 1 - y[0]), into the widest instance's dead layer of L - 1 variables
        const LayerView eqv = L ? lay[widest][L - 1] : LayerView{};
        if (L)
            if (int rc = eq_evals(ood_cur + 4, L - 1, blk + pl.eqv_off, true, eqv.den)) return rc;
        // per lane: the layer being reduced, and the challenge not yet applied to it
        struct Cur { LayerView v; u32 n_vars; const u32 *pending; u32 inst; };
        std::vector<Cur> cur;
        for (u32 j = 0; j < gl.n_active; j++) {
            const u32 i = lanes[lane0[L] + j].inst;
            const u32 n_v = (u32)gkr_n_v(pl.inst[i], L);
            cur.push_back({lay[i][n_v + 1], n_v + 1, nullptr, i});
        }
        auto target = [&](const Cur &c, GkrFold how) {
            return how == GKR_FOLD_IN_PLACE ? c.v : lay[c.inst][pl.inst[c.inst].log_n - 1];
        };
        for (u32 rnd = 0; rnd < L; rnd++) {
            const u32 rem = L - rnd;
            const uint64_t mask = gkr_round_lanes(pl, L, rem);
            for (u32 j = 0; j < gl.n_active; j++) {
                if (!((mask >> j) & 1)) continue;
                Cur &c = cur[j];
                const GkrFold how = gkr_round_fold(pl, pl.inst[c.inst], L, rem);
                u32 *const slot = blk + pl.sums_off + 8 * j;
                if (how == GKR_NO_FOLD) {
                    if (int rc = gkr_sum(c.v.kind, eqv.den, c.v.num, c.v.den, nullptr, nullptr, rem, nullptr, nullptr, nullptr, blk + pl.lambda_off,
                                         slot, false))
                        return rc;
                } else {
                    const LayerView to = target(c, how);
                    if (int rc = gkr_sum(c.v.kind, eqv.den, c.v.num, c.v.den, to.num, to.den, rem, nullptr, c.pending, nullptr, blk + pl.lambda_off,
                                         slot, true))
                        return rc;
                    const bool had_num = c.v.kind == kGkrGeneric || c.v.kind == kGkrMultiplicities;
                    const u32 kind = c.v.kind == kGkrMultiplicities ? kGkrGeneric : c.v.kind;
                    c.v = to;
                    c.v.kind = kind;
                    if (!had_num) for (int k = 0; k < 4; k++) c.v.num[k] = nullptr;
                    c.n_vars--;
                }
                c.pending = ood_next + 4 * rnd;              // the challenge this round is about to draw
            }
            if (int rc = round_finish(chan_dev, blk + pl.sums_off, blk + pl.state_off, gl.n_active, mask, ood_cur + 4 * rnd, blk + pl.inv_off + 4 * rnd,
                                      blk + pl.alpha_off, true, blk + gl.poly_off + 20 * rnd, ood_next + 4 * rnd, status))
                return rc;
        }
        // the last challenge of the layer: a plain fold leaves the 2-point layer the mask is read from
        for (Cur &c : cur) {
            if (!c.pending) continue;
            const LayerView to = target(c, gkr_last_fold(pl, pl.inst[c.inst], L));
            if (c.v.kind == kGkrGeneric || c.v.kind == kGkrMultiplicities)
                if (int rc = mle_fold(c.v.kind == kGkrMultiplicities, c.v.num, c.n_vars, nullptr, c.pending, to.num)) return rc;
            if (int rc = mle_fold(false, c.v.den, c.n_vars, nullptr, c.pending, to.den)) return rc;
        }
        if (int rc = layer_end(chan_dev, ld, gl.n_active, blk + gl.mask_off, blk + pl.ctv_off, ood_next + 4 * L)) return rc;
    }
    TSTWO_HIP(hipMemcpyAsync(block_host, blk, (size_t)pl.block_words * 4, hipMemcpyDeviceToHost, st));
    TSTWO_HIP(hipStreamSynchronize(st));
    if (block_host[pl.status_off] & kStatusDegenerate) return set_error(TSTWO_ERR_BAD_ARG, "sum-check: degenerate eq point");
    return TSTWO_OK;
}

}  // namespace

extern "C" {

int tstwo_gkr_prove_batch_words(const tstwo_gkr_instance *instances, size_t n_instances, size_t *block_words) {
    if (!block_words) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    GkrPlan pl;
    if (int rc = plan_of(instances, n_instances, pl)) return rc;
    *block_words = pl.block_words;
    return TSTWO_OK;
}

int tstwo_gkr_prove_batch(const u32 chan[10], const tstwo_gkr_instance *instances, size_t n_instances, u32 *block, size_t block_words) {
    TSTWO_REQUIRE_READY();
    if (!chan || !block) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    GkrPlan pl;
    if (int rc = plan_of(instances, n_instances, pl)) return rc;
    if (block_words < pl.block_words) return set_error(TSTWO_ERR_BAD_ARG, "prove_batch: the block is too small (tstwo_gkr_prove_batch_words)");
    for (size_t i = 0; i < n_instances; i++) {
        const tstwo_gkr_instance &in = instances[i];
        const int n_num = in.kind == kGkrGeneric ? 4 : in.kind == kGkrMultiplicities ? 1 : 0;
        TSTWO_REQUIRE_TABLE(in.den, 4);
        TSTWO_REQUIRE_TABLE(in.num, (size_t)n_num);
        for (int c = 0; c < 4; c++)
            if (((uintptr_t)in.den[c] & 3) || (c < n_num && ((uintptr_t)in.num[c] & 3)))
                return set_error(TSTWO_ERR_BAD_ARG, "prove_batch: misaligned device pointer");
    }
    if (stream_is_capturing()) return set_error(TSTWO_ERR_BAD_ARG, "prove_batch during graph capture (it reads its result back)");
    return prove_batch_run(chan, instances, pl, block);
}

}  // extern "C"

// gkr_plan.h — the whole schedule of tstwo_gkr_prove_batch for a batch of (kind, log_n) instances, made before anything is
// enqueued (host only: no HIP, no context).  tests/gkr_plan.py restates this in Python; tests/test_cpu_gkr_plan.py compiles this
// header and compares.
//
// Instance i has log_n layers the prover generates (k = 0 .. log_n - 1 variables, k = 0 the output layer) below the caller's input
// (log_n variables).  The proof has n_layers = max log_n GKR layers; instance i enters at layer first = n_layers - log_n and at
// layer L >= first its oracle has n_v = L - first variables and reduces its layer of n_v + 1 variables.  Layer L has L sum-check
// rounds (rem = L .. 1 variables left); an instance takes part in the rounds with rem <= n_v.  The active instances of a layer, in
// instance order, are the LANES of the transcript kernels and of tstwo_gkr_round_finish_dev (sumcheck.ts batches exactly those).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tstwo {

constexpr uint32_t kGkrMaxInstances = 64, kGkrMaxLog = 28;
constexpr uint32_t kGkrGrandProduct = 0, kGkrGeneric = 1, kGkrMultiplicities = 2, kGkrSingles = 3;

// How an instance's layer gets its first variable fixed in a round (or behind the last round of a layer).
enum GkrFold : uint32_t {
    GKR_NO_FOLD,            // its first round of the layer: the sum alone
    GKR_FOLD_IN_PLACE,      // a layer the prover owns, secure columns
    GKR_FOLD_NEW,           // the caller's input (never written): into the buffers of the instance's dead layer of log_n - 1 variables
    GKR_FOLD_NEW_BASE       // the same, base numerators (they become secure: LogUpMultiplicities turns LogUpGeneric)
};

struct GkrPlanInst {
    uint32_t kind, log_n, first;
    uint32_t gen_cols;      // columns of a generated layer: 4 (grand product) or 8 (numerators, then denominators)
    uint64_t gen_off;       // word offset of the instance's generated layers in the pool
};
struct GkrPlanLayer {
    uint32_t n_rounds, n_active;
    uint64_t enter, active;             // bit i = INSTANCE i enters at / is active in this layer
    uint32_t poly_off, mask_off;        // block words: 20 per round; 16 per lane
};
struct GkrPlan {
    uint32_t n_inst = 0, n_layers = 0;
    std::vector<GkrPlanInst> inst;
    std::vector<GkrPlanLayer> layers;
    // word offsets in the block (all multiples of 4).  Per instance, 8 words each: state and sums by LANE, ctv and out by INSTANCE.
    uint32_t chan_off = 0, status_off = 16, alpha_off = 20, lambda_off = 24, eqv_off = 28;
    uint32_t state_off = 32, sums_off = 0, ctv_off = 0, out_off = 0, ood_off[2] = {0, 0}, inv_off = 0, final_ood = 0, block_words = 0;
    uint64_t pool_words = 0;            // every generated layer of every instance
};

// a column of a generated layer of k variables occupies this many words (16-byte aligned columns)
inline uint64_t gkr_col_words(uint32_t k) { return k < 2 ? 4 : 1ull << k; }
// word offset of generated layer k inside the pool; column c follows at c * gkr_col_words(k)
inline uint64_t gkr_layer_off(const GkrPlanInst &p, uint32_t k) {
    const uint64_t cols_before = k <= 2 ? 4ull * k : (1ull << k) + 4;
    return p.gen_off + p.gen_cols * cols_before;
}
// variables of instance p's oracle at layer L (negative: not entered yet)
inline int gkr_n_v(const GkrPlanInst &p, uint32_t L) { return (int)L - (int)p.first; }
// fold number f (0-based) of the layer instance p reduces at layer L
inline GkrFold gkr_fold_kind(const GkrPlan &pl, const GkrPlanInst &p, uint32_t L, uint32_t f) {
    const bool input = L + 1 == pl.n_layers;              // n_v + 1 == log_n: only the last layer reduces the caller's layers
    if (!input || f) return GKR_FOLD_IN_PLACE;
    return p.kind == kGkrMultiplicities ? GKR_FOLD_NEW_BASE : GKR_FOLD_NEW;
}
// what round `rem` of layer L does to instance p's layer (p takes part: 1 <= rem <= n_v)
inline GkrFold gkr_round_fold(const GkrPlan &pl, const GkrPlanInst &p, uint32_t L, uint32_t rem) {
    const uint32_t n_v = (uint32_t)gkr_n_v(p, L);
    return rem == n_v ? GKR_NO_FOLD : gkr_fold_kind(pl, p, L, n_v - rem - 1);
}
// the fold behind the last round: fold number n_v - 1
inline GkrFold gkr_last_fold(const GkrPlan &pl, const GkrPlanInst &p, uint32_t L) { return gkr_fold_kind(pl, p, L, (uint32_t)gkr_n_v(p, L) - 1); }
// lanes (bit j = the j-th active instance of layer L) that take part in round `rem`
inline uint64_t gkr_round_lanes(const GkrPlan &pl, uint32_t L, uint32_t rem) {
    uint64_t m = 0;
    uint32_t lane = 0;
    for (const GkrPlanInst &p : pl.inst) {
        const int n_v = gkr_n_v(p, L);
        if (n_v < 0) continue;
        if ((uint32_t)n_v >= rem) m |= 1ull << lane;
        lane++;
    }
    return m;
}

// Returns the reason (a TSTWO_ERR_BAD_ARG) for a batch that has no schedule.
inline const char *gkr_plan(const uint32_t *kinds, const uint32_t *log_ns, size_t n, GkrPlan &pl) {
    pl = GkrPlan{};
    if (n == 0) return "no instances";
    if (n > kGkrMaxInstances) return "prove_batch: 1 to 64 instances";
    uint32_t n_layers = 0;
    for (size_t i = 0; i < n; i++) {
        if (kinds[i] > kGkrSingles) return "unknown GKR layer kind";
        if (log_ns[i] == 0) return "Some output claims were not set during proving (an input layer of 0 variables is an output layer)";
        if (log_ns[i] > kGkrMaxLog) return "GKR layer too large";
        if (kinds[i] == kGkrMultiplicities && log_ns[i] == 1) return "LogUpMultiplicities should never reach tryIntoMask";
        if (log_ns[i] > n_layers) n_layers = log_ns[i];
    }
    pl.n_inst = (uint32_t)n;
    pl.n_layers = n_layers;
    uint64_t pool = 0;
    for (size_t i = 0; i < n; i++) {
        GkrPlanInst p{kinds[i], log_ns[i], n_layers - log_ns[i], kinds[i] == kGkrGrandProduct ? 4u : 8u, pool};
        pool = gkr_layer_off(p, p.log_n);
        pl.inst.push_back(p);
    }
    pl.pool_words = pool;
    const uint32_t n8 = 8 * pl.n_inst, l4 = 4 * n_layers;
    pl.sums_off = pl.state_off + n8;
    pl.ctv_off = pl.sums_off + n8;
    pl.out_off = pl.ctv_off + n8;
    pl.ood_off[0] = pl.out_off + n8;
    pl.ood_off[1] = pl.ood_off[0] + l4;
    pl.inv_off = pl.ood_off[1] + l4;
    pl.final_ood = pl.ood_off[n_layers & 1];               // layer L reads point L & 1 (L coordinates) and writes point (L + 1) & 1
    uint32_t off = pl.inv_off + l4;
    for (uint32_t L = 0; L < n_layers; L++) {
        GkrPlanLayer lay{L, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < n; i++) {
            const int n_v = gkr_n_v(pl.inst[i], L);
            if (n_v < 0) continue;
            lay.active |= 1ull << i;
            if (n_v == 0) lay.enter |= 1ull << i;
            lay.n_active++;
        }
        lay.poly_off = off;
        lay.mask_off = off + 20 * L;
        off = lay.mask_off + 16 * lay.n_active;
        pl.layers.push_back(lay);
    }
    pl.block_words = off;
    return nullptr;
}

}  // namespace tstwo

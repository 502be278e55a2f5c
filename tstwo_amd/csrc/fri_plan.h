// fri_plan.h — which launches tstwo_fri_commit_layers takes for an input (host only: no HIP, no context).
// tests/fri_plan.py restates this in Python; tests/test_cpu_fri_plan.py compiles this header and compares.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tstwo {

// Line layer i has 2^(col_logs[0] - 1 - i) rows: layer 0 is the fold of circle column 0, the last one has 2^log_last_layer_size.
// Alpha entry k is the k-th felt the channel draws: entry 0 behind the first-layer tree, entry i + 1 behind layer i's tree.
struct FriStep {
    enum Kind {
        FIRST_TREE,             // one tree over every circle column's coordinate columns (log: column 0's); draws alpha_out = 0
        CIRCLE_WRITE,           // circle column 0 -> layer 0, written, not accumulated; reads alpha_in = 0
        COMMIT,                 // layer -> its tree; draws alpha_out = layer + 1
        FOLD_COMMIT,            // layer - 1 folded into layer inside the leaf launch of layer's tree; reads alpha_in = layer, draws layer + 1
        FOLD_LINE,              // layer - 1 folded into layer; reads alpha_in = layer
        CIRCLE_ACCUM,           // circle column folded into layer with the alpha that folded into it; reads alpha_in = layer
        TAIL                    // one workgroup: trees of layer .. layer + n_layers - 1 and the folds between and behind them; draws
    } kind;                     // alpha_out = layer + 1 onwards; pre: it first folds layer - 1 into layer, reading alpha_in = layer
    uint32_t layer, log;        // the layer the step writes or commits (TAIL: its first) and that layer's log size
    uint32_t column;            // CIRCLE_*: the circle column read
    uint32_t alpha_in, alpha_out;
    uint32_t n_layers;          // TAIL
    bool pre;                   // TAIL
};
constexpr uint32_t kFriTailLog = 9;          // k_fri_tail holds layers of at most 2^9 rows

// The steps of a commit, in launch order.  Returns the reason (a TSTWO_ERR_BAD_ARG) and no steps for an input that has no schedule.
// fused = false is the schedule of tstwo_fri_commit_layers_poseidon252: FOLD_COMMIT and TAIL hash Blake2s leaves inside the fold, so
// a commit over Poseidon trees takes the unfused kinds only — every layer above the last is a COMMIT, every fold a FOLD_LINE.
inline const char *fri_plan(const uint32_t *col_logs, size_t n_columns, uint32_t log_last_layer_size, std::vector<FriStep> &steps,
                            bool fused = true) {
    steps.clear();
    if (!n_columns) return "no columns";
    for (size_t i = 0; i < n_columns; i++) {
        if (col_logs[i] < 3 || col_logs[i] > 31) return "fri commit: circle evaluations of log size 3..31";
        if (i && col_logs[i - 1] <= col_logs[i]) return "column sizes not decreasing";
    }
    const uint32_t last = log_last_layer_size;
    uint32_t layer = 0, log = col_logs[0] - 1;          // CIRCLE_TO_LINE_FOLD_STEP = 1
    if (last > log) return "fri commit: last layer larger than the first line layer";
    steps.push_back({FriStep::FIRST_TREE, 0, col_logs[0], 0, 0, 0, 0, false});
    steps.push_back({FriStep::CIRCLE_WRITE, 0, log, 0, 0, 0, 0, false});
    size_t nxt = 1;                                     // the next circle column to join
    bool committed = false;                             // the fold that produced `layer` hashed it into its tree already
    while (log > last) {
        // every remaining layer fits one workgroup's LDS and no column is left: one launch does tree / mix / draw / fold for all of them
        if (fused && !committed && log <= kFriTailLog && nxt == n_columns) {
            steps.push_back({FriStep::TAIL, layer, log, 0, 0, layer + 1, log - last, false});
            break;
        }
        if (!committed) steps.push_back({FriStep::COMMIT, layer, log, 0, 0, layer + 1, 0, false});
        committed = false;
        layer++, log--;
        const bool joins = nxt < n_columns && col_logs[nxt] - 1 == log;
        const bool tail_next = log <= kFriTailLog && nxt + (joins ? 1 : 0) == n_columns;
        if (log == last || joins || !fused) {          // never committed, or not complete before the column is in
            steps.push_back({FriStep::FOLD_LINE, layer, log, 0, layer, 0, 0, false});
        } else if (tail_next) {                         // the tail launch folds the layer on its way in
            steps.push_back({FriStep::TAIL, layer, log, 0, layer, layer + 1, log - last, true});
            break;
        } else {                                        // committed as it stands: the folded row is its tree's leaf message
            steps.push_back({FriStep::FOLD_COMMIT, layer, log, 0, layer, layer + 1, 0, false});
            committed = true;
        }
        if (joins) steps.push_back({FriStep::CIRCLE_ACCUM, layer, log, (uint32_t)nxt++, layer, 0, 0, false});
    }
    if (nxt != n_columns) {                             // Rust: assert!(columns.is_empty())
        steps.clear();
        return "not all columns were consumed";
    }
    return nullptr;
}

}  // namespace tstwo

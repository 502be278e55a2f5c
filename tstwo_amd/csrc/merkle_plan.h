// merkle_plan.h — which launches the Blake2s Merkle entries take for an input (host only: no HIP, no context): tstwo_merkle_commit
// (merkle_plan_tree, also the tree of a FRI commit layer with its fold and channel hook), tstwo_merkle_commit_layer
// (merkle_plan_layer) and tstwo_merkle_commit_many (merkle_plan_set).  merkle.hip walks the steps; nothing is launched before the
// whole plan stands.  tests/merkle_plan.py restates this in Python; tests/test_cpu_merkle_plan.py compiles this header and compares.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tstwo {

constexpr int kUpLog = 16;                   // layers below 2^kUpLog nodes are latency-bound: a quad of lanes per node, several levels per launch
constexpr int kMaxTrees = 8;                 // equally shaped trees per launch (blockIdx.y)
constexpr int kMerkleMaxHashCols = 256;      // common.h: kMaxHashCols, columns absorbed per launch (multiple of 16)
constexpr int kMerkleCapDefault = 32;        // common.h: Knobs::merkle_cap
constexpr int kMerklePairLogDefault = 19;    // common.h: Knobs::merkle_pair_log

// What the plan reads besides the input: Context::n_cus, Knobs::merkle_cap, Knobs::merkle_pair_log.
struct MerkleEnv { uint32_t n_cus; int cap, pair_log; };

struct MerkleLayerWords {                    // the LayerParams of one k_merkle_layer launch
    uint32_t total_words, w_begin, w_end, col_word0, n_cols, load_state, is_final;
};

struct MerkleStep {
    enum Kind {
        LEAF_STATIC,            // k_merkle_leaf_static<n_cols / 16>: layer log from n_cols columns per tree
        LEAF_PAIR,              // k_merkle_leaf_pair<n_cols / 16>: layers log and log - 1, a lane per pair of sibling leaves
        LEAF4,                  // k_merkle_leaf4: layer log from 4 columns
        LEAF4_UPQ,              // k_merkle_leaf4_upq<wg>: layer log from 4 columns and `levels` levels above it
        LAYER,                  // k_merkle_layer<has_prev>: layer log from columns [col0, col0 + n_cols) of its own, message words per lp
        INNER,                  // k_merkle_inner: layer log from its children
        INNER_SET,              // k_merkle_inner_set: the same for every tree of a set
        SUBTREE2C,              // k_merkle_subtree2c: layers log - 1 and log - 2 from the children at layer log
        UPQ,                    // k_merkle_upq<wg>: layers log - 1 .. log - levels from the children at layer log
        CHANNEL                 // k_channel_mix_draw on the root: a hook that no launch of the tree could take
    } kind;
    uint32_t log;               // the layer written; SUBTREE2C, UPQ: the layer read (log_child)
    uint32_t levels;            // LEAF4_UPQ, UPQ
    uint32_t wg, grid;          // lanes per workgroup (256 or 1024; CHANNEL: 64); workgroups per tree, the cap of merkle_layer_blocks applied
    uint32_t tree, n_trees;     // the trees covered (blockIdx.y): [tree, tree + n_trees) of the call
    uint32_t col0, n_cols;      // LEAF_*, LAYER: the columns read, counted among the columns of log size `log` in table order
    bool has_prev;              // LAYER
    bool fold, hook;            // the launch first writes its 4 columns as the fold; it takes the channel step on the root
    MerkleLayerWords lp;        // LAYER
};

// reasons; all but the fold's are a TSTWO_ERR_BAD_ARG
constexpr const char *kMerkleFoldNotCarried = "fri commit: the fold was not carried by the leaf launch";      // TSTWO_ERR_HIP

// Workgroups of a one-lane-per-node launch over n_nodes nodes of each of n_trees trees: at most `cap` per CU, then lanes grid-stride
// over more nodes; a set of trees has the same lanes in flight as one tree's launch.
inline uint32_t merkle_layer_blocks(size_t n_nodes, uint32_t n_trees, const MerkleEnv &env) {
    const uint32_t blocks = (uint32_t)((n_nodes + 255) / 256);
    const uint32_t cap = env.n_cus * (uint32_t)env.cap / n_trees;
    return blocks <= cap ? blocks : cap ? cap : 1;
}

// Whether the leaf layer of 16 / 32 / 48 / 64-column trees is hashed together with the layer above it (LEAF_PAIR): from 2^pair_log
// leaves up (below that a tree is a handful of latency-bound launches and the static leaf keeps its lane per row), when layer
// log - 1 has no columns of its own and every leaf column is 8-byte aligned (the kernel's loads fetch two words; a column at an odd
// word offset keeps the static leaf, which needs 4-byte alignment only).
inline bool merkle_leaf_takes_pair(uint32_t log, bool columns_below, bool cols_aligned8, const MerkleEnv &env) {
    return log >= 1 && log <= 30 && (int)log >= env.pair_log && !columns_below && cols_aligned8;
}

inline MerkleStep merkle_step(MerkleStep::Kind kind, uint32_t log, uint32_t grid, uint32_t wg, uint32_t tree, uint32_t n_trees) {
    MerkleStep s = {};
    s.kind = kind, s.log = log, s.grid = grid, s.wg = wg, s.tree = tree, s.n_trees = n_trees;
    return s;
}

// Column-free levels log_child - 1 .. log_stop below 2^kUpLog nodes, a few fused launches instead of one launch per level.  *hook:
// a channel step is on offer; the launch that produces the root of a single tree (log_stop = 0: one workgroup) takes it.
inline void merkle_plan_upper(uint32_t tree, uint32_t n_trees, uint32_t log_child, uint32_t log_stop, bool *hook, std::vector<MerkleStep> &steps) {
    bool root_hook = false;
    if (hook && *hook && n_trees == 1 && log_stop == 0 && log_child > log_stop) {
        root_hook = true;
        *hook = false;
    }
    while (log_child > log_stop) {
        const uint32_t remaining = log_child - log_stop, parents_log = log_child - 1;
        MerkleStep s = merkle_step(MerkleStep::UPQ, log_child, 1, 256, tree, n_trees);
        if (parents_log >= 9 && remaining >= 9 && remaining <= 16) {
            // 256 quads per workgroup, 9 levels each, FIRST: the wide levels (256 and 128 compressions on one CU are the slow
            // part of a single-workgroup tree top) run on 2^(parents_log-8) CUs side by side, and what is left (<= 7 levels)
            // fits one 64-quad workgroup, one wave per SIMD.  (The other order — 64-quad workgroups first, one 256-quad
            // workgroup to finish — put those wide levels on one CU.)
            s.wg = 1024, s.grid = 1u << (parents_log - 8), s.levels = 9;
        } else if (parents_log <= 6) {            // <= 64 parents: one 64-quad workgroup finishes the run
            s.levels = remaining, s.hook = root_hook;
        } else if (parents_log <= 8) {            // <= 256 parents: ONE workgroup of 256 quads finishes the run (up to 9 levels)
            s.wg = 1024, s.levels = remaining, s.hook = root_hook;
        } else {                                  // >= 512 parents: 64 quads per workgroup, 64 -> 1 = up to 7 levels each
            s.grid = 1u << (parents_log - 6), s.levels = remaining < 7 ? remaining : 7;
        }
        steps.push_back(s);
        log_child -= s.levels;
    }
}

// Column-free layers log_child - 1 .. log_stop of every tree of a set, the plan of every tree above its columns: layers of at
// least 2^kUpLog nodes two per launch (SUBTREE2C; measured for 32 x 2^22: 0.308 ms, against 0.313 for one launch per layer and
// 0.326 / 0.332 for runs of 3 / 4 layers), a single leftover one on its own, the smaller ones by merkle_plan_upper.
inline void merkle_plan_column_free(uint32_t tree, uint32_t n_trees, uint32_t log_child, uint32_t log_stop, bool *hook, const MerkleEnv &env,
                                    std::vector<MerkleStep> &steps) {
    for (; log_child >= log_stop + 2 && log_child - 2 >= (uint32_t)kUpLog; log_child -= 2)      // >= 2^kUpLog tops: whole workgroups of 256
        steps.push_back(merkle_step(MerkleStep::SUBTREE2C, log_child, (uint32_t)(((size_t)1 << (log_child - 2)) / 256), 256, tree, n_trees));
    if (log_child > log_stop && log_child - 1 >= (uint32_t)kUpLog) {
        log_child -= 1;
        steps.push_back(merkle_step(MerkleStep::INNER_SET, log_child, merkle_layer_blocks((size_t)1 << log_child, n_trees, env), 256, tree, n_trees));
    }
    merkle_plan_upper(tree, n_trees, log_child, log_stop, hook, steps);
}

// One layer of 2^log nodes from its children (has_prev) and n_cols columns of its own: appends its launches, or returns the reason
// there are none.  fold: the 4 columns of a leaf layer are first written as a fold, inside the leaf launch.
inline const char *merkle_plan_layer(uint32_t log, bool has_prev, size_t n_cols, bool fold, bool layers_aligned16, const MerkleEnv &env, uint32_t tree,
                                     std::vector<MerkleStep> &steps) {
    if (log > 31) return "merkle: log size out of range";
    if (!layers_aligned16) return "merkle: layers must be 16-byte aligned";
    if (fold && (has_prev || log > 30 || n_cols != 4)) return kMerkleFoldNotCarried;
    const uint32_t blocks = merkle_layer_blocks((size_t)1 << log, 1, env);
    MerkleStep s = merkle_step(MerkleStep::LAYER, log, blocks, 256, tree, 1);
    s.n_cols = (uint32_t)n_cols, s.has_prev = has_prev, s.fold = fold;
    if (has_prev ? n_cols == 0 : log <= 30 && (n_cols == 4 || n_cols == 16 || n_cols == 32 || n_cols == 48 || n_cols == 64)) {
        s.kind = has_prev ? MerkleStep::INNER : n_cols == 4 ? MerkleStep::LEAF4 : MerkleStep::LEAF_STATIC;
        steps.push_back(s);
        return nullptr;
    }
    // columns are absorbed kMaxHashCols per launch; launch boundaries fall on 64-byte block boundaries
    const uint32_t child_words = has_prev ? 16u : 0u, W = child_words + (uint32_t)n_cols;
    size_t col_base = 0;
    do {
        size_t take = n_cols - col_base;
        if (take > (size_t)kMerkleMaxHashCols) take = kMerkleMaxHashCols;
        const bool final_launch = col_base + take == n_cols;
        if (!final_launch) take -= (child_words + col_base + take) % 16;      // every launch but the last ends on a block boundary
        const bool first = col_base == 0;
        s.col0 = (uint32_t)col_base, s.n_cols = (uint32_t)take;
        s.lp.total_words = W;
        s.lp.w_begin = first ? 0u : (uint32_t)(child_words + col_base);
        s.lp.w_end = final_launch ? (W > 0 ? W : 1u) + 16u : (uint32_t)(child_words + col_base + take);
        s.lp.col_word0 = (uint32_t)(child_words + col_base);
        s.lp.n_cols = (uint32_t)take;
        s.lp.load_state = first ? 0u : 1u;
        s.lp.is_final = final_launch ? 1u : 0u;
        steps.push_back(s);
        col_base += take;
    } while (col_base < n_cols);
    return nullptr;
}

// One tree of tstwo_merkle_commit_many, or the one of tstwo_merkle_commit.
struct MerkleTree {
    const uint32_t *log_sizes;
    size_t n_cols;
    bool cols_aligned8;         // every column of the largest log size is 8-byte aligned
    bool layers_aligned16;
    bool null_arg;              // commit_many: a null layers buffer, column table or log size table
};

// Every launch of one tree, appended to `steps` in order (vcs/prover.ts:24-27: from the largest layer down), or the reason there is
// no plan.  fold: the tree's 4 columns are first written as a fold, inside the leaf launch; a launch sequence that cannot carry it is
// an error.  hook: a channel step on the root is on offer: the single-workgroup launch that produces the root takes it, and a
// trailing CHANNEL step does when no launch could.
inline const char *merkle_plan_tree(const MerkleTree &t, bool fold, bool hook, const MerkleEnv &env, uint32_t tree, std::vector<MerkleStep> &steps) {
    uint32_t count[32] = {}, max_log = 0;
    for (size_t i = 0; i < t.n_cols; i++) {
        if (t.log_sizes[i] > 31) return "merkle: log size out of range";
        count[t.log_sizes[i]]++;
        if (t.log_sizes[i] > max_log) max_log = t.log_sizes[i];
    }
    if (t.n_cols == 4 && max_log >= 1 && (int)max_log <= kUpLog && count[max_log] == 4) {
        // a tree of exactly 4 equally long columns with at most 2^kUpLog rows (every FRI layer but the first few): leaves and the
        // first 7 levels in one launch of 64-quad workgroups; up to 2^9 rows one workgroup of 256 quads takes the whole tree and the hook
        const bool whole = max_log <= 9;
        MerkleStep s = merkle_step(MerkleStep::LEAF4_UPQ, max_log, 1, whole ? 1024 : 256, tree, 1);
        s.levels = whole ? max_log : 7u, s.grid = 1u << (max_log - s.levels), s.n_cols = 4, s.fold = fold, s.hook = whole && hook;
        steps.push_back(s);
        if (whole) hook = false;
        else merkle_plan_upper(tree, 1, max_log - s.levels, 0, &hook, steps);
    } else {
        bool have_prev = false;
        for (int lg = (int)max_log; lg >= 0;) {
            const uint32_t k = count[lg];
            if (k == 0 && have_prev) {
                // a run of column-free layers below lg + 1: one plan for all of them (stop above the next layer that has columns)
                int stop = lg;
                while (stop > 0 && !count[stop - 1]) stop--;
                merkle_plan_column_free(tree, 1, (uint32_t)lg + 1, (uint32_t)stop, &hook, env, steps);
                lg = stop - 1;
                continue;
            }
            if (!have_prev && !fold && (k == 16 || k == 32 || k == 48 || k == 64) && t.layers_aligned16 &&
                merkle_leaf_takes_pair((uint32_t)lg, lg >= 1 && count[lg - 1], t.cols_aligned8, env)) {
                // the static leaf's shapes, with the column-free layer above the leaves riding on the leaf launch
                MerkleStep s = merkle_step(MerkleStep::LEAF_PAIR, (uint32_t)lg, merkle_layer_blocks((size_t)1 << (lg - 1), 1, env), 256, tree, 1);
                s.n_cols = k;
                steps.push_back(s);
                have_prev = true;
                lg -= 2;
                continue;
            }
            if (const char *why = merkle_plan_layer((uint32_t)lg, have_prev, k, fold && !have_prev, t.layers_aligned16, env, tree, steps)) return why;
            have_prev = true;
            lg--;
        }
    }
    if (hook) steps.push_back(merkle_step(MerkleStep::CHANNEL, 0, 1, 64, tree, 1));
    return nullptr;
}

// tstwo_merkle_commit_many shares every launch among the trees (blockIdx.y = tree) when they have ONE shape that the static leaf
// kernel serves: 2 to kMaxTrees trees of 16 / 32 / 48 / 64 columns, at most kMaxHashCols columns in all, of one log size in
// kUpLog + 1 .. 30, every layers buffer 16-byte aligned.  *log: that size.  Any other set is committed tree by tree.
inline const char *merkle_set_uniform(const MerkleTree *trees, size_t n_trees, bool *uniform, uint32_t *log) {
    bool u = n_trees >= 2 && n_trees <= (size_t)kMaxTrees;
    const size_t n_cols = n_trees ? trees[0].n_cols : 0;
    uint32_t lg = 0;
    for (size_t r = 0; r < n_trees && u; r++) {
        const MerkleTree &q = trees[r];
        if (q.null_arg) return "merkle: null argument";
        u = q.n_cols == n_cols && (n_cols == 16 || n_cols == 32 || n_cols == 48 || n_cols == 64) && n_cols * n_trees <= (size_t)kMerkleMaxHashCols &&
            q.layers_aligned16;
        for (size_t k = 0; k < q.n_cols && u; k++) {
            if (r == 0 && k == 0) lg = q.log_sizes[0];
            u = q.log_sizes[k] == lg;
        }
    }
    *uniform = u && lg >= (uint32_t)kUpLog + 1 && lg <= 30;
    *log = lg;
    return nullptr;
}

// The steps of tstwo_merkle_commit_many, in launch order, or the reason there is no plan (and no steps): a uniform set's launches
// cover all trees, the tails of the trees running side by side; the trees of any other set follow each other, each as
// merkle_plan_tree states it.
inline const char *merkle_plan_set(const MerkleTree *trees, size_t n_trees, const MerkleEnv &env, std::vector<MerkleStep> &steps) {
    steps.clear();
    bool uniform = false;
    uint32_t lg = 0;
    const char *why = merkle_set_uniform(trees, n_trees, &uniform, &lg);
    if (!why && uniform) {
        bool aligned8 = true;
        for (size_t r = 0; r < n_trees; r++) aligned8 = aligned8 && trees[r].cols_aligned8;
        const bool pair = merkle_leaf_takes_pair(lg, false, aligned8, env);      // one log size: no columns below the leaves
        const uint32_t top = pair ? lg - 1 : lg;                                 // the last layer the leaf launch writes
        MerkleStep s = merkle_step(pair ? MerkleStep::LEAF_PAIR : MerkleStep::LEAF_STATIC, lg, merkle_layer_blocks((size_t)1 << top, (uint32_t)n_trees, env),
                                   256, 0, (uint32_t)n_trees);
        s.n_cols = (uint32_t)trees[0].n_cols;
        steps.push_back(s);
        merkle_plan_column_free(0, (uint32_t)n_trees, top, 0, nullptr, env, steps);
    }
    for (size_t r = 0; r < n_trees && !why && !uniform; r++) why = merkle_plan_tree(trees[r], false, false, env, (uint32_t)r, steps);
    if (why) steps.clear();
    return why;
}

}  // namespace tstwo

// Prints the plan of csrc/merkle_plan.h, in the format of tests/merkle_plan.py::render, for every input line
// (tests/test_cpu_merkle_plan.py); "error: <reason>" for an input without a plan.  Every line starts "<kind> n_cus cap pair_log":
//   T fold hook aligned8 aligned16 LOG*COUNT ...                       one tree (tstwo_merkle_commit, the tree of a FRI commit layer)
//   L log has_prev n_cols aligned16                                    one layer (tstwo_merkle_commit_layer)
//   S | null_arg aligned8 aligned16 LOG*COUNT ... | ...                a set of trees (tstwo_merkle_commit_many)
//   C                                                                  the header's constants
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "merkle_plan.h"

using namespace tstwo;

static void read_logs(std::istringstream &in, std::vector<uint32_t> &logs) {      // up to the next "|" or the end of the line
    std::string w;
    while (in >> w && w != "|") {
        unsigned lg = 0, n = 0;
        if (std::sscanf(w.c_str(), "%u*%u", &lg, &n) == 2) logs.insert(logs.end(), n, lg);
    }
}

static void print(const std::vector<MerkleStep> &steps) {
    for (size_t i = 0; i < steps.size(); i++) {
        const MerkleStep &s = steps[i];
        const bool many = s.grid > 1;
        std::printf("%s", i ? " " : "");
        switch (s.kind) {
            case MerkleStep::LEAF_STATIC: std::printf("static%u(%u)", s.n_cols, s.log); break;
            case MerkleStep::LEAF_PAIR: std::printf("pair%u(%u)", s.n_cols, s.log); break;
            case MerkleStep::LEAF4: std::printf("leaf4(%u)", s.log); break;
            case MerkleStep::LEAF4_UPQ: std::printf("leaf4_upq<%u>(%u)", s.wg, s.log); break;
            case MerkleStep::INNER: std::printf("inner(%u)", s.log); break;
            case MerkleStep::INNER_SET: std::printf("inner_set(%u)", s.log); break;
            case MerkleStep::SUBTREE2C: std::printf("s2c(%u)", s.log); break;
            case MerkleStep::CHANNEL: std::printf("channel()"); break;
            case MerkleStep::UPQ:       // the four arms by their names in plan(): A and C have 256 quads per workgroup, B and C one workgroup
                if (s.wg == 1024 && many) std::printf("A(%u)", s.log);
                else std::printf("%c(%u,%u)", s.wg == 1024 ? 'C' : many ? 'D' : 'B', s.log, s.levels);
                break;
            case MerkleStep::LAYER: {   // xN: the launches of this layer; (log, the layer's columns)
                size_t a = i, b = i;
                while (a > 0 && steps[a - 1].kind == MerkleStep::LAYER && steps[a - 1].log == s.log && steps[a - 1].tree == s.tree) a--;
                while (b + 1 < steps.size() && steps[b + 1].kind == MerkleStep::LAYER && steps[b + 1].log == s.log && steps[b + 1].tree == s.tree) b++;
                std::printf("layer<%c>x%zu(%u,%u)", s.has_prev ? 'T' : 'F', b - a + 1, s.log, s.lp.total_words - (s.has_prev ? 16u : 0u));
                break;
            }
        }
        std::printf("[t%u,%ux%u,%u", s.tree, s.grid, s.n_trees, s.wg);
        if (s.kind == MerkleStep::UPQ || s.kind == MerkleStep::LEAF4_UPQ) std::printf(",lv%u", s.levels);
        if (s.kind == MerkleStep::LAYER)
            std::printf(",c%u+%u,lp%u:%u:%u:%u:%u:%u:%u", s.col0, s.n_cols, s.lp.total_words, s.lp.w_begin, s.lp.w_end, s.lp.col_word0, s.lp.n_cols,
                        s.lp.load_state, s.lp.is_final);
        std::printf("]%s%s", s.fold ? "+fold" : "", s.hook ? "+hook" : "");
    }
    std::printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        MerkleEnv env = {};
        if (!(in >> kind >> env.n_cus >> env.cap >> env.pair_log)) continue;
        std::vector<MerkleStep> steps;
        const char *why = nullptr;
        if (kind == "C") {
            std::printf("%d %d %d %d %d\n", kUpLog, kMaxTrees, kMerkleMaxHashCols, kMerkleCapDefault, kMerklePairLogDefault);
            continue;
        } else if (kind == "T") {
            int fold = 0, hook = 0, a8 = 0, a16 = 0;
            in >> fold >> hook >> a8 >> a16;
            std::vector<uint32_t> logs;
            read_logs(in, logs);
            const MerkleTree t = {logs.data(), logs.size(), a8 != 0, a16 != 0, false};
            why = merkle_plan_tree(t, fold != 0, hook != 0, env, 0, steps);
        } else if (kind == "L") {
            uint32_t log = 0, n_cols = 0;
            int has_prev = 0, a16 = 0;
            in >> log >> has_prev >> n_cols >> a16;
            why = merkle_plan_layer(log, has_prev != 0, n_cols, false, a16 != 0, env, 0, steps);
        } else {
            std::vector<std::vector<uint32_t>> logs;
            std::vector<MerkleTree> trees;
            std::string bar;
            int null_arg = 0, a8 = 0, a16 = 0;
            in >> bar;
            while (in >> null_arg >> a8 >> a16) {
                logs.emplace_back();
                read_logs(in, logs.back());
                trees.push_back({nullptr, logs.back().size(), a8 != 0, a16 != 0, null_arg != 0});
            }
            for (size_t r = 0; r < trees.size(); r++) trees[r].log_sizes = logs[r].data();
            why = merkle_plan_set(trees.data(), trees.size(), env, steps);
        }
        if (why) std::printf("error: %s\n", why);
        else print(steps);
    }
    return 0;
}

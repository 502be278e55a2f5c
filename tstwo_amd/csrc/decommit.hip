// decommit.hip — host-side proof assembly over device-resident trees and columns: the decommitment walk of MerkleProver.decommit
// (vcs/prover.ts:32-109), the query folding of FriProver.decommit_on_queries (fri.ts:346-384, 768-785) and the word gather that
// fetches what they select.  Nothing here hashes: the only kernel is k_gather_words.
#include <string.h>

#include <vector>

#include "common.h"

using namespace tstwo;

namespace {

struct GatherItem { const u32 *src; unsigned long long idx; };
__global__ void __launch_bounds__(256) k_gather_words(const GatherItem *__restrict__ items, u32 words, size_t total, u32 *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t item = i / words, w = i % words;
    out[i] = items[item].src[items[item].idx * words + w];
}

// One upload of the request items, one launch per record size (the first n_a items are records of words_a words, the n_b items
// behind them records of words_b words), one read-back of all words into host_out, in item order.  The gathers write straight
// into the result page when the words fit: the read-back is then a synchronisation, not a copy.
int gather_to_host(const GatherItem *items, size_t n_a, u32 words_a, size_t n_b, u32 words_b, void *host_out) {
    const size_t total_a = n_a * words_a, out_words = total_a + n_b * words_b;
    if (out_words == 0) return TSTWO_OK;
    Context &c = ctx();
    const size_t items_bytes = (((n_a + n_b) * sizeof(GatherItem) + 63) / 64) * 64;
    int rc = ensure_scratch(items_bytes + out_words * sizeof(u32));
    if (rc) return rc;
    rc = small_h2d(c.scratch, items, (n_a + n_b) * sizeof(GatherItem));     // stream-ordered behind whatever still reads the scratch
    if (rc) return rc;
    const GatherItem *d_items = (const GatherItem *)c.scratch;
    u32 *const page = (u32 *)result_target(out_words * sizeof(u32));
    u32 *d_out = page ? page : (u32 *)((unsigned char *)c.scratch + items_bytes);
    if (total_a) hipLaunchKernelGGL(k_gather_words, dim3(ceil_div(total_a, 256)), dim3(256), 0, c.stream, d_items, words_a, total_a, d_out);
    if (n_b) hipLaunchKernelGGL(k_gather_words, dim3(ceil_div(n_b * words_b, 256)), dim3(256), 0, c.stream, d_items + n_a, words_b, n_b * words_b, d_out + total_a);
    TSTWO_LAUNCH_CHECK();
    if (!page) return small_d2h(host_out, d_out, out_words * sizeof(u32));
    const void *view = nullptr;
    rc = result_wait(&view);
    if (rc) return rc;
    memcpy(host_out, view, out_words * sizeof(u32));
    return TSTWO_OK;
}

}  // namespace

namespace tstwo {
int download_roots(const uint8_t *const *layers, size_t n_trees, uint8_t *roots) {
    std::vector<GatherItem> items(n_trees);
    for (size_t r = 0; r < n_trees; r++) items[r] = {(const u32 *)layers[r], 0};
    return gather_to_host(items.data(), n_trees, 8u, 0, 0u, roots);
}
}  // namespace tstwo

extern "C" {

int tstwo_gather_words(const void *const *srcs, const uint64_t *idx, u32 words, size_t n_items, u32 *host_out) {
    TSTWO_REQUIRE_READY();
    if (n_items == 0 || words == 0) return TSTWO_OK;
    if (!srcs || !idx || !host_out) return set_error(TSTWO_ERR_BAD_ARG, "gather: null argument");
    std::vector<GatherItem> items(n_items);
    for (size_t i = 0; i < n_items; i++) items[i] = {(const u32 *)srcs[i], idx[i]};
    return gather_to_host(items.data(), n_items, words, 0, 0u, host_out);
}

// MerkleProver.decommit (vcs/prover.ts:32-109) against device-resident layers and columns: the walk over the layers
// (which nodes are visited, which child digests / column values the verifier cannot recompute) runs here on the host
// side of the library; the selected words are then fetched with two gathers.
struct DecommitLists {
    std::vector<GatherItem> hashes, queried, witness;      // (device base, element index); digests are 8 words, values 1
};
// The walk of one tree: appends its requests to the shared lists.
static int plan_decommit(const uint8_t *layers, u32 max_log, const u32 *const *cols, const u32 *col_log_sizes, size_t n_cols,
                         const u32 *query_logs, const uint64_t *const *queries, const size_t *n_queries, size_t n_query_sets,
                         DecommitLists &out) {
    if (!layers || (n_cols && (!cols || !col_log_sizes)) || (n_query_sets && (!query_logs || !queries || !n_queries)))
        return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: null argument");
    if (max_log > 31) return set_error(TSTWO_ERR_BAD_ARG, "merkle: log size out of range");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    for (size_t i = 0; i < n_cols; i++)
        if (col_log_sizes[i] > max_log) return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: column larger than the tree");
    std::vector<uint64_t> last, cur;
    for (int lg = (int)max_log; lg >= 0; lg--) {
        const uint64_t *direct = nullptr;
        size_t nd = 0;
        for (size_t k = 0; k < n_query_sets; k++)
            if (query_logs[k] == (u32)lg) { direct = queries[k]; nd = n_queries[k]; }
        if (nd && !direct) return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: null argument");
        for (size_t k = 0; k < nd; k++)
            if (direct[k] >> lg) return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: query position outside its layer");
        const bool has_child = (u32)lg < max_log;
        const u32 *child_layer = has_child ? (const u32 *)(layers + 32 * (((size_t)1 << (lg + 1)) - 1)) : nullptr;
        size_t pi = 0, di = 0;
        cur.clear();
        for (;;) {
            bool any = false;
            uint64_t node = 0;
            if (pi < last.size()) { node = last[pi] >> 1; any = true; }
            if (di < nd && (!any || direct[di] < node)) { node = direct[di]; any = true; }
            if (!any) break;
            if (has_child)
                for (uint64_t k = 2 * node; k <= 2 * node + 1; k++) {
                    if (pi < last.size() && last[pi] == k) pi++;
                    else out.hashes.push_back({child_layer, k});
                }
            const bool queried = di < nd && direct[di] == node;
            if (queried) di++;
            for (size_t i = 0; i < n_cols; i++)          // columns of this layer, in the caller's order (stable sort by size)
                if (col_log_sizes[i] == (u32)lg) (queried ? out.queried : out.witness).push_back({cols[i], node});
            cur.push_back(node);
        }
        last.swap(cur);
    }
    return TSTWO_OK;
}

// The words the lists select: 8-word digests, then 1-word column values (gather_to_host), handed out to the caller's buffers.
// (the last n_extra entries of l.hashes go to `extra` instead of hash_witness: the roots of a FRI proof's trees)
static int run_decommit(const DecommitLists &l, u32 *queried_values, uint8_t *hash_witness, u32 *column_witness, size_t n_extra = 0,
                        uint8_t *extra = nullptr) {
    const size_t nh = l.hashes.size(), nq = l.queried.size(), nw = l.witness.size(), nv = nq + nw;
    if (nh + nv == 0) return TSTWO_OK;
    std::vector<GatherItem> items;
    items.reserve(nh + nv);
    items.insert(items.end(), l.hashes.begin(), l.hashes.end());
    items.insert(items.end(), l.queried.begin(), l.queried.end());
    items.insert(items.end(), l.witness.begin(), l.witness.end());
    std::vector<u32> host(8 * nh + nv);
    int rc = gather_to_host(items.data(), nh, 8u, nv, 1u, host.data());
    if (rc) return rc;
    if (nh - n_extra) memcpy(hash_witness, host.data(), 32 * (nh - n_extra));
    if (n_extra) memcpy(extra, host.data() + 8 * (nh - n_extra), 32 * n_extra);
    if (nq) memcpy(queried_values, host.data() + 8 * nh, 4 * nq);
    if (nw) memcpy(column_witness, host.data() + 8 * nh + nq, 4 * nw);
    return TSTWO_OK;
}

// totals[3]: the capacities of the three output buffers (in elements) on entry, the required counts on return.  An error when a
// list does not fit its buffer or has none to go to.
static int claim_outputs(const char *who, size_t n_values, size_t n_hashes, size_t n_witness, const void *values, const void *hashes,
                         const void *witness, size_t totals[3]) {
    const size_t need[3] = {n_values, n_hashes, n_witness};
    const void *const buf[3] = {values, hashes, witness};
    bool fits = true;
    for (int k = 0; k < 3; k++) {
        fits = fits && need[k] <= totals[k] && (need[k] == 0 || buf[k]);
        totals[k] = need[k];
    }
    return fits ? TSTWO_OK : set_error(TSTWO_ERR_BAD_ARG, std::string(who) + ": output buffer too small (required counts returned)");
}

// Request r is described by reqs[r]; the outputs are the concatenation of the per-tree outputs in request order,
// counts[3r..3r+2] = (queried values, hashes, column witness words) of request r.
static int decommit_trees(const tstwo_decommit_request *reqs, size_t n_reqs, u32 *queried_values, uint8_t *hash_witness, u32 *column_witness,
                          size_t *counts, size_t totals[3]) {
    DecommitLists l;
    for (size_t r = 0; r < n_reqs; r++) {
        const size_t q0 = l.queried.size(), h0 = l.hashes.size(), w0 = l.witness.size();
        const tstwo_decommit_request &q = reqs[r];
        int rc = plan_decommit(q.layers, q.max_log, q.cols, q.col_log_sizes, q.n_cols, q.query_logs, q.queries, q.n_queries,
                               q.n_query_sets, l);
        if (rc) return rc;
        counts[3 * r] = l.queried.size() - q0;
        counts[3 * r + 1] = l.hashes.size() - h0;
        counts[3 * r + 2] = l.witness.size() - w0;
    }
    int rc = claim_outputs("merkle decommit", l.queried.size(), l.hashes.size(), l.witness.size(), queried_values, hash_witness, column_witness, totals);
    if (rc) return rc;
    return run_decommit(l, queried_values, hash_witness, column_witness);
}

// MerkleProver.decommit of one tree: the one-request case of tstwo_merkle_decommit_many.  *n_queried, *n_hashes,
// *n_column_witness are in/out like its totals[3] (capacities / required sizes).
int tstwo_merkle_decommit(const uint8_t *layers, u32 max_log, const u32 *const *cols, const u32 *col_log_sizes, size_t n_cols,
                          const u32 *query_logs, const uint64_t *const *queries, const size_t *n_queries, size_t n_query_sets,
                          u32 *queried_values, size_t *n_queried, uint8_t *hash_witness, size_t *n_hashes,
                          u32 *column_witness, size_t *n_column_witness) {
    TSTWO_REQUIRE_READY();
    if (!n_queried || !n_hashes || !n_column_witness) return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: null argument");
    const tstwo_decommit_request req = {layers, max_log, cols, col_log_sizes, n_cols, query_logs, queries, n_queries, n_query_sets};
    size_t counts[3], totals[3] = {*n_queried, *n_hashes, *n_column_witness};
    int rc = decommit_trees(&req, 1, queried_values, hash_witness, column_witness, counts, totals);
    *n_queried = totals[0]; *n_hashes = totals[1]; *n_column_witness = totals[2];
    return rc;
}

// Several trees in one round trip (every layer of a FRI proof, every tree of a commitment scheme).  totals[3] is in/out:
// capacities / required sizes.
int tstwo_merkle_decommit_many(const tstwo_decommit_request *reqs, size_t n_reqs, u32 *queried_values, uint8_t *hash_witness,
                               u32 *column_witness, size_t *counts, size_t totals[3]) {
    TSTWO_REQUIRE_READY();
    if ((n_reqs && (!reqs || !counts)) || !totals) return set_error(TSTWO_ERR_BAD_ARG, "merkle decommit: null argument");
    return decommit_trees(reqs, n_reqs, queried_values, hash_witness, column_witness, counts, totals);
}

// ---- FriProver.decommit_on_queries (fri.ts:768-785) in ONE call: the position logic of
// computeDecommitmentPositionsAndWitnessEvals (fri.ts:346-384) for every layer, the Merkle walk of every layer's tree
// (vcs/prover.ts:32-109, plan_decommit above) and ONE gather round trip for all witness evaluations, hash witnesses and
// column witnesses of the proof.
namespace {
// Queries.fold (queries.ts:140-158): positions >> n, de-duplicated (the input is ascending, so is the output)
void fold_queries(std::vector<uint64_t> &q, u32 n) {
    size_t w = 0;
    for (size_t i = 0; i < q.size(); i++) {
        const uint64_t v = q[i] >> n;
        if (w == 0 || q[w - 1] != v) q[w++] = v;
    }
    q.resize(w);
}
// fri.ts:346-384: every position of the folding cosets the queries touch (-> Merkle query set), and those among them the
// verifier cannot compute itself (-> witness evaluations)
void decommitment_positions(const std::vector<uint64_t> &q, u32 fold_step, std::vector<uint64_t> &positions, std::vector<uint64_t> &witness) {
    size_t i = 0;
    while (i < q.size()) {
        const uint64_t coset = q[i] >> fold_step, start = coset << fold_step;
        const size_t first = i;
        while (i < q.size() && (q[i] >> fold_step) == coset) i++;
        size_t k = first;
        for (uint64_t pos = start; pos < start + ((uint64_t)1 << fold_step); pos++) {
            positions.push_back(pos);
            if (k < i && q[k] == pos) { k++; continue; }       // the verifier can calculate this one
            witness.push_back(pos);
        }
    }
}
}  // namespace

int tstwo_fri_decommit(const tstwo_fri_layer *fri_layers, size_t n_layers, const uint64_t *queries, size_t n_queries, u32 log_domain_size,
                       u32 first_fold_step, u32 fold_step, u32 *witness_evals, uint8_t *hash_witness, u32 *column_witness, uint8_t *commitments,
                       size_t *counts, size_t totals[3]) {
    TSTWO_REQUIRE_READY();
    if ((n_layers && (!fri_layers || !counts)) || (n_queries && !queries) || !totals) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: null argument");
    if (log_domain_size > 31 || first_fold_step > 31 || fold_step > 31 || fold_step == 0) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: log size / fold step out of range");
    std::vector<uint64_t> q(queries, queries + n_queries);
    for (size_t i = 0; i < n_queries; i++) {
        if (q[i] >> log_domain_size) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: query position outside the domain");
        if (i && q[i - 1] >= q[i]) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: query positions must be ascending and distinct");
    }
    DecommitLists l;
    std::vector<GatherItem> evals;            // one item per coordinate word of a witness evaluation, layer by layer
    std::vector<std::vector<uint64_t>> pos_sets;
    for (size_t r = 0; r < n_layers; r++) {
        const tstwo_fri_layer &fl = fri_layers[r];
        if (!fl.layers || !fl.n_evals || !fl.cols || !fl.eval_logs) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: null argument");
        TSTWO_REQUIRE_TABLE(fl.cols, 4 * fl.n_evals);
        const size_t h0 = l.hashes.size(), w0 = l.witness.size(), e0 = evals.size();
        // Merkle query sets of this tree: one per distinct evaluation size (first layer: the circle evaluations folded to their
        // own size, get_query_positions_by_log_size fri.ts:470-480; inner layers: the one line evaluation)
        pos_sets.clear();
        std::vector<u32> set_logs;
        std::vector<u32> col_logs(4 * fl.n_evals);
        const u32 step = r == 0 ? first_fold_step : fold_step;
        for (size_t e = 0; e < fl.n_evals; e++) {
            const u32 lg = fl.eval_logs[e];
            if (lg > log_domain_size || lg > fl.max_log) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: evaluation larger than its tree / the query domain");
            if (r > 0 && (fl.n_evals != 1 || lg != fl.max_log)) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: an inner layer commits one line evaluation");
            for (int k = 0; k < 4; k++) col_logs[4 * e + k] = lg;
            std::vector<uint64_t> cq = q;
            if (r == 0) fold_queries(cq, log_domain_size - lg);
            else if (cq.size() && (cq.back() >> lg)) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: layer sizes do not follow the fold steps");
            std::vector<uint64_t> pos, wit;
            decommitment_positions(cq, step, pos, wit);
            if (pos.size() && (pos.back() >> lg)) return set_error(TSTWO_ERR_BAD_ARG, "fri decommit: fold step larger than the evaluation");
            for (uint64_t p : wit)
                for (int k = 0; k < 4; k++) evals.push_back({fl.cols[4 * e + k], p});
            bool seen = false;
            for (u32 sl : set_logs) seen = seen || sl == lg;
            if (!seen) { set_logs.push_back(lg); pos_sets.push_back(std::move(pos)); }
        }
        std::vector<const uint64_t *> qp(pos_sets.size());
        std::vector<size_t> qn(pos_sets.size());
        for (size_t k = 0; k < pos_sets.size(); k++) { qp[k] = pos_sets[k].data(); qn[k] = pos_sets[k].size(); }
        const size_t q0 = l.queried.size();
        int rc = plan_decommit(fl.layers, fl.max_log, fl.cols, col_logs.data(), 4 * fl.n_evals, set_logs.data(), qp.data(), qn.data(), pos_sets.size(), l);
        if (rc) return rc;
        l.queried.resize(q0);                  // the queried values themselves are not part of a FRI layer proof (fri.ts:262-269)
        counts[3 * r] = (evals.size() - e0) / 4;
        counts[3 * r + 1] = l.hashes.size() - h0;
        counts[3 * r + 2] = l.witness.size() - w0;
        // the next layer is queried at the folded positions (fri.ts:776-783)
        fold_queries(q, r == 0 ? first_fold_step : fold_step);
    }
    int rc = claim_outputs("fri decommit", evals.size() / 4, l.hashes.size(), l.witness.size(), witness_evals, hash_witness, column_witness, totals);
    if (rc) return rc;
    l.queried = evals;                         // travel as the "queried" 1-word items of the shared gather
    if (commitments)                           // the trees' roots (FriLayerProof.commitment) ride along: digest 0 of every layers buffer
        for (size_t r = 0; r < n_layers; r++) l.hashes.push_back({(const u32 *)fri_layers[r].layers, 0});
    return run_decommit(l, witness_evals, hash_witness, column_witness, commitments ? n_layers : 0, commitments);
}

}  // extern "C"

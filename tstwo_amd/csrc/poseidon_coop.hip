// poseidon_coop.hip — Poseidon252 with one hash per 8 lanes (felt252_coop.cuh), for the places where a hash waits for the one
// before it: hash_many and commitOnLayer with 8 lanes per message / node, Poseidon252Channel on the device (channel/poseidon.ts:
// 122-360, vcs/poseidon252_merkle.ts:146-178) and FriProver.commit's layer loop over Poseidon trees in one call.  poseidon.hip
// keeps the lane-per-hash kernels, which win wherever there are enough hashes to fill the device (poseidon_plan.h: the threshold).
//
// A group of 8 lanes owns a hash and every field operation shuffles inside the group: a kernel here clamps the index of a tail
// group to the last valid one (it recomputes that hash) and masks its store; no lane leaves early.
#include <vector>

#include "common.h"
#include "felt252_coop.cuh"
#include "fri_plan.h"
#include "poseidon_plan.h"

using namespace tstwo;
using feltc::Lane;

namespace {

constexpr int kThreads = 256;
constexpr int kGroups = kThreads / 8;          // hashes per workgroup

// hash_many over n_in elements (felt252.cuh's sponge): elem(e) is THIS lane's limb of element e, canonical; n_in is wave-uniform.
template <class Elem>
__device__ __forceinline__ u32 sponge(const Lane &l, u32 n_in, const Elem &elem) {
    u32 s0 = 0u, s1 = 0u, s2 = 0u;
    const u32 pairs = (n_in + 2u) / 2u;            // n_in + 1 elements padded to an even count
#pragma unroll 1
    for (u32 q = 0; q < pairs; q++) {
        const u32 e = 2u * q;
        u32 x, y;
        if (e < n_in) x = feltc::to_mont(l, elem(e));
        else x = l.one;                             // e == n_in: the appended 1
        if (e + 1u < n_in) y = feltc::to_mont(l, elem(e + 1u));
        else if (e + 1u == n_in) y = l.one;
        else y = 0u;                                // the padding 0
        s0 = feltc::add(l, s0, x);
        s1 = feltc::add(l, s1, y);
        feltc::hades_coop(l, s0, s1, s2);
    }
    return feltc::from_mont(l, s0);
}

// tstwo_poseidon252_hash_many_coop: group g hashes message g = in[g k .. g k + k) (elements of 8 words), lane j its limb j.
__global__ void __launch_bounds__(kThreads) k_p252c_hash_many(const u32 *__restrict__ in, size_t n, u32 k, u32 *__restrict__ out) {
    const Lane l = feltc::lane_info();
    size_t g = (size_t)blockIdx.x * kGroups + threadIdx.x / 8;
    const bool live = g < n;
    if (!live) g = n - 1;                           // a tail group hashes the last message again and stores nothing
    const u32 *msg = in + g * k * 8 + l.j;
    const u32 h = sponge(l, k, [&](u32 e) { return gload1(msg + 8 * (size_t)e); });
    if (live) gstore1(out + 8 * g + l.j, h);
}

// Column pointer i for a lane-varying i: one 8-byte vector load from the device table or from the by-value table at the start of
// the kernel-argument segment (ColPtrs is the first kernel argument), through the constant address space.
__device__ __forceinline__ const u32 *colp_v(const ColPtrs &c, u32 i) {
    typedef const unsigned long long __attribute__((address_space(4))) *k64;
    typedef const char __attribute__((address_space(4))) *kbytes;
    const k64 tab = c.ext ? (k64)(unsigned long long)c.ext : (k64)((kbytes)__builtin_amdgcn_kernarg_segment_ptr());
    return (const u32 *)tab[i];
}

// commitOnLayer with 8 lanes per node: node i = hashNode((prev[2i], prev[2i+1]) if HAS_PREV, cols[..][i]).  Lane j reads limb j of a
// child, and of column block b the value of column 8b + 7 - j (absent ones zero), which is where pack_m31x8 wants it.
template <bool HAS_PREV>
__global__ void __launch_bounds__(kThreads) k_p252c_layer(ColPtrs cols, u32 n_cols, const u32 *__restrict__ prev, u32 *__restrict__ out,
                                                          size_t n_nodes) {
    const Lane l = feltc::lane_info();
    size_t node = (size_t)blockIdx.x * kGroups + threadIdx.x / 8;
    const bool live = node < n_nodes;
    if (!live) node = n_nodes - 1;
    const u32 nch = HAS_PREV ? 2u : 0u;
    const u32 n_in = nch + (n_cols + 7u) / 8u;
    const u32 h = sponge(l, n_in, [&](u32 e) {
        if (HAS_PREV && e < 2u) return gload1(prev + 8 * (2 * node + e) + l.j);
        const u32 ci = 8u * (e - nch) + 7u - l.j;
        u32 v = 0u;
        if (ci < n_cols) v = gload1(colp_v(cols, ci) + node);
        return feltc::pack_m31x8(l, v);
    });
    if (live) gstore1(out + 8 * node + l.j, h);
}

// Poseidon252Channel in device memory: chan = 8 digest limbs (canonical), n_challenges, n_sent.  One wave; its 8 groups compute the
// same thing and group 0 stores.  root: mix_root = hash_many([digest, root]), 2 permutations; felt: draw_felt = the first four
// 31-bit slices of poseidonHash(digest, n_sent) = Hades(digest, n_sent, 2)[0], each reduced as M31.reduce does.
__global__ void __launch_bounds__(64) k_p252c_channel(u32 *__restrict__ chan, const u32 *__restrict__ root, u32 *__restrict__ felt) {
    const Lane l = feltc::lane_info();
    u32 d = gload1(chan + l.j);
    u32 n_challenges = gload1(chan + 8), n_sent = gload1(chan + 9);
    if (root) {                                                    // wave-uniform
        const u32 r = gload1(root + l.j), d0 = d;
        d = sponge(l, 2u, [&](u32 e) { return e ? r : d0; });
        n_challenges += 1u;
        n_sent = 0u;
    }
    if (felt) {
        u32 s0 = feltc::to_mont(l, d), s1 = feltc::to_mont(l, l.j == 0u ? n_sent : 0u), s2 = feltc::dbl(l, l.one);
        feltc::hades_coop(l, s0, s1, s2);
        const u32 h = feltc::from_mont(l, s0);
        n_sent += 1u;
        // slice k = bits [31 k, 31 k + 31) of h: from limbs (31 k) >> 5 and the next one; computed by every lane for k = j & 3
        const u32 k = l.j & 3u, l0 = (31u * k) >> 5, sh = (31u * k) & 31u, base = l.lane & ~7u;
        const u32 lo = (u32)__shfl((int)h, (int)(base + l0)), hi = (u32)__shfl((int)h, (int)(base + l0 + 1u));
        u32 word = (u32)((((unsigned long long)hi << 32) | lo) >> sh) & 0x7fffffffu;
        if (word == 0x7fffffffu) word = 0u;
        if (l.lane < 4u) gstore1(felt + l.lane, word);
    }
    if (l.lane < 8u) gstore1(chan + l.lane, d);
    if (l.lane == 0u) {
        gstore1(chan + 8, n_challenges);
        gstore1(chan + 9, n_sent);
    }
}

int coop_commit_layer(u32 log_size, const uint8_t *prev, const u32 *const *cols, size_t n_cols, uint8_t *out) {
    if (log_size > 30) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: log size out of range");
    if (!out) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null output layer");
    if (!aligned16(out) || !aligned16(prev)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: layers must be 16-byte aligned");
    if (n_cols > 0xFFFFFFF0u) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: too many columns");
    ColPtrs cp;
    if (n_cols == 0) {
        for (int k = 0; k < kMaxColsPerLaunch; k++) cp.p[k] = nullptr;
        cp.ext = nullptr;
    } else if (int rc = fill_col_table(cp, cols, n_cols, 0)) {
        return rc;
    }
    const size_t n_nodes = (size_t)1 << log_size;
    const dim3 grid(ceil_div(n_nodes, kGroups));
    if (prev)
        hipLaunchKernelGGL(k_p252c_layer<true>, grid, dim3(kThreads), 0, ctx().stream, cp, (u32)n_cols, (const u32 *)prev, (u32 *)out, n_nodes);
    else
        hipLaunchKernelGGL(k_p252c_layer<false>, grid, dim3(kThreads), 0, ctx().stream, cp, (u32)n_cols, (const u32 *)nullptr, (u32 *)out, n_nodes);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// A whole tree in tstwo_merkle_commit's layout (layer k at byte 32 (2^k - 1)): per layer the kernel poseidon_plan.h names.
int commit_tree(const u32 *const *cols, const u32 *log_sizes, size_t n_cols, uint8_t *layers) {
    u32 max_log = 0;
    for (size_t i = 0; i < n_cols; i++) max_log = log_sizes[i] > max_log ? log_sizes[i] : max_log;
    std::vector<const u32 *> lc(n_cols);
    const uint8_t *prev = nullptr;
    for (int lg = (int)max_log; lg >= 0; lg--) {                   // vcs/prover.ts:24-27
        size_t k = 0;
        for (size_t i = 0; i < n_cols; i++)
            if (log_sizes[i] == (u32)lg) lc[k++] = cols[i];
        uint8_t *dst = layers + 32 * (((size_t)1 << lg) - 1);
        const int rc = p252_layer_is_coop((u32)lg) ? coop_commit_layer((u32)lg, prev, lc.data(), k, dst)
                                                   : tstwo_poseidon252_merkle_commit_layer((u32)lg, prev, lc.data(), k, dst);
        if (rc) return rc;
        prev = dst;
    }
    return TSTWO_OK;
}

int channel_step(u32 *chan, const uint8_t *root, u32 *felt) {
    hipLaunchKernelGGL(k_p252c_channel, dim3(1), dim3(64), 0, ctx().stream, chan, (const u32 *)root, felt);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // namespace

extern "C" {

int tstwo_poseidon252_hash_many_coop(const u32 *in, size_t n_msgs, u32 felts_per_msg, u32 *out) {
    TSTWO_REQUIRE_READY();
    if (n_msgs == 0) return TSTWO_OK;
    if (!out || (felts_per_msg && !in)) return set_error(TSTWO_ERR_BAD_ARG, "null device pointer");
    if (!aligned16(in) || !aligned16(out)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252: buffers must be 16-byte aligned");
    if (n_msgs > ((size_t)1 << 32) || felts_per_msg > (1u << 20)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252: batch too large");
    hipLaunchKernelGGL(k_p252c_hash_many, dim3(ceil_div(n_msgs, kGroups)), dim3(kThreads), 0, ctx().stream, in, n_msgs, felts_per_msg, out);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_poseidon252_merkle_commit_layer_coop(u32 log_size, const uint8_t *prev, const u32 *const *cols, size_t n_cols, uint8_t *out) {
    TSTWO_REQUIRE_READY();
    if (n_cols && !cols) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null column table");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    return coop_commit_layer(log_size, prev, cols, n_cols, out);
}

int tstwo_poseidon252_channel_mix_root_draw_felt(u32 *chan, const uint8_t *root, u32 *felt) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(chan);
    if ((((uintptr_t)root) & 3) || (((uintptr_t)felt) & 3)) return set_error(TSTWO_ERR_BAD_ARG, "channel: unaligned pointer");
    return channel_step(chan, root, felt);
}

// tstwo_fri_commit_layers (fri.hip) over Poseidon trees and the Poseidon device channel: the same checks in the same order, the same
// ownership of what it returns, the unfused schedule of fri_plan.h (the fused kinds hash Blake2s leaves inside the fold).
int tstwo_fri_commit_layers_poseidon252(const u32 *const *circle_cols, const u32 *col_logs, size_t n_columns, const u32 *itw, u32 tw_log,
                                        u32 log_last_layer_size, u32 *chan, u32 *alphas, size_t alphas_cap, uint8_t **first_tree,
                                        tstwo_fri_layer_out *out, size_t out_cap, size_t *n_out) {
    TSTWO_REQUIRE_READY();
    if (!circle_cols || !col_logs || !first_tree || !out || !n_out) return set_error(TSTWO_ERR_BAD_ARG, "fri commit: null argument");
    *n_out = 0;
    *first_tree = nullptr;
    TSTWO_REQUIRE_TABLE(circle_cols, 4 * n_columns);
    TSTWO_REQUIRE_PTRS(itw, chan, alphas);
    if (!aligned16(alphas)) return set_error(TSTWO_ERR_BAD_ARG, "fold: alpha must be 16-byte aligned");
    std::vector<FriStep> plan;
    if (const char *why = fri_plan(col_logs, n_columns, log_last_layer_size, plan, false)) return set_error(TSTWO_ERR_BAD_ARG, why);
    const u32 first_log = col_logs[0] - 1;
    const size_t n_inner = first_log - log_last_layer_size;
    if (out_cap < n_inner + 1 || alphas_cap < n_inner + 1) return set_error(TSTWO_ERR_BAD_ARG, "fri commit: output / alpha capacity too small");
    if (tw_log > 31 || first_log > tw_log) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");      // bounds every fold's need
    std::vector<void *> owned;                       // everything allocated here, released again if a step fails
    auto fail = [&](int rc) { for (void *p : owned) (void)tstwo_free(p); *first_tree = nullptr; return rc; };
    auto alloc = [&](void **p, size_t bytes) { int rc = tstwo_malloc(p, bytes); if (!rc) owned.push_back(*p); return rc; };
    auto alloc_tree = [&](uint8_t **t, u32 lg) { return alloc((void **)t, tstwo_merkle_layers_bytes(lg)); };
    auto alloc_eval = [&](u32 *cols[4], u32 lg) {
        for (int k = 0; k < 4; k++) { int rc = alloc((void **)&cols[k], sizeof(u32) << lg); if (rc) return rc; }
        return (int)TSTWO_OK;
    };
    u32 *ev[32][4] = {};                             // line layer i: its evaluation and its tree (the last layer has none)
    uint8_t *tree[32] = {};
    for (const FriStep &s : plan) {
        u32 *const a_in = alphas + 4 * (size_t)s.alpha_in, *const a_out = alphas + 4 * (size_t)s.alpha_out;
        const u32 lg4[4] = {s.log, s.log, s.log, s.log};
        int rc = TSTWO_OK;
        switch (s.kind) {
        case FriStep::FIRST_TREE: {                  // one tree over every circle column's coordinate columns, root -> channel -> alpha_0
            std::vector<u32> logs(4 * n_columns);
            for (size_t i = 0; i < n_columns; i++) for (int k = 0; k < 4; k++) logs[4 * i + k] = col_logs[i];
            if ((rc = alloc_tree(first_tree, s.log))) break;
            if ((rc = commit_tree(circle_cols, logs.data(), 4 * n_columns, *first_tree))) break;
            rc = channel_step(chan, *first_tree, a_out);
            break;
        }
        case FriStep::CIRCLE_WRITE:                  // the line evaluation starts at zero: written, not accumulated (fri.hip)
            if ((rc = alloc_eval(ev[s.layer], s.log))) break;
            [[fallthrough]];
        case FriStep::CIRCLE_ACCUM:
            rc = fri_fold_circle_dev(ev[s.layer], (size_t)1 << s.log, circle_cols + 4 * s.column, col_logs[s.column], itw, tw_log, a_in,
                                     s.kind == FriStep::CIRCLE_ACCUM);
            break;
        case FriStep::COMMIT:
            if ((rc = alloc_tree(&tree[s.layer], s.log))) break;
            if ((rc = commit_tree(ev[s.layer], lg4, 4, tree[s.layer]))) break;
            rc = channel_step(chan, tree[s.layer], a_out);
            break;
        case FriStep::FOLD_LINE:
            if ((rc = alloc_eval(ev[s.layer], s.log))) break;
            rc = tstwo_fri_fold_line_dev(ev[s.layer - 1], s.log + 1, itw, tw_log, a_in, ev[s.layer]);
            break;
        default:                                     // the unfused schedule has no other kind
            rc = set_error(TSTWO_ERR_BAD_ARG, "fri commit: fused step in a Poseidon252 schedule");
            break;
        }
        if (rc) return fail(rc);
    }
    for (size_t i = 0; i <= n_inner; i++) {
        out[i].log_size = first_log - (u32)i;
        for (int k = 0; k < 4; k++) out[i].cols[k] = ev[i][k];
        out[i].layers = tree[i];
    }
    *n_out = n_inner + 1;
    return TSTWO_OK;
}

}  // extern "C"

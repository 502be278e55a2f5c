// merkle.hip — MerkleOps.commitOnLayer / MerkleProver.commit over BLAKE2s-256 (the compression itself: blake2s.cuh).
//
// Node message = [left32 || right32]? || LE32(col_0[i]) || ... || LE32(col_{C-1}[i]) (vcs/blake2_merkle.ts:9-24), one lane per
// node in the wide layers: column-major columns make lane i read word i of every column, one coalesced 256-byte access per column
// per wave.  Algorithmic bytes for a layer of n nodes: 4*C*n (+ 64*n children) read, 32*n written; the compression is VALU-bound
// (~1.2k lane-ops per 64-byte block) — DESIGN.md §4.2 prices it against the integer-issue ceiling as well as the HBM roofline.
//
// Holds the layer kernels (k_merkle_layer, k_merkle_leaf_static, k_merkle_leaf_pair, k_merkle_leaf4, k_merkle_inner[_set],
// k_merkle_subtree2c); the latency path below 2^kUpLog nodes, a quad of lanes per node (k_merkle_upq, k_merkle_leaf4_upq) with
// the channel step that can ride on a root (ChanHook, k_channel_mix_draw); the FRI commit tail (k_fri_tail) and the grind
// (k_grind); then the host side.  Which launches an input takes — kernel, layer, levels, grid, trees, columns, who carries the fold
// and the channel step — is merkle_plan.h's, decided before anything is launched; run_plan here issues a plan's steps from the
// pointers of the call, and every entry is "check the pointers, plan, run_plan": tstwo_merkle_commit[_layer|_many],
// merkle_commit_then_channel.  Then launch_fri_tail, tstwo_channel_mix_root_draw_felt, tstwo_grind_blake2s.  Reading trees back is
// decommit.hip's.
#include <string.h>

#include <type_traits>
#include <vector>

#include "blake2s.cuh"
#include "common.h"
#include "grind_plan.h"
#include "merkle_plan.h"

using namespace tstwo;
using namespace tstwo::b2s;

namespace {

struct LayerParams {
    u32 total_words;   // W: message length in 32-bit words (16 if children, plus one per column)
    u32 w_begin;       // first message word handled by this launch (multiple of 16)
    u32 w_end;         // one past the last word handled (multiple of 16, or >= W on the final launch)
    u32 col_word0;     // message word index of cols.p[0]
    u32 n_cols;        // columns in this launch's table
    u32 load_state;    // 1: resume from the 8-word state stored in out[] by the previous launch
    u32 is_final;      // 1: this launch holds the last block (finalise)
};

// One lane hashes several nodes (grid-stride) and software-pipelines the message: the 16 words of the next
// 64-byte block are fetched into a second register set while the current block is compressed, so the
// compression (VALU-bound, ~1k ops) hides the HBM latency.  Loads are never branched around (a per-word
// branch makes hipcc wait vmcnt(0) per element): out-of-range words read a clamped column and are zeroed
// by a select.
template <bool HAS_PREV>
__device__ __forceinline__ void load_block(u32 (&m)[16], const uint4 *__restrict__ prev, const HashColPtrs &cols,
                                           const LayerParams &lp, size_t node, u32 w) {
    if (HAS_PREV && w == 0) {      // wave-uniform
        const uint4 *c = prev + 4 * node;
        uint4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        m[0] = c0.x; m[1] = c0.y; m[2] = c0.z; m[3] = c0.w; m[4] = c1.x; m[5] = c1.y; m[6] = c1.z; m[7] = c1.w;
        m[8] = c2.x; m[9] = c2.y; m[10] = c2.z; m[11] = c2.w; m[12] = c3.x; m[13] = c3.y; m[14] = c3.z; m[15] = c3.w;
    } else if (lp.n_cols == 0) {   // wave-uniform: empty message block
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = 0u;
    } else {
        const u32 last = lp.n_cols - 1u;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const u32 ci = w + (u32)k - lp.col_word0;                // wave-uniform
            const u32 v = cols.p[min(ci, last)][node];
            m[k] = (ci <= last) ? v : 0u;
        }
    }
}

template <bool HAS_PREV>
__global__ void __launch_bounds__(256) k_merkle_layer(const uint4 *__restrict__ prev, HashColPtrs cols, uint4 *__restrict__ out,
                                                     size_t n_nodes, LayerParams lp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t node0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 W = lp.total_words;
    const u32 w_stop = lp.w_end < W ? lp.w_end : W;
    // wave-uniform trip structure: `rows` nodes per lane (tail lanes clamp their loads and skip their stores),
    // `nb` 64-byte blocks per node
    const u32 nb = w_stop > lp.w_begin ? (w_stop - lp.w_begin + 15u) / 16u : 1u;
    const u32 rows = (u32)((n_nodes + stride - 1) / stride);
    const u32 total = rows * nb;
    const size_t last_node = n_nodes - 1;

    u32 ma[16], mb[16], h[8];
    u32 j = 0, blk = 0;                                   // uniform: row number / block number of the block in flight
    load_block<HAS_PREV>(ma, prev, cols, lp, min(node0, last_node), lp.w_begin);

#define MERKLE_STEP(CUR, NXT)                                                                                         \
    {                                                                                                                 \
        const size_t node = node0 + (size_t)j * stride;                                                               \
        const size_t nc = min(node, last_node);                                                                       \
        const u32 wc = lp.w_begin + 16u * blk;                                                                        \
        if (blk == 0) {                                                                                               \
            if (lp.load_state) {                                                                                      \
                uint4 a = out[2 * nc], b = out[2 * nc + 1];                                                           \
                h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w; h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;       \
            } else {                                                                                                  \
                h[0] = IV0 ^ 0x01010020u; h[1] = IV1; h[2] = IV2; h[3] = IV3; h[4] = IV4; h[5] = IV5; h[6] = IV6; h[7] = IV7; \
            }                                                                                                         \
        }                                                                                                             \
        u32 jn = j, bn = blk + 1;                                                                                     \
        if (bn == nb) { bn = 0; jn = j + 1; }                                                                         \
        if (it + 1 < total)                                                                                           \
            load_block<HAS_PREV>(NXT, prev, cols, lp, min(node0 + (size_t)jn * stride, last_node), lp.w_begin + 16u * bn); \
        const u32 bytes_end = (wc + 16 < W ? wc + 16 : W) * 4u;                                                       \
        b2s_compress(h, CUR, bytes_end, lp.is_final && (wc + 16 >= W));                                               \
        if (blk + 1 == nb && node < n_nodes) {                                                                        \
            out[2 * node] = make_uint4(h[0], h[1], h[2], h[3]);                                                       \
            out[2 * node + 1] = make_uint4(h[4], h[5], h[6], h[7]);                                                   \
        }                                                                                                             \
        j = jn; blk = bn;                                                                                             \
    }

    for (u32 it = 0; it < total; it += 2) {
        MERKLE_STEP(ma, mb)
        if (it + 1 < total) {
            const u32 it_save = it;
            it = it_save + 1;
            MERKLE_STEP(mb, ma)
            it = it_save;
        }
    }
#undef MERKLE_STEP
}

// ---- lean special cases of k_merkle_layer (same results, fewer non-hash instructions per compression) ----
// (1) bottom layer whose column count is exactly 16*NBLK (e.g. the 32-column trace shard): every message word has
//     a compile-time column index, so the column pointers are fetched once (scalar registers) instead of a
//     clamp + scalar load + select per word per block.
// Up to kMaxTrees equally shaped trees per launch (tstwo_merkle_commit_many): blockIdx.y selects the tree — its columns are
// cols.p[blockIdx.y * 16 * NBLK ...] of the by-value table, its layers buffer ts.t[blockIdx.y].
struct TreeSet { uint4 *t[kMaxTrees]; };
template <int NBLK>
__global__ void __launch_bounds__(256) k_merkle_leaf_static(HashColPtrs cols, TreeSet outs, size_t n_nodes) {
    uint4 *__restrict__ out = outs.t[blockIdx.y];
    const u32 col0 = blockIdx.y * (16 * NBLK);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t node0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 rows = (u32)((n_nodes + stride - 1) / stride);
    const size_t last_node = n_nodes - 1;
    u32 cur[16], nxt[16];
    // word `node` of column k = scalar base (kernel argument) + ONE 32-bit byte offset shared by all columns: global_load with
    // an SGPR base and a VGPR offset, instead of a 64-bit address pair per column in VGPRs (columns are at most 4 GiB: the
    // host takes this kernel for log_size <= 30 only)
    auto word = [&](int k, u32 byte_off) -> u32 { return *(const TSTWO_GLOBAL u32 *)((const TSTWO_GLOBAL char *)cols.p[col0 + k] + byte_off); };
    {
        const u32 oc = (u32)min(node0, last_node) * 4u;
#pragma unroll
        for (int k = 0; k < 16; k++) cur[k] = word(k, oc);
    }
    // The digest of node j is stored one compression LATER (behind the loads of node j + 1's first block): the compiler waits
    // vmcnt(0) at the loop header, so a store issued at the end of an iteration has its whole write latency exposed there
    // (gfx9 stores count on vmcnt); issued here it has a full compression to complete.  Costs 8 VGPRs.
    u32 hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t pnode = n_nodes;                                       // node whose digest is waiting in hp (none yet)
    for (u32 j = 0; j < rows; j++) {
        const size_t node = node0 + (size_t)j * stride;
        const size_t nn = min(node + stride, last_node);          // next node of this lane (clamped: loads are never branched around)
        const size_t nc = min(node, last_node);
        u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
#pragma unroll
        for (int b = 0; b < NBLK; b++) {
            // fetch the next 64-byte block (next block of this node, or block 0 of the lane's next node) while this one is compressed
            const int bn = (b + 1) % NBLK;
            const u32 src = (u32)((b + 1 < NBLK) ? nc : nn) * 4u;
#pragma unroll
            for (int k = 0; k < 16; k++) nxt[k] = word(16 * bn + k, src);
            if (b == 0 && pnode < n_nodes) {
                out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
                out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
            }
            b2s_compress(h, cur, 64u * (b + 1), b == NBLK - 1);
#pragma unroll
            for (int k = 0; k < 16; k++) cur[k] = nxt[k];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) hp[k] = h[k];
        pnode = node;
    }
    if (pnode < n_nodes) {
        out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
        out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
    }
}

// (1a) the same leaf layer AND the layer above it, when that layer has no columns: a lane owns the sibling rows 2i and 2i + 1, so
// the parent's message (left digest || right digest) is in its registers when the second leaf is done — layer log - 1 costs
// no load, no LDS and no launch of its own, and the column-free launches that follow read half as much.  One 8-byte load per
// column fetches word 2i (row A) and word 2i + 1 (row B): 512 contiguous bytes per wave instruction, from the column's scalar
// base plus one 32-bit byte offset (8 * pair < 2^32: the host takes this kernel for log_size <= 30 only).
// Order of a pair: A.b0, B.b0, A.b1, B.b1, ..., parent — two live states.  The next block (the lane's next pair's first block behind
// the last one) is requested in two halves: columns 0-7 before A's compression, columns 8-15 before B's, when A's 16 words are
// dead — 32 message registers less at the widest point than a whole block ahead, and every load still has at least one
// compression (the last half: B's and the parent's) to arrive.  Stores as in k_merkle_leaf_static, behind a compression's worth
// of time before anything waits for them: the two leaf digests (64 contiguous bytes per lane) go out in front of the parent's
// compression, whose message they are anyway; the parent (32 bytes) waits in hp for the next pair's first loads.  Default cache
// policy for the digests (non-temporal digest stores measured 16-24 % slower); NT is the policy of the COLUMN loads, words that
// are read exactly once.  Measured, non-temporal column loads lie inside the default policy's range (8 trees of 32 x 2^22, five
// rounds alternating: merkle_ms 2.138-2.149 against 2.140-2.156, profiles/merkle_pair_parent_vs_branch.txt): no gain, so the
// DEFAULT policy ships (TSTWO_MERKLE_PAIR_NT = 0 below); the parameter stays for the next measurement.
// The 8-byte loads need every column 8-byte aligned: the host takes this kernel only then (leaf_takes_pair), the static leaf otherwise.
// outs.t[tree] is layer log (2 * n_pairs digests); layer log - 1 lies 32 * n_pairs bytes below it in the same layers buffer.
#ifndef TSTWO_MERKLE_PAIR_NT
#define TSTWO_MERKLE_PAIR_NT 0
#endif
constexpr bool kPairNT = TSTWO_MERKLE_PAIR_NT != 0;
template <int NBLK, bool NT>
__global__ void __launch_bounds__(256) k_merkle_leaf_pair(HashColPtrs cols, TreeSet outs, size_t n_pairs) {
    uint4 *__restrict__ leaf = outs.t[blockIdx.y];
    uint4 *__restrict__ up = outs.t[blockIdx.y] - 2 * n_pairs;
    const u32 col0 = blockIdx.y * (16 * NBLK);
    // pair numbers fit 32 bits (n_pairs <= 2^29, the grid at most 2^21 lanes per tree): one register each, not two
    const u32 np = (u32)n_pairs, stride = gridDim.x * blockDim.x, pair0 = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 rows = (np + stride - 1) / stride;
    const u32 last_pair = np - 1;
    u32 ca[16], cb[16], na[16], nb[16];                            // rows A / B: the block being compressed, the block in flight
    auto words = [&](int k, u32 byte_off, u32 &a, u32 &b) {
        const u32x2_t v = gload_as<NT>((const TSTWO_GLOBAL u32x2_t *)((const TSTWO_GLOBAL char *)cols.p[col0 + k] + byte_off));
        a = v.x; b = v.y;
    };
    {
        const u32 oc = min(pair0, last_pair) * 8u;
#pragma unroll
        for (int k = 0; k < 16; k++) words(k, oc, ca[k], cb[k]);
    }
    u32 hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};                          // the parent digest waiting for its store
    u32 ppair = np;                                                // its node of layer log - 1 (none yet)
    for (u32 j = 0; j < rows; j++) {
        const u32 pair = pair0 + j * stride;
        const u32 pn = min(pair + stride, last_pair);                 // next pair of this lane (clamped: loads are never branched around)
        const u32 pc = min(pair, last_pair);
        Digest A = {{IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7}}, B = A;
        // one block of both rows; written out per block below, not as `#pragma unroll` over b: four blocks of two compressions are
        // past the size up to which the compiler honours the pragma, and a rolled loop indexes the pointer table at run time
        auto block = [&](auto bc) __attribute__((always_inline)) {
            constexpr int b = decltype(bc)::value;
            constexpr int bn = (b + 1) % NBLK;
            // (the offset is made opaque in front of each half so that its zero-extension is selected in the block of the loads:
            // extended in an earlier block it becomes a 64-bit VGPR offset, and every load gets a v_lshl_add_u64 and an address
            // pair of its own)
            u32 src = ((b + 1 < NBLK) ? pc : pn) * 8u;
            asm volatile("" : "+v"(src));
#pragma unroll
            for (int k = 0; k < 8; k++) words(16 * bn + k, src, na[k], nb[k]);
            if (b == 0 && ppair < np) {
                up[2 * (size_t)ppair] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
                up[2 * (size_t)ppair + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
            }
            b2s_compress(A.w, ca, 64u * (b + 1), b == NBLK - 1);
            asm volatile("" : "+v"(src));
#pragma unroll
            for (int k = 8; k < 16; k++) words(16 * bn + k, src, na[k], nb[k]);
            b2s_compress(B.w, cb, 64u * (b + 1), b == NBLK - 1);
#pragma unroll
            for (int k = 0; k < 16; k++) { ca[k] = na[k]; cb[k] = nb[k]; }
        };
        block(std::integral_constant<int, 0>{});
        if constexpr (NBLK > 1) block(std::integral_constant<int, 1>{});
        if constexpr (NBLK > 2) block(std::integral_constant<int, 2>{});
        if constexpr (NBLK > 3) block(std::integral_constant<int, 3>{});
        if (pair < np) {
            leaf[4 * (size_t)pair] = make_uint4(A.w[0], A.w[1], A.w[2], A.w[3]);
            leaf[4 * (size_t)pair + 1] = make_uint4(A.w[4], A.w[5], A.w[6], A.w[7]);
            leaf[4 * (size_t)pair + 2] = make_uint4(B.w[0], B.w[1], B.w[2], B.w[3]);
            leaf[4 * (size_t)pair + 3] = make_uint4(B.w[4], B.w[5], B.w[6], B.w[7]);
        }
        const Digest top = hash_pair(A, B);
#pragma unroll
        for (int k = 0; k < 8; k++) hp[k] = top.w[k];
        ppair = pair;
    }
    if (ppair < np) {
        up[2 * (size_t)ppair] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
        up[2 * (size_t)ppair + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
    }
}

// fold_line fused into the leaf hashing of the NEXT FRI layer's tree (the folded row IS that tree's 16-byte leaf message,
// vcs/blake2_merkle.ts:9-24 over the 4 coordinate columns): FoldSpec describes the layer being folded; the leaf kernels then
// compute row i = f0 + alpha f1 from rows 2i, 2i+1 (fri.ts:120-152), store it to the new evaluation and hash it from registers.
struct FoldSpec { const u32 *in[4]; const u32 *inv_x; const u32 *alpha; };       // alpha: 4 words in device memory (the drawn QM31)
struct FoldRow { uint2 a, b, c, d; u32 t; };
__device__ __forceinline__ FoldRow fold_row_load(const FoldSpec &fs, size_t i) {
    return {gload2(fs.in[0] + 2 * i), gload2(fs.in[1] + 2 * i), gload2(fs.in[2] + 2 * i), gload2(fs.in[3] + 2 * i), gload1(fs.inv_x + i)};
}
__device__ __forceinline__ qm31 fold_row(const FoldRow &r, qm31 alpha) {
    const qm31 f0 = {m31_add(r.a.x, r.a.y), m31_add(r.b.x, r.b.y), m31_add(r.c.x, r.c.y), m31_add(r.d.x, r.d.y)};
    const qm31 f1 = qm31_mul_m31({m31_sub(r.a.x, r.a.y), m31_sub(r.b.x, r.b.y), m31_sub(r.c.x, r.c.y), m31_sub(r.d.x, r.d.y)}, r.t);
    return qm31_add(f0, qm31_mul(alpha, f1));
}

// (1b) bottom layer of exactly 4 columns — every FRI layer (the 4 coordinate columns of a QM31 column): a 16-byte
//      message, one final block whose words 4..15 are zero.
template <bool FOLD>
__global__ void __launch_bounds__(256) k_merkle_leaf4(u32 *__restrict__ c0, u32 *__restrict__ c1, u32 *__restrict__ c2, u32 *__restrict__ c3,
                                                     uint4 *__restrict__ out, size_t n_nodes, FoldSpec fs) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t node0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 rows = (u32)((n_nodes + stride - 1) / stride);
    const size_t last_node = n_nodes - 1;
    auto word = [&](const u32 *col, u32 byte_off) -> u32 { return *(const TSTWO_GLOBAL u32 *)((const TSTWO_GLOBAL char *)col + byte_off); };
    const u32 o0 = (u32)min(node0, last_node) * 4u;       // scalar base + one 32-bit offset (log_size <= 30: host)
    u32 a = 0, b = 0, c = 0, d = 0;
    FoldRow fr = {};
    qm31 alpha = {0, 0, 0, 0};
    if (FOLD) {
        alpha = {fs.alpha[0], fs.alpha[1], fs.alpha[2], fs.alpha[3]};
        fr = fold_row_load(fs, min(node0, last_node));
    } else {
        a = word(c0, o0); b = word(c1, o0); c = word(c2, o0); d = word(c3, o0);
    }
    u32 hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};                        // deferred store: see k_merkle_leaf_static
    size_t pnode = n_nodes;
    for (u32 j = 0; j < rows; j++) {
        const size_t node = node0 + (size_t)j * stride;
        const size_t nn = min(node + stride, last_node);
        const u32 on = (u32)nn * 4u;
        u32 na = 0, nb = 0, ncc = 0, nd = 0;
        FoldRow nfr = {};
        if (FOLD) {
            nfr = fold_row_load(fs, nn);                             // next node's rows in flight during the compression
        } else {
            na = word(c0, on); nb = word(c1, on); ncc = word(c2, on); nd = word(c3, on);      // next node's words in flight during the compression
        }
        if (pnode < n_nodes) {
            out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
            out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
        }
        if (FOLD) {
            const qm31 r = fold_row(fr, alpha);
            a = r.a; b = r.b; c = r.c; d = r.d;
            if (node < n_nodes) { gstore1(c0 + node, a); gstore1(c1 + node, b); gstore1(c2 + node, c); gstore1(c3 + node, d); }
        }
        u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
        const u32 m[16] = {a, b, c, d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        b2s_compress(h, m, 16u, true);
#pragma unroll
        for (int k = 0; k < 8; k++) hp[k] = h[k];
        pnode = node;
        if (FOLD) fr = nfr;
        else { a = na; b = nb; c = ncc; d = nd; }
    }
    if (pnode < n_nodes) {
        out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
        out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
    }
}

// (2) inner layer without columns: node = Blake2s(left || right), one 64-byte block.
__device__ __forceinline__ void merkle_inner_body(const uint4 *__restrict__ prev, uint4 *__restrict__ out, size_t n_nodes) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t node0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 rows = (u32)((n_nodes + stride - 1) / stride);
    const size_t last_node = n_nodes - 1;
    uint4 c[4], cn[4];
    {
        const uint4 *p = prev + 4 * min(node0, last_node);
        c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; c[3] = p[3];
    }
    u32 hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};                        // deferred store: see k_merkle_leaf_static
    size_t pnode = n_nodes;
    for (u32 j = 0; j < rows; j++) {
        const size_t node = node0 + (size_t)j * stride;
        const uint4 *pn = prev + 4 * min(node + stride, last_node);
        cn[0] = pn[0]; cn[1] = pn[1]; cn[2] = pn[2]; cn[3] = pn[3];
        if (pnode < n_nodes) {
            out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
            out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
        }
        u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
        const u32 m[16] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w,
                           c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w};
        b2s_compress(h, m, 64u, true);
#pragma unroll
        for (int k = 0; k < 8; k++) hp[k] = h[k];
        pnode = node;
        c[0] = cn[0]; c[1] = cn[1]; c[2] = cn[2]; c[3] = cn[3];
    }
    if (pnode < n_nodes) {
        out[2 * pnode] = make_uint4(hp[0], hp[1], hp[2], hp[3]);
        out[2 * pnode + 1] = make_uint4(hp[4], hp[5], hp[6], hp[7]);
    }
}

__global__ void __launch_bounds__(256) k_merkle_inner(const uint4 *__restrict__ prev, uint4 *__restrict__ out, size_t n_nodes) {
    merkle_inner_body(prev, out, n_nodes);
}
// the same for layer log_out of every tree of a set (children = its layer log_out + 1)
__global__ void __launch_bounds__(256) k_merkle_inner_set(TreeSet ts, u32 log_out) {
    uint4 *layers = ts.t[blockIdx.y];
    merkle_inner_body(layers + 2 * (((size_t)1 << (log_out + 1)) - 1), layers + 2 * (((size_t)1 << log_out) - 1), (size_t)1 << log_out);
}

// (3) Two column-free layers in one launch: the four children of a node of layer `log_child - 2` hash into their two parents
// and then into that node, so that a parent's message is the two digests still in registers.  The intermediate layer is
// written once and never read back, and one launch disappears.  Both layers are written to their places in the layers buffer
// (MerkleProver keeps all layers, vcs/prover.ts:24-29; layer k at byte offset 32*(2^k - 1)).
// The two-level subtree with every global access a 1 KiB-contiguous wave access (round 4).  In round 3's lane-per-subtree form a
// lane read its four children as eight 16-byte loads at a 128-byte lane stride and wrote its digests at 64- and 32-byte lane strides: every
// instruction touches 64 lines a piece each, the pieces of a line arrive a compression apart, and with 32 waves per CU the lines
// do not survive in the caches in between — the counters showed 1.31 x the child bytes fetched and 1.16-1.24 x the digest bytes
// written (profiles/r03_cfft_pmc.json), on launches that move 4.3 TB/s.  Here a wave loads its 256 children as eight 1 KiB rows,
// transposes them to "lane owns 128 consecutive bytes" through its OWN 4.5 KiB of LDS (two halves of 4 KiB, one pad slot per
// 8 chunks: conflict-free both ways; wave-local, so no barrier — the LDS executes a wave's instructions in order), and stores
// the 128 + 64 digests it produced the same way, all six store instructions back to back at the end of the wave.
// Needs the top layer (2^(log_child-2) nodes) to be a multiple of 256 nodes.  Both callers launch it only for top layers of at
// least 2^kUpLog = 2^16 nodes (everything smaller goes to the quad-lane levels), so that always holds.
__device__ __forceinline__ u32 xslot(u32 chunk) { return chunk + (chunk >> 3); }
__global__ void __launch_bounds__(256) k_merkle_subtree2c(TreeSet ts, u32 log_child) {
    __shared__ uint4 xch[4][288];                       // per wave: 256 chunks of 16 bytes + 32 pad slots
    uint4 *__restrict__ layers = ts.t[blockIdx.y];
    const u32 lane = threadIdx.x & 63u;
    uint4 *x = xch[threadIdx.x >> 6];
    const size_t top0 = (size_t)blockIdx.x * 256u + (threadIdx.x & ~63u);        // the wave's first node of layer log_child - 2
    const u32 *cbase = (const u32 *)(layers + 2 * ((((size_t)1 << log_child) - 1) + 4 * top0));
    uint4 in[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = gload4(cbase, 4u * (64u * k + lane));
    Digest ch[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int k = 0; k < 4; k++) x[xslot(64u * k + lane)] = in[4 * h + k];
        asm volatile("" ::: "memory");
        if ((lane >> 5) == (u32)h) {                    // chunks 8 l .. 8 l + 7 of this half belong to lane 32 h + l
            const uint4 *mine = x + 9u * (lane & 31u);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint4 a = mine[2 * j], b = mine[2 * j + 1];
                ch[j] = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
            }
        }
        asm volatile("" ::: "memory");
    }
    const Digest l = hash_pair(ch[0], ch[1]);
    const Digest r = hash_pair(ch[2], ch[3]);
    const Digest top = hash_pair(l, r);
    // layer log_child - 1: the wave's 128 digests = 256 chunks; lane's chunks 4 lane .. 4 lane + 3
    {
        uint4 *mine = x + xslot(4u * lane);             // 4 lane + j, j < 4, stays inside one group of 8: same pad
        mine[0] = make_uint4(l.w[0], l.w[1], l.w[2], l.w[3]); mine[1] = make_uint4(l.w[4], l.w[5], l.w[6], l.w[7]);
        mine[2] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]); mine[3] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
    }
    asm volatile("" ::: "memory");
    uint4 o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = x[xslot(64u * k + lane)];
    asm volatile("" ::: "memory");
    {
        uint4 *mine = x + xslot(2u * lane);
        mine[0] = make_uint4(top.w[0], top.w[1], top.w[2], top.w[3]); mine[1] = make_uint4(top.w[4], top.w[5], top.w[6], top.w[7]);
    }
    asm volatile("" ::: "memory");
    uint4 o2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) o2[k] = x[xslot(64u * k + lane)];
    u32 *mid = (u32 *)(layers + 2 * ((((size_t)1 << (log_child - 1)) - 1) + 2 * top0));
    u32 *up = (u32 *)(layers + 2 * ((((size_t)1 << (log_child - 2)) - 1) + top0));
#pragma unroll
    for (int k = 0; k < 4; k++) gstore4(mid, 4u * (64u * k + lane), o[k]);
#pragma unroll
    for (int k = 0; k < 2; k++) gstore4(up, 4u * (64u * k + lane), o2[k]);
}

// Levels log_child-1 .. log_child-levels, 4 lanes per node: a workgroup of WG lanes owns WG/4 consecutive parents of the
// first level and everything above them (WG/4 -> 1 is log2(WG/4)+1 levels).  Children digests live in LDS between levels.
// the level loop shared by k_merkle_upq and k_merkle_leaf4_upq: `sh` holds the 2*active child digests of this workgroup
__device__ __forceinline__ void lds_only_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int WG>
__device__ __forceinline__ void upq_levels(uint4 *__restrict__ layers, u32 *sh, u32 log_child, u32 levels, u32 active, u32 blk) {
    const u32 t = threadIdx.x, q = t >> 2, j = t & 3;
    QuadMsgAddrs qa;                                               // this lane's 40 message-word addresses: the quad's slot sh[16q..16q+15]
    quad_msg_addrs(qa, (u32)(uintptr_t)(__attribute__((address_space(3))) u32 *)sh + 64u * q, j);
    for (u32 lv = 1; lv <= levels; lv++) {
        const u32 log_out = log_child - lv;
        u32 o_lo = 0, o_hi = 0;
        const bool on = q < active;                                // quad-uniform
        if (on) {
            b2s_quad_block64_lds(qa, j, o_lo, o_hi);
            u32 *out = reinterpret_cast<u32 *>(layers + 2 * (((size_t)1 << log_out) - 1) + 2 * ((size_t)blk * active + q));
            out[j] = o_lo;
            out[4 + j] = o_hi;
        }
        // LDS-only barriers: __syncthreads() also waits for the digest stores above to be acknowledged by memory (vmcnt(0)) —
        // nobody in this launch reads them back, and that wait was most of a level's time on this latency-bound path
        lds_only_barrier();                                        // every quad has read its children
        if (on) {
            sh[8 * q + j] = o_lo;
            sh[8 * q + 4 + j] = o_hi;
        }
        lds_only_barrier();
        active >>= 1;
    }
}
// The launch that produces a tree's root can run the channel's mix_root + draw_felt on it right away (wave 0, root still in LDS):
// the FRI commit loop's "tree, then channel" pair as one launch (ChanHook; null pointers: no channel step).
struct ChanHook { u32 *chan, *felt; };
__device__ __forceinline__ void chan_step_from_lds(const ChanHook &hk, const u32 *root_lds) {
    if (!hk.chan || threadIdx.x >= 64) return;
    u32 d[8], f[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = hk.chan[k];
    u32 n_chal = hk.chan[8], n_sent = hk.chan[9];
    chan_mix_draw(d, n_chal, n_sent, root_lds, true, hk.felt != nullptr, f);
    if (hk.felt && threadIdx.x < 4) hk.felt[threadIdx.x] = threadIdx.x == 0 ? f[0] : threadIdx.x == 1 ? f[1] : threadIdx.x == 2 ? f[2] : f[3];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) hk.chan[k] = d[k];
        hk.chan[8] = n_chal;
        hk.chan[9] = n_sent;
    }
}
template <int WG>
__global__ void __launch_bounds__(WG) k_merkle_upq(TreeSet ts, u32 log_child, u32 levels, ChanHook hk) {
    uint4 *__restrict__ layers = ts.t[blockIdx.y];
    constexpr u32 Q = WG / 4;
    __shared__ __attribute__((aligned(16))) u32 sh[Q * 16];      // 2Q child digests x 8 words
    const u32 t = threadIdx.x;
    const u32 active = min(Q, 1u << (log_child - 1));             // parents this workgroup produces at the first level
    {
        const uint4 *child = layers + 2 * (((size_t)1 << log_child) - 1) + (size_t)blockIdx.x * (4 * active);
        if (t < 4 * active) reinterpret_cast<uint4 *>(sh)[t] = child[t];      // 2*active digests = 4*active uint4
    }
    __syncthreads();
    upq_levels<WG>(layers, sh, log_child, levels, active, blockIdx.x);
    if (log_child == levels) chan_step_from_lds(hk, sh);          // this launch reached layer 0: the root is sh[0..7]
}
// One leaf of a 4-column tree (a 16-byte message, vcs/blake2_merkle.ts:9-24): hashed, written to the leaf layer (node `node` of
// layer log_leaf) and to LDS as child digest `slot` of the quad levels that follow.
__device__ __forceinline__ void leaf4_to_lds(uint4 *layers, u32 log_leaf, size_t node, u32 *sh, u32 slot, u32 m0, u32 m1, u32 m2, u32 m3) {
    u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
    const u32 m[16] = {m0, m1, m2, m3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    b2s_compress(h, m, 16u, true);
    uint4 *leaf = layers + 2 * ((((size_t)1 << log_leaf) - 1) + node);
    const uint4 lo = make_uint4(h[0], h[1], h[2], h[3]), hi = make_uint4(h[4], h[5], h[6], h[7]);
    leaf[0] = lo; leaf[1] = hi;
    reinterpret_cast<uint4 *>(sh)[2 * slot] = lo;
    reinterpret_cast<uint4 *>(sh)[2 * slot + 1] = hi;
}
// A small 4-column tree (every FRI layer below 2^17 rows) without a launch of its own for the leaves: the first 2*active lanes
// of the workgroup hash one leaf each (16-byte message, vcs/blake2_merkle.ts:9-24), write it to the leaf layer and to LDS,
// and the quad levels follow in the same launch.
template <int WG, bool FOLD>
__global__ void __launch_bounds__(WG) k_merkle_leaf4_upq(u32 *__restrict__ c0, u32 *__restrict__ c1, u32 *__restrict__ c2, u32 *__restrict__ c3,
                                                        uint4 *__restrict__ layers, u32 log_leaf, u32 levels, ChanHook hk, FoldSpec fs) {
    constexpr u32 Q = WG / 4;
    __shared__ __attribute__((aligned(16))) u32 sh[Q * 16];
    const u32 t = threadIdx.x;
    const u32 active = min(Q, 1u << (log_leaf - 1));              // parents of the first level in this workgroup
    if (t < 2 * active) {
        const size_t node = (size_t)blockIdx.x * (2 * active) + t;
        u32 m0, m1, m2, m3;
        if (FOLD) {
            const qm31 r = fold_row(fold_row_load(fs, node), {fs.alpha[0], fs.alpha[1], fs.alpha[2], fs.alpha[3]});
            m0 = r.a; m1 = r.b; m2 = r.c; m3 = r.d;
            gstore1(c0 + node, m0); gstore1(c1 + node, m1); gstore1(c2 + node, m2); gstore1(c3 + node, m3);
        } else {
            m0 = c0[node]; m1 = c1[node]; m2 = c2[node]; m3 = c3[node];
        }
        leaf4_to_lds(layers, log_leaf, node, sh, t, m0, m1, m2, m3);
    }
    __syncthreads();
    upq_levels<WG>(layers, sh, log_leaf, levels, active, blockIdx.x);
    if (log_leaf == levels) chan_step_from_lds(hk, sh);
}

__global__ void __launch_bounds__(64) k_channel_mix_draw(u32 *__restrict__ chan, const u32 *__restrict__ root, u32 *__restrict__ felt,
                                                        u32 do_mix, u32 do_draw) {
    u32 d[8], f[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = chan[k];
    u32 n_chal = chan[8], n_sent = chan[9];
    chan_mix_draw(d, n_chal, n_sent, root, do_mix != 0, do_draw != 0, f);
    if (do_draw && threadIdx.x < 4) {
        u32 v = f[0];
        v = threadIdx.x == 1 ? f[1] : v;
        v = threadIdx.x == 2 ? f[2] : v;
        v = threadIdx.x == 3 ? f[3] : v;
        felt[threadIdx.x] = v;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) chan[k] = d[k];
        chan[8] = n_chal;
        chan[9] = n_sent;
    }
}

// ---- FRI commit tail: every layer from 2^log0 <= 2^9 rows down to the last one in ONE launch of one workgroup.  Per layer the
// host loop costs three launches (tree, channel, fold) of a few microseconds of work each plus the gaps between dependent
// kernels; here a layer is: the 4-column tree in LDS (leaves one per lane, levels by quads: the k_merkle_leaf4_upq body), the
// channel's mix_root + draw_felt by wave 0 (state kept in its registers across the layers), fold_line by the first 2^(lg-1)
// lanes.  Evaluations and trees go to the same buffers, in the same layouts, as the per-layer path.
struct FriTail {
    u32 *eval[11][4];        // eval[0]: the input evaluation (2^log0 rows, already folded); eval[i + 1]: output of fold i
    uint4 *tree[10];         // tree[i]: layers buffer of the tree over eval[i]
    u32 n_layers, log0;
    const u32 *pre[4];       // non-null: eval[0] is still to be computed — the fold_line of this evaluation of 2^(log0+1) rows with
    const u32 *pre_alpha;    // the alpha at pre_alpha (drawn by an earlier launch); the kernel writes eval[0]
};
__global__ void __launch_bounds__(1024) k_fri_tail(FriTail ft, const u32 *__restrict__ itw, u32 tw_log, u32 *__restrict__ chan,
                                                  u32 *__restrict__ alphas) {
    constexpr u32 Q = 256;
    __shared__ __attribute__((aligned(16))) u32 sh[Q * 16];
    __shared__ __attribute__((aligned(16))) u32 evl[4][512];         // the current layer's evaluation, coordinate-major
    __shared__ u32 alpha_sh[4];
    const u32 t = threadIdx.x;
    u32 d[8], n_chal = 0, n_sent = 0;
    if (t < 64) {
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = chan[k];
        n_chal = chan[8]; n_sent = chan[9];
    }
    // Between the layers the evaluation never goes through memory: row t of the next layer is computed by lane t — the lane that
    // hashes leaf t of the next tree (registers) — and the fold reads rows 2t, 2t+1 from LDS.  (The first form read the folded
    // rows back from global memory behind a device-scope fence, twice per layer: most of a layer's time outside its tree levels.)
    u32 row[4] = {0u, 0u, 0u, 0u};
    if (t < (1u << ft.log0)) {
        if (ft.pre_alpha) {          // the fold into the first layer of the tail rides along (one launch fewer)
            const qm31 alpha = *reinterpret_cast<const qm31 *>(ft.pre_alpha);
            const u32 tw0 = gload1(itw + ((size_t)1 << tw_log) - ((size_t)2 << ft.log0) + t);
            const uint2 a = gload2(ft.pre[0] + 2 * t), b = gload2(ft.pre[1] + 2 * t), c = gload2(ft.pre[2] + 2 * t), e = gload2(ft.pre[3] + 2 * t);
            const qm31 f0 = {m31_add(a.x, a.y), m31_add(b.x, b.y), m31_add(c.x, c.y), m31_add(e.x, e.y)};
            const qm31 f1 = qm31_mul_m31({m31_sub(a.x, a.y), m31_sub(b.x, b.y), m31_sub(c.x, c.y), m31_sub(e.x, e.y)}, tw0);
            const qm31 r0 = qm31_add(f0, qm31_mul(alpha, f1));
            row[0] = r0.a; row[1] = r0.b; row[2] = r0.c; row[3] = r0.d;
#pragma unroll
            for (int c2 = 0; c2 < 4; c2++) { gstore1(ft.eval[0][c2] + t, row[c2]); evl[c2][t] = row[c2]; }
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) { row[c] = gload1(ft.eval[0][c] + t); evl[c][t] = row[c]; }
        }
    }
    for (u32 i = 0; i < ft.n_layers; i++) {
        const u32 lg = ft.log0 - i;                                  // 1 <= lg <= 9
        uint4 *layers = ft.tree[i];
        const u32 active = 1u << (lg - 1);
        // the fold's x^-1 of this layer: requested now, used behind the tree and the channel step
        const u32 tw = t < active ? gload1(itw + ((size_t)1 << tw_log) - ((size_t)1 << lg) + t) : 0u;
        // tree over the 4 coordinate columns (vcs/blake2_merkle.ts:9-24): leaves, then all levels
        if (t < 2 * active) leaf4_to_lds(layers, lg, t, sh, t, row[0], row[1], row[2], row[3]);
        lds_only_barrier();
        upq_levels<1024>(layers, sh, lg, lg, active, 0u);            // the root is in sh[0..7] afterwards
        // channel: mix the root, draw alpha (wave 0; channel/blake2.ts:115-184, Rust draw semantics)
        if (t < 64) {
            u32 f[4];
            chan_mix_draw(d, n_chal, n_sent, sh, true, true, f);
            if (t < 4) {
                const u32 v = t == 0 ? f[0] : t == 1 ? f[1] : t == 2 ? f[2] : f[3];
                alpha_sh[t] = v;
                alphas[4 * i + t] = v;
            }
        }
        lds_only_barrier();
        // fold_line (fri.ts:120-152): row t of the next evaluation from rows 2t, 2t + 1 of this one
        qm31 r = {0u, 0u, 0u, 0u};
        if (t < active) {
            const qm31 alpha = {alpha_sh[0], alpha_sh[1], alpha_sh[2], alpha_sh[3]};
            const uint2 a = *reinterpret_cast<const uint2 *>(&evl[0][2 * t]), b = *reinterpret_cast<const uint2 *>(&evl[1][2 * t]),
                        c = *reinterpret_cast<const uint2 *>(&evl[2][2 * t]), e = *reinterpret_cast<const uint2 *>(&evl[3][2 * t]);
            const qm31 f0 = {m31_add(a.x, a.y), m31_add(b.x, b.y), m31_add(c.x, c.y), m31_add(e.x, e.y)};
            const qm31 f1 = qm31_mul_m31({m31_sub(a.x, a.y), m31_sub(b.x, b.y), m31_sub(c.x, c.y), m31_sub(e.x, e.y)}, tw);
            r = qm31_add(f0, qm31_mul(alpha, f1));
            gstore1(ft.eval[i + 1][0] + t, r.a); gstore1(ft.eval[i + 1][1] + t, r.b);
            gstore1(ft.eval[i + 1][2] + t, r.c); gstore1(ft.eval[i + 1][3] + t, r.d);
        }
        lds_only_barrier();              // every lane has read its two rows of this layer
        if (t < active) { evl[0][t] = r.a; evl[1][t] = r.b; evl[2][t] = r.c; evl[3][t] = r.d; }
        row[0] = r.a; row[1] = r.b; row[2] = r.c; row[3] = r.d;
        lds_only_barrier();
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) chan[k] = d[k];
        chan[8] = n_chal;
        chan[9] = n_sent;
    }
}

// Proof-of-work grind: lane i of a batch tests nonce base + i; digest' = Blake2s(digest || LE64(nonce)) is one 40-byte block.
struct GrindDigest { u32 w[8]; };
__global__ void __launch_bounds__(256) k_grind(GrindDigest d, u32 pow_bits, unsigned long long base, unsigned long long count,
                                              unsigned long long *__restrict__ best) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned long long nonce = base + i;
    u32 m[16] = {d.w[0], d.w[1], d.w[2], d.w[3], d.w[4], d.w[5], d.w[6], d.w[7], (u32)nonce, (u32)(nonce >> 32), 0, 0, 0, 0, 0, 0};
    u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
    b2s_compress(h, m, 40u, true);
    u32 tz = 0;                                   // trailing zeros of the first 16 bytes as a little-endian u128
    if (h[0]) tz = __ffs(h[0]) - 1;
    else if (h[1]) tz = 32 + __ffs(h[1]) - 1;
    else if (h[2]) tz = 64 + __ffs(h[2]) - 1;
    else if (h[3]) tz = 96 + __ffs(h[3]) - 1;
    else tz = 128;
    if (tz >= pow_bits) atomicMin(best, nonce);
}

// ---- host.  merkle_plan.h decides; what follows checks pointers, asks for the plan and issues it.
static_assert(kMerkleMaxHashCols == kMaxHashCols && kMerkleCapDefault == Knobs{}.merkle_cap && kMerklePairLogDefault == Knobs{}.merkle_pair_log,
              "merkle_plan.h restates common.h's constants");

// The pointers of one tree of a call.  layers: its layers buffer, layer k at byte 32 (2^k - 1).  tstwo_merkle_commit_layer has no
// such buffer: `out` is its one layer, `prev` that layer's children, and every column belongs to the layer (log_sizes is null).
struct TreePtrs {
    const u32 *const *cols;
    const u32 *log_sizes;
    size_t n_cols;
    uint8_t *layers, *out;
    const uint8_t *prev;
};

MerkleEnv plan_env() { return {(u32)ctx().n_cus, knobs().merkle_cap, knobs().merkle_pair_log}; }

// What the plan reads of a tree.  A request with a null pointer (null_arg) is not looked into.
MerkleTree shape_of(const TreePtrs &t) {
    MerkleTree m = {t.log_sizes, t.n_cols, true, aligned16(t.layers), !t.layers || !t.cols || !t.log_sizes};
    if (m.null_arg) return m;
    u32 max_log = 0;
    for (size_t i = 0; i < t.n_cols; i++) max_log = t.log_sizes[i] > max_log ? t.log_sizes[i] : max_log;
    for (size_t i = 0; i < t.n_cols; i++)
        if (t.log_sizes[i] == max_log && ((uintptr_t)t.cols[i] & 7)) m.cols_aligned8 = false;
    return m;
}

// The steps of the call being served: one vector for the life of the library, so that a commit allocates nothing for its plan.
std::vector<MerkleStep> &plan_steps() {
    static std::vector<MerkleStep> steps;
    steps.clear();
    return steps;
}

int plan_error(const char *why) { return why ? set_error(why == kMerkleFoldNotCarried ? TSTWO_ERR_HIP : TSTWO_ERR_BAD_ARG, why) : TSTWO_OK; }

// The pointers a tree committed on its own must have.
int check_tree(const TreePtrs &t) {
    if (!t.layers) return set_error(TSTWO_ERR_BAD_ARG, "merkle: null layers buffer");
    if (t.n_cols && !t.log_sizes) return set_error(TSTWO_ERR_BAD_ARG, "merkle: null log size table");
    TSTWO_REQUIRE_TABLE(t.cols, t.n_cols);
    return TSTWO_OK;
}

// Issues every step of a plan.  trees: the pointers the plan's tree numbers refer to; fold / hook: what the steps that carry the
// fold / take the channel step are given.
int run_plan(const std::vector<MerkleStep> &steps, const TreePtrs *trees, const FoldSpec *fold, const ChanHook &hook) {
    hipStream_t stream = ctx().stream;
    for (const MerkleStep &s : steps) {
        const TreePtrs &t = trees[s.tree];
        const dim3 grid(s.grid, s.n_trees), wg(s.wg);
        const size_t n_nodes = (size_t)1 << s.log;
        TreeSet ts = {}, at = {};                        // every tree's layers buffer, and its layer s.log in it
        for (u32 r = 0; r < s.n_trees; r++) {
            ts.t[r] = (uint4 *)trees[s.tree + r].layers;
            at.t[r] = t.out ? (uint4 *)t.out : ts.t[r] + 2 * (n_nodes - 1);
        }
        const auto children = [&] { return t.out ? (const uint4 *)t.prev : ts.t[0] + 2 * (2 * n_nodes - 1); };      // of layer s.log
        HashColPtrs hp;                                 // the columns read: s.n_cols from the s.col0-th column of log size s.log, tree after tree
        u32 n = 0;
        for (u32 r = 0; r < s.n_trees && s.n_cols; r++) {
            const TreePtrs &q = trees[s.tree + r];
            u32 skip = s.col0;
            for (size_t i = 0; i < q.n_cols && n < (r + 1) * s.n_cols; i++) {
                if (q.log_sizes && q.log_sizes[i] != s.log) continue;
                if (skip) skip--;
                else hp.p[n++] = q.cols[i];
            }
        }
        const ChanHook hk = s.hook ? hook : ChanHook{nullptr, nullptr};
        switch (s.kind) {
            case MerkleStep::LEAF_STATIC:
                switch (s.n_cols / 16) {
                    case 1: hipLaunchKernelGGL(k_merkle_leaf_static<1>, grid, wg, 0, stream, hp, at, n_nodes); break;
                    case 2: hipLaunchKernelGGL(k_merkle_leaf_static<2>, grid, wg, 0, stream, hp, at, n_nodes); break;
                    case 3: hipLaunchKernelGGL(k_merkle_leaf_static<3>, grid, wg, 0, stream, hp, at, n_nodes); break;
                    default: hipLaunchKernelGGL(k_merkle_leaf_static<4>, grid, wg, 0, stream, hp, at, n_nodes); break;
                }
                break;
            case MerkleStep::LEAF_PAIR:
                switch (s.n_cols / 16) {
                    case 1: hipLaunchKernelGGL((k_merkle_leaf_pair<1, kPairNT>), grid, wg, 0, stream, hp, at, n_nodes / 2); break;
                    case 2: hipLaunchKernelGGL((k_merkle_leaf_pair<2, kPairNT>), grid, wg, 0, stream, hp, at, n_nodes / 2); break;
                    case 3: hipLaunchKernelGGL((k_merkle_leaf_pair<3, kPairNT>), grid, wg, 0, stream, hp, at, n_nodes / 2); break;
                    default: hipLaunchKernelGGL((k_merkle_leaf_pair<4, kPairNT>), grid, wg, 0, stream, hp, at, n_nodes / 2); break;
                }
                break;
            case MerkleStep::LEAF4:
            case MerkleStep::LEAF4_UPQ: {
                u32 *w0 = const_cast<u32 *>(hp.p[0]), *w1 = const_cast<u32 *>(hp.p[1]), *w2 = const_cast<u32 *>(hp.p[2]), *w3 = const_cast<u32 *>(hp.p[3]);
                const FoldSpec fs = s.fold ? *fold : FoldSpec{};
                if (s.kind == MerkleStep::LEAF4) {
                    const auto kernel = s.fold ? k_merkle_leaf4<true> : k_merkle_leaf4<false>;
                    hipLaunchKernelGGL(kernel, grid, wg, 0, stream, w0, w1, w2, w3, at.t[0], n_nodes, fs);
                } else {
                    const auto kernel = s.wg == 1024 ? (s.fold ? k_merkle_leaf4_upq<1024, true> : k_merkle_leaf4_upq<1024, false>)
                                                     : (s.fold ? k_merkle_leaf4_upq<256, true> : k_merkle_leaf4_upq<256, false>);
                    hipLaunchKernelGGL(kernel, grid, wg, 0, stream, w0, w1, w2, w3, ts.t[0], s.log, s.levels, hk, fs);
                }
                break;
            }
            case MerkleStep::LAYER: {
                const LayerParams lp = {s.lp.total_words, s.lp.w_begin, s.lp.w_end, s.lp.col_word0, s.lp.n_cols, s.lp.load_state, s.lp.is_final};
                if (s.has_prev) hipLaunchKernelGGL(k_merkle_layer<true>, grid, wg, 0, stream, children(), hp, at.t[0], n_nodes, lp);
                else hipLaunchKernelGGL(k_merkle_layer<false>, grid, wg, 0, stream, (const uint4 *)nullptr, hp, at.t[0], n_nodes, lp);
                break;
            }
            case MerkleStep::INNER: hipLaunchKernelGGL(k_merkle_inner, grid, wg, 0, stream, children(), at.t[0], n_nodes); break;
            case MerkleStep::INNER_SET: hipLaunchKernelGGL(k_merkle_inner_set, grid, wg, 0, stream, ts, s.log); break;
            case MerkleStep::SUBTREE2C: hipLaunchKernelGGL(k_merkle_subtree2c, grid, wg, 0, stream, ts, s.log); break;
            case MerkleStep::UPQ: {
                const auto kernel = s.wg == 1024 ? k_merkle_upq<1024> : k_merkle_upq<256>;
                hipLaunchKernelGGL(kernel, grid, wg, 0, stream, ts, s.log, s.levels, hk);
                break;
            }
            case MerkleStep::CHANNEL: {                  // no launch of the tree took the step
                int rc = tstwo_channel_mix_root_draw_felt(hook.chan, t.layers, hook.felt);
                if (rc) return rc;
                break;
            }
        }
    }
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// tstwo_merkle_commit, with the two steps of a FRI commit layer that can ride on the tree's launches.  fold (null: none): the
// tree's 4 columns are first written as that fold, inside the leaf launch.  hook (chan null: none): the channel step on the root.
int commit_tree(const u32 *const *cols, const u32 *log_sizes, size_t n_cols, uint8_t *layers, uint8_t root[32], const FoldSpec *fold,
                const ChanHook &hook) {
    TSTWO_REQUIRE_READY();
    const TreePtrs t = {cols, log_sizes, n_cols, layers, nullptr, nullptr};
    std::vector<MerkleStep> &steps = plan_steps();
    int rc = check_tree(t);
    if (rc == TSTWO_OK) rc = plan_error(merkle_plan_tree(shape_of(t), fold != nullptr, hook.chan != nullptr, plan_env(), 0, steps));
    if (rc == TSTWO_OK) rc = run_plan(steps, &t, fold, hook);
    if (rc) return rc;
    return root ? small_d2h(root, layers, 32) : TSTWO_OK;
}
}  // namespace

namespace tstwo {
// fri.hip's commit loop: tstwo_merkle_commit(…) followed by mix_root + draw_felt on its root, the channel step riding on the tree's
// last launch when that launch is a single workgroup (every FRI layer's tree), a k_channel_mix_draw launch otherwise.
int merkle_commit_then_channel(const u32 *const *cols, const u32 *log_sizes, size_t n_cols, uint8_t *layers, u32 *chan, u32 *felt,
                               const u32 *const *fold_in, const u32 *inv_x, const u32 *alpha_dev) {
    FoldSpec fs = {};
    if (fold_in) fs = {{fold_in[0], fold_in[1], fold_in[2], fold_in[3]}, inv_x, alpha_dev};
    return commit_tree(cols, log_sizes, n_cols, layers, nullptr, fold_in ? &fs : nullptr, {chan, felt});
}
// fri.hip's commit loop hands the layers from 2^log0 <= 2^9 rows down to the last one to k_fri_tail (see there).
int launch_fri_tail(u32 *const (*eval)[4], uint8_t *const *trees, u32 n_layers, u32 log0, const u32 *itw, u32 tw_log, u32 *chan, u32 *alphas,
                    const u32 *const *pre, const u32 *pre_alpha) {
    if (n_layers == 0 || n_layers > 10 || log0 < n_layers || log0 > 9 || log0 - n_layers + 1 < 1)
        return set_error(TSTWO_ERR_BAD_ARG, "fri tail: layer range out of bounds");
    FriTail ft = {};
    for (u32 i = 0; i <= n_layers; i++)
        for (int k = 0; k < 4; k++) ft.eval[i][k] = eval[i][k];
    for (u32 i = 0; i < n_layers; i++) ft.tree[i] = (uint4 *)trees[i];
    ft.n_layers = n_layers;
    ft.log0 = log0;
    if (pre && pre_alpha) {
        if (tw_log > 31 || log0 + 1 > tw_log) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");
        for (int k = 0; k < 4; k++) ft.pre[k] = pre[k];
        ft.pre_alpha = pre_alpha;
    }
    hipLaunchKernelGGL(k_fri_tail, dim3(1), dim3(1024), 0, ctx().stream, ft, itw, tw_log, chan, alphas);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}
}  // namespace tstwo

extern "C" {

size_t tstwo_merkle_layers_bytes(u32 max_log) { return 32u * (((size_t)2 << max_log) - 1); }

int tstwo_grind_blake2s(const uint8_t digest[32], u32 pow_bits, uint64_t start_nonce, uint64_t *nonce_out) {
    TSTWO_REQUIRE_READY();
    if (!digest || !nonce_out) return set_error(TSTWO_ERR_BAD_ARG, "grind: null argument");
    if (pow_bits > 128) return set_error(TSTWO_ERR_BAD_ARG, "grind: pow_bits > 128");
    Context &c = ctx();
    int rc = ensure_scratch(64);
    if (rc) return rc;
    unsigned long long *best = (unsigned long long *)c.scratch;
    GrindDigest d;
    for (int i = 0; i < 8; i++)
        d.w[i] = (u32)digest[4 * i] | ((u32)digest[4 * i + 1] << 8) | ((u32)digest[4 * i + 2] << 16) | ((u32)digest[4 * i + 3] << 24);
    const unsigned long long none = kGrindNone;
    for (GrindSearch s = grind_begin(GRIND_BLAKE2S, start_nonce); grind_next(s);) {      // grind_plan.h
        TSTWO_HIP(hipMemsetAsync(best, 0xFF, sizeof(none), c.stream));      // none = all ones
        hipLaunchKernelGGL(k_grind, dim3((unsigned)((s.batch + kGrindLanes - 1) / kGrindLanes)), dim3(kGrindLanes), 0, c.stream, d, pow_bits,
                           (unsigned long long)s.base, (unsigned long long)s.batch, best);
        TSTWO_LAUNCH_CHECK();
        unsigned long long found = none;
        { int rc2 = small_d2h(&found, best, sizeof(found)); if (rc2) return rc2; }
        if (found != none) { *nonce_out = found; return TSTWO_OK; }
    }
    return set_error(TSTWO_ERR_BAD_ARG, "grind: nonce space exhausted");
}

// Device-resident Blake2sChannel (state: 10 words = digest[8], n_challenges, n_sent).  root: 32 bytes in device memory
// (e.g. offset 0 of a tstwo_merkle_commit layers buffer) or NULL to skip the mix; felt: 4 words in device memory or NULL
// to skip the draw.  Nothing is synchronised: the next kernel on the stream can consume `felt`.
int tstwo_channel_mix_root_draw_felt(u32 *chan, const uint8_t *root, u32 *felt) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(chan);
    if ((((uintptr_t)root) & 3) || (((uintptr_t)felt) & 3)) return set_error(TSTWO_ERR_BAD_ARG, "channel: unaligned pointer");
    hipLaunchKernelGGL(k_channel_mix_draw, dim3(1), dim3(64), 0, ctx().stream, chan, (const u32 *)root, felt, root ? 1u : 0u, felt ? 1u : 0u);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_merkle_commit_layer(u32 log_size, const uint8_t *prev, const u32 *const *cols, size_t n_cols, uint8_t *out) {
    TSTWO_REQUIRE_READY();
    if (n_cols && !cols) return set_error(TSTWO_ERR_BAD_ARG, "merkle: null column table");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    if (!out && log_size <= 31) return set_error(TSTWO_ERR_BAD_ARG, "merkle: null output layer");      // (the plan reports a log size out of range)
    const TreePtrs t = {cols, nullptr, n_cols, nullptr, out, prev};
    std::vector<MerkleStep> &steps = plan_steps();
    int rc = plan_error(merkle_plan_layer(log_size, prev != nullptr, n_cols, false, aligned16(out) && aligned16(prev), plan_env(), 0, steps));
    return rc ? rc : run_plan(steps, &t, nullptr, {});
}

int tstwo_merkle_commit(const u32 *const *cols, const u32 *log_sizes, size_t n_cols, uint8_t *layers, uint8_t root[32]) {
    return commit_tree(cols, log_sizes, n_cols, layers, root, nullptr, {});
}

// Several trees in ONE launch sequence (a TreeVec committed together: the 8 trees of BASELINE config 5's trace on one GPU,
// pcs/prover.ts:62-64).  A tree ends in ~65 us of launches with almost nothing to do (the layers below 2^19 nodes: 1 M of a
// 32-column log-22 tree's 12.6 M compressions); committed one after the other, 8 trees pay that 8 times.  When the trees
// have ONE shape that the static leaf kernel serves (16 / 32 / 48 / 64 columns of one log size, at most 8 trees and 256
// columns in all), every launch covers all trees (blockIdx.y = tree) and the tails run side by side; any other input is
// committed tree by tree.  Bit-identical to tstwo_merkle_commit per tree (same kernels, same nodes).
int tstwo_merkle_commit_many(const tstwo_commit_request *reqs, size_t n_trees, uint8_t *roots) {
    TSTWO_REQUIRE_READY();
    if (n_trees && !reqs) return set_error(TSTWO_ERR_BAD_ARG, "merkle: null request table");
    std::vector<TreePtrs> trees(n_trees);
    std::vector<MerkleTree> shapes(n_trees);
    for (size_t r = 0; r < n_trees; r++) {
        trees[r] = {reqs[r].cols, reqs[r].log_sizes, reqs[r].n_cols, reqs[r].layers, nullptr, nullptr};
        shapes[r] = shape_of(trees[r]);
    }
    // which pointers must be there depends on the path: the rule is asked first, then the whole plan (which asks it again)
    bool uniform = false;
    u32 lg = 0;
    int rc = plan_error(merkle_set_uniform(shapes.data(), n_trees, &uniform, &lg));
    for (size_t r = 0; r < n_trees && rc == TSTWO_OK; r++) {
        if (uniform) TSTWO_REQUIRE_TABLE(trees[r].cols, trees[r].n_cols);
        else rc = check_tree(trees[r]);
    }
    std::vector<MerkleStep> &steps = plan_steps();
    if (rc == TSTWO_OK) rc = plan_error(merkle_plan_set(shapes.data(), n_trees, plan_env(), steps));
    if (rc == TSTWO_OK) rc = run_plan(steps, trees.data(), nullptr, {});
    if (rc) return rc;
    if (!roots) return TSTWO_OK;
    std::vector<const uint8_t *> bufs(n_trees);
    for (size_t r = 0; r < n_trees; r++) bufs[r] = reqs[r].layers;
    return download_roots(bufs.data(), n_trees, roots);
}

}  // extern "C"

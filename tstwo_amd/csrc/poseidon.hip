// poseidon.hip — the Poseidon252 Merkle channel on the device: hash_many, MerkleOps<FieldElement252>.commitOnLayer
// (backend/cpu/poseidon252.ts:44-78), MerkleProver.commit over Poseidon252 and the proof-of-work grind (backend/cpu/grind.ts:31-42
// over Poseidon252Channel).  One lane computes one hash; the field arithmetic and the Hades permutation are in felt252.cuh.
//
// hash_many(v) (Starknet's poseidon_hash_many): append 1, then 0 if the length is odd; from s = (0, 0, 0), per pair (x, y):
// s0 += x, s1 += y, permute; the hash is s0.  hashNode (vcs/poseidon252_merkle.ts:22-58) hashes [left, right (if any)] + one
// element per 8 columns (felt252.cuh: pack_m31x8, zero-padded), so a node with children only costs 2 permutations and a
// 32-column leaf 3.
//
// Elements in device memory are 8 little-endian u32 limbs, canonical: 32 bytes, so a Poseidon tree has exactly the layout of
// tstwo_merkle_commit (layer k at byte 32 (2^k - 1), root first) and the decommit / gather entries of decommit.hip serve it as is.
#include <algorithm>

#include "common.h"
#include "felt252.cuh"
#include "grind_plan.h"

using namespace tstwo;
using felt::F;

namespace {

constexpr int kThreads = 256;
// Layers of at most 2^kTailLog nodes with no columns joining at or below them are hashed by ONE single-workgroup launch
// (k_p252_tail): one launch instead of kTailLog + 1.  A layer costs ~2 permutations of latency either way, so the saving is the
// launch gaps.
constexpr u32 kTailLog = 8;

__device__ __forceinline__ F load_felt(const u32 *p) {
    const uint4 a = gload4(p), b = gload4(p + 4);
    F r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}

__device__ __forceinline__ void store_felt(u32 *p, const F &x) {
    gstore4(p, make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]));
    gstore4(p + 4, make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]));
}

// hash_many over n_in elements, element e = elem(e) (canonical, wave-uniform e): the sponge above.  The pair loop is not
// unrolled, so the permutation is inlined once per kernel.
template <class Elem>
__device__ __forceinline__ F sponge(u32 n_in, const Elem &elem) {
    F s0 = felt::zero(), s1 = felt::zero(), s2 = felt::zero();
    const u32 pairs = (n_in + 2u) / 2u;            // n_in + 1 elements padded to an even count
#pragma unroll 1
    for (u32 q = 0; q < pairs; q++) {
        const u32 e = 2u * q;
        F x, y;
        if (e < n_in) x = felt::to_mont(elem(e));
        else x = felt::one_mont();                  // e == n_in: the appended 1
        if (e + 1u < n_in) y = felt::to_mont(elem(e + 1u));
        else if (e + 1u == n_in) y = felt::one_mont();
        else y = felt::zero();                      // the padding 0
        s0 = felt::add(s0, x);
        s1 = felt::add(s1, y);
        felt::hades(s0, s1, s2);
    }
    return felt::from_mont(s0);
}

// tstwo_poseidon252_hash_many: lane i hashes message i = in[i k .. i k + k) (elements of 8 words).
__global__ void __launch_bounds__(kThreads) k_p252_hash_many(const u32 *__restrict__ in, size_t n, u32 k, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const u32 *msg = in + i * k * 8;
    const F h = sponge(k, [&](u32 e) { return load_felt(msg + 8 * (size_t)e); });
    store_felt(out + 8 * i, h);
}

// Column block b of node `node` (wave-uniform b): columns 8b .. 8b + 7, absent ones zero.  Column pointers are wave-uniform
// (scalar loads from the kernel-argument table or the device table), each lane reads its own row: coalesced.
__device__ __forceinline__ F column_block(const ColPtrs &cols, u32 n_cols, u32 b, size_t node) {
    u32 w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u32 ci = 8u * b + (u32)k;
        w[k] = ci < n_cols ? gload1(colp_u(cols, ci) + node) : 0u;
    }
    return felt::pack_m31x8(w);
}

// commitOnLayer: node i = hashNode((prev[2i], prev[2i+1]) if HAS_PREV, cols[..][i]).  With no columns this is the children-only
// node: 2 permutations.
template <bool HAS_PREV>
__global__ void __launch_bounds__(kThreads) k_p252_layer(ColPtrs cols, u32 n_cols, const u32 *__restrict__ prev, u32 *__restrict__ out,
                                                         size_t n_nodes) {
    const size_t node = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (node >= n_nodes) return;
    const u32 nch = HAS_PREV ? 2u : 0u;
    const u32 n_in = nch + (n_cols + 7u) / 8u;
    const F h = sponge(n_in, [&](u32 e) {
        if (HAS_PREV && e < 2u) return load_felt(prev + 8 * (2 * node + e));
        return column_block(cols, n_cols, e - nch, node);
    });
    store_felt(out + 8 * node, h);
}

// The column-free top of a tree in one launch of one workgroup: layers log_child - 1 .. 0 of the tstwo_merkle_commit layout,
// children of the first from memory, of the others from LDS (written by this workgroup one barrier earlier).
__global__ void __launch_bounds__(kThreads) k_p252_tail(u32 *__restrict__ layers, u32 log_child) {
    __shared__ u32 lds[(2u << kTailLog) * 8 + (1u << kTailLog) * 8];   // children (<= 2^(kTailLog+1) nodes) | outputs (<= 2^kTailLog)
    const u32 t = threadIdx.x;
    const u32 n_child = 1u << log_child;
    const u32 *src = layers + 8 * (size_t)(n_child - 1);
    for (u32 w = t; w < 8 * n_child; w += kThreads) lds[w] = src[w];
    __syncthreads();
    u32 src_off = 0, dst_off = (2u << kTailLog) * 8;
    for (int lg = (int)log_child - 1; lg >= 0; lg--) {
        const u32 n = 1u << lg;
        if (t < n) {
            const F h = sponge(2u, [&](u32 e) {
                F c;
#pragma unroll
                for (int k = 0; k < 8; k++) c.v[k] = lds[src_off + 8 * (2 * t + e) + k];
                return c;
            });
            store_felt(layers + 8 * (size_t)(n - 1) + 8 * t, h);
#pragma unroll
            for (int k = 0; k < 8; k++) lds[dst_off + 8 * t + k] = h.v[k];
        }
        __syncthreads();
        const u32 s = src_off;
        src_off = dst_off;
        dst_off = s;
    }
}

// Grind: lane i of a batch tests nonce base + i.  mix_u64(nonce) on a Poseidon252Channel is mix_u32s([0,0,0,0,0,hi,lo]) =
// hash_many([digest, nonce]) (one element: 7 words, no padding), i.e. 2 permutations.
struct FeltArg { u32 v[8]; };
__global__ void __launch_bounds__(kThreads) k_p252_grind(FeltArg d, u32 pow_bits, unsigned long long base, unsigned long long count,
                                                         unsigned long long *__restrict__ best) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const unsigned long long nonce = base + i;
    const F h = sponge(2u, [&](u32 e) {
        F x;
        if (e == 0u) {
#pragma unroll
            for (int k = 0; k < 8; k++) x.v[k] = d.v[k];
        } else {
            x = felt::zero();
            x.v[0] = (u32)nonce;
            x.v[1] = (u32)(nonce >> 32);
        }
        return x;
    });
    if (felt::trailing_zeros(h) >= pow_bits) atomicMin(best, nonce);
}

int fill_cols(ColPtrs &cp, const u32 *const *cols, size_t n_cols) {
    if (n_cols == 0) {
        for (int k = 0; k < kMaxColsPerLaunch; k++) cp.p[k] = nullptr;
        cp.ext = nullptr;
        return TSTWO_OK;
    }
    return fill_col_table(cp, cols, n_cols, 0);
}

int p252_commit_layer(u32 log_size, const uint8_t *prev, const u32 *const *cols, size_t n_cols, uint8_t *out) {
    if (log_size > 30) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: log size out of range");
    if (!out) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null output layer");
    if (!aligned16(out) || !aligned16(prev)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: layers must be 16-byte aligned");
    if (n_cols > 0xFFFFFFF0u) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: too many columns");
    ColPtrs cp;
    if (int rc = fill_cols(cp, cols, n_cols)) return rc;
    const size_t n_nodes = (size_t)1 << log_size;
    const dim3 grid(ceil_div(n_nodes, kThreads));
    if (prev)
        hipLaunchKernelGGL(k_p252_layer<true>, grid, dim3(kThreads), 0, ctx().stream, cp, (u32)n_cols, (const u32 *)prev, (u32 *)out, n_nodes);
    else
        hipLaunchKernelGGL(k_p252_layer<false>, grid, dim3(kThreads), 0, ctx().stream, cp, (u32)n_cols, (const u32 *)nullptr, (u32 *)out, n_nodes);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // namespace

extern "C" {

int tstwo_poseidon252_hash_many(const u32 *in, size_t n_msgs, u32 felts_per_msg, u32 *out) {
    TSTWO_REQUIRE_READY();
    if (n_msgs == 0) return TSTWO_OK;
    if (!out || (felts_per_msg && !in)) return set_error(TSTWO_ERR_BAD_ARG, "null device pointer");
    if (!aligned16(in) || !aligned16(out)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252: buffers must be 16-byte aligned");
    if (n_msgs > ((size_t)1 << 32) || felts_per_msg > (1u << 20)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252: batch too large");
    hipLaunchKernelGGL(k_p252_hash_many, dim3(ceil_div(n_msgs, kThreads)), dim3(kThreads), 0, ctx().stream, in, n_msgs, felts_per_msg, out);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_poseidon252_merkle_commit_layer(u32 log_size, const uint8_t *prev, const u32 *const *cols, size_t n_cols, uint8_t *out) {
    TSTWO_REQUIRE_READY();
    if (n_cols && !cols) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null column table");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    return p252_commit_layer(log_size, prev, cols, n_cols, out);
}

int tstwo_poseidon252_merkle_commit(const u32 *const *cols, const u32 *log_sizes, size_t n_cols, uint8_t *layers, uint8_t root[32]) {
    TSTWO_REQUIRE_READY();
    if (!layers) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null layers buffer");
    if (!aligned16(layers)) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: layers must be 16-byte aligned");
    if (n_cols && !log_sizes) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: null log size table");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    u32 max_log = 0;
    for (size_t i = 0; i < n_cols; i++) {
        if (log_sizes[i] > 30) return set_error(TSTWO_ERR_BAD_ARG, "poseidon252 merkle: log size out of range");
        if (log_sizes[i] > max_log) max_log = log_sizes[i];
    }
    // lowest layer at which a column joins (max_log + 1 when none): the tail launch may only take layers below it
    int lowest_col = (int)max_log + 1;
    for (size_t i = 0; i < n_cols; i++) lowest_col = std::min(lowest_col, (int)log_sizes[i]);
    const u32 **lc = n_cols ? new const u32 *[n_cols] : nullptr;
    const uint8_t *prev = nullptr;
    int rc = TSTWO_OK;
    for (int lg = (int)max_log; lg >= 0 && rc == TSTWO_OK; lg--) {   // vcs/prover.ts:24-27
        if (prev && lg < lowest_col && lg <= (int)kTailLog) {
            hipLaunchKernelGGL(k_p252_tail, dim3(1), dim3(kThreads), 0, ctx().stream, (u32 *)layers, (u32)lg + 1);
            if (hipGetLastError() != hipSuccess) rc = set_error(TSTWO_ERR_HIP, "poseidon252 merkle: tail kernel launch failed");
            break;
        }
        size_t k = 0;
        for (size_t i = 0; i < n_cols; i++)
            if (log_sizes[i] == (u32)lg) lc[k++] = cols[i];
        uint8_t *dst = layers + 32 * (((size_t)1 << lg) - 1);
        rc = p252_commit_layer((u32)lg, prev, lc, k, dst);
        prev = dst;
    }
    delete[] lc;
    if (rc) return rc;
    if (root) return small_d2h(root, layers, 32);
    return TSTWO_OK;
}

int tstwo_grind_poseidon252(const u32 digest[8], u32 pow_bits, uint64_t start_nonce, uint64_t *nonce_out) {
    TSTWO_REQUIRE_READY();
    if (!digest || !nonce_out) return set_error(TSTWO_ERR_BAD_ARG, "grind: null argument");
    if (pow_bits > 128) return set_error(TSTWO_ERR_BAD_ARG, "grind: pow_bits > 128");
    // canonical digest: compare with p from the top limb down
    for (int k = 7; k >= 0; k--) {
        if (digest[k] != felt::kP[k]) {
            if (digest[k] > felt::kP[k]) return set_error(TSTWO_ERR_BAD_ARG, "grind: digest is not a canonical field element");
            break;
        }
        if (k == 0) return set_error(TSTWO_ERR_BAD_ARG, "grind: digest is not a canonical field element");
    }
    Context &c = ctx();
    int rc = ensure_scratch(64);
    if (rc) return rc;
    unsigned long long *best = (unsigned long long *)c.scratch;
    FeltArg d;
    for (int k = 0; k < 8; k++) d.v[k] = digest[k];
    static_assert(kThreads == (int)kGrindLanes, "grind_plan.h restates the workgroup of k_p252_grind");
    const unsigned long long none = kGrindNone;
    for (GrindSearch s = grind_begin(GRIND_P252, start_nonce); grind_next(s);) {      // grind_plan.h
        TSTWO_HIP(hipMemsetAsync(best, 0xFF, sizeof(none), c.stream));
        hipLaunchKernelGGL(k_p252_grind, dim3((unsigned)((s.batch + kThreads - 1) / kThreads)), dim3(kThreads), 0, c.stream, d, pow_bits,
                           (unsigned long long)s.base, (unsigned long long)s.batch, best);
        TSTWO_LAUNCH_CHECK();
        unsigned long long found = none;
        if (int rc2 = small_d2h(&found, best, sizeof(found))) return rc2;
        if (found != none) {
            *nonce_out = found;
            return TSTWO_OK;
        }
    }
    return set_error(TSTWO_ERR_BAD_ARG, "grind: nonce space exhausted");
}

}  // extern "C"

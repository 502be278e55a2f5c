// cfft.hip — Circle FFT (PolyOps.evaluate / PolyOps.interpolate) for gfx950.
//
// What it computes (reference: backend/cpu/circle.ts:84-207,243-278, poly/utils.ts:78-100):
//   layer i pairs v[idx] with v[idx + 2^i]; its twiddle depends only on h = idx >> (i+1):
//     line layers i >= 1 : tw(i,h) = tree[L - 2^(n-i) + h]           (tree = twiddle buffer, L = |tree|)
//     circle layer i = 0 : tw(0,h) = +-tw(1, (h>>1)^1), negative iff (h ^ (h>>1)) & 1   ([y,-y,-x,x])
//   evaluate  : layers n-1 .. 0 with butterfly  (v0 + v1 t, v0 - v1 t)
//   interpolate: layers 0 .. n-1 with ibutterfly (v0 + v1, (v0 - v1) t) on the inverse tree, then * 2^-n.
//
// How it maps to the MI355X: the n layers are cut into passes over HBM.  A pass owns a contiguous
// range of layers [lo, lo+k) and a workgroup owns a *tile*: every index whose bits outside
// [lo, lo+k) u [0, c) are fixed, i.e. 2^k "rows" of 2^c contiguous words.  The tile is staged in LDS
// (coalesced 16-byte global accesses; rows are >= 128 B so strided passes still move whole lines),
// the k layers run as register radix-32/16 stages (G = 5/4 layers per LDS round trip, every
// butterfly pair owned by exactly one lane), and the tile is written back in place.  log 22 = two
// passes: layers 21..13 on [2^9 rows x 32 words] tiles, then layers 12..0 on contiguous 2^13 tiles.
// LDS index e is padded as e + (e >> 5): unit-stride runs and the stride-32 pattern of the bottom
// radix-32 stage are both bank-conflict free (32 banks for 4-byte accesses).
// Twiddles are read straight from the tree (L2 resident; a tile's twiddles are shared by every
// column, and blocks of the same tile are launched adjacently).
//
// Algorithmic bytes: 8 per element per transform (column read once + written once); real HBM/MALL
// traffic: 8 per element per pass (+ <= 2 for twiddles).  DESIGN.md §CFFT has the roofline numbers.
#include <unordered_map>
#include <unordered_set>

#include "cfft_plan.h"
#include "common.h"
#include "host_field.h"
#include <stdlib.h>

using namespace tstwo;

namespace {

constexpr int kThreads = (int)kCfftGenericThreads;     // lanes of the generic kernel (k_cfft_pass)
constexpr int kMaxV4 = 8;          // 16-byte vectors per lane per tile (32 words)

struct PassParams {
    u32 n;        // log size of the column
    u32 lo;       // lowest layer of this pass
    u32 k;        // layers [lo, lo+k)
    u32 c;        // log2(words per row); 0 for the bottom pass (lo == 0, one contiguous row)
    u32 logt;     // c + k = log2(tile words)
    u32 scale;    // interpolate's 2^-n, applied by the last pass; 0 = no scaling
    u32 cols_per_wg;
    const u32 *tw_end;  // tree + L
};

__device__ __forceinline__ u32 phys(u32 e) { return e + (e >> 5); }

// x * t for a twiddle stored doubled (t2 = 2t < 2^32): the 64-bit product's high word is
// floor(x t / 2^31) and its low word >> 1 is (x t) mod 2^31, so the Mersenne fold needs no
// and/alignbit (stwo's SIMD backend keeps "dbl" twiddles for the same reason).
__device__ __forceinline__ u32 m31_mul_dbl(u32 x, u32 t2) {
    u64 p = (u64)x * (u64)t2;
    u32 s = (u32)(p >> 32) + ((u32)p >> 1);
    return min(s, s - M31_P);
}
__device__ __forceinline__ void bf_dbl(u32 &v0, u32 &v1, u32 t2) {
    u32 m = m31_mul_dbl(v1, t2);
    u32 a = m31_add(v0, m);
    v1 = m31_sub(v0, m);
    v0 = a;
}
__device__ __forceinline__ void ibf_dbl(u32 &v0, u32 &v1, u32 t2) {
    u32 a = m31_add(v0, v1);
    v1 = m31_mul_dbl(m31_sub(v0, v1), t2);
    v0 = a;
}

// ---- butterflies in priority phases (the issue model and TSTWO_PHASE: common.h)
// N independent butterflies (x[i], y[i]) with doubled twiddles t2[i]; leaves the wave at kPrioHeavy (the next layer starts
// heavy as well) — the caller drops to kPrioLight after its last layer.
template <bool INV, int N>
__device__ __forceinline__ void bf_layer(u32 (&x)[N], u32 (&y)[N], const u32 (&t2)[N]) {
    static_assert(N == 8 || N == 4, "phase() pins 4, 8 or 16 values");
    const u32 P = vgpr_P();
    u32 s[N], d[N], u[N], w[N], u2[N], w2[N];
    u64 p[N];
    if (!INV) {
        phase<kPrioHeavy>(y);
#pragma unroll
        for (int i = 0; i < N; i++) p[i] = (u64)y[i] * (u64)t2[i];
        phase<kPrioLight>(p);
#pragma unroll
        for (int i = 0; i < N; i++) { s[i] = (u32)(p[i] >> 32) + ((u32)p[i] >> 1); d[i] = s[i] - P; }
        phase<kPrioHeavy>(d);
#pragma unroll
        for (int i = 0; i < N; i++) s[i] = min(s[i], d[i]);
        phase<kPrioLight>(s);
#pragma unroll
        for (int i = 0; i < N; i++) { u[i] = x[i] + s[i]; w[i] = x[i] - s[i]; u2[i] = u[i] - P; w2[i] = w[i] + P; }
        phase<kPrioHeavy>(u2, w2);
#pragma unroll
        for (int i = 0; i < N; i++) { x[i] = min(u[i], u2[i]); y[i] = min(w[i], w2[i]); }
    } else {
        phase<kPrioLight>(x, y);
#pragma unroll
        for (int i = 0; i < N; i++) { u[i] = x[i] + y[i]; w[i] = x[i] - y[i]; u2[i] = u[i] - P; w2[i] = w[i] + P; }
        phase<kPrioHeavy>(u2, w2);
#pragma unroll
        for (int i = 0; i < N; i++) { x[i] = min(u[i], u2[i]); p[i] = (u64)min(w[i], w2[i]) * (u64)t2[i]; }
        phase<kPrioLight>(p);
#pragma unroll
        for (int i = 0; i < N; i++) { s[i] = (u32)(p[i] >> 32) + ((u32)p[i] >> 1); d[i] = s[i] - P; }
        phase<kPrioHeavy>(d);
#pragma unroll
        for (int i = 0; i < N; i++) y[i] = min(s[i], d[i]);
    }
}

// v[i] *= t (t2 = 2t, wave-uniform): the 2^-n scale of the last inverse pass, in the same phases (leaves kPrioHeavy)
__device__ __forceinline__ void mul8_dbl(u32 (&v)[8], u32 t2) {
    const u32 P = vgpr_P();
    u32 s[8], d[8];
    u64 p[8];
    phase<kPrioHeavy>(v);
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = (u64)v[i] * (u64)t2;
    phase<kPrioLight>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) { s[i] = (u32)(p[i] >> 32) + ((u32)p[i] >> 1); d[i] = s[i] - P; }
    phase<kPrioHeavy>(d);
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = min(s[i], d[i]);
}

// Workgroup barrier that only drains LDS traffic.  __syncthreads() also waits vmcnt(0), which would
// serialise the in-flight prefetch loads / tile stores behind every stage (guide §5 "Pipelining across
// barriers"); global memory is never shared between lanes inside these kernels, so LDS ordering suffices.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Ordering between LDS accesses of ONE wave (a stage whose exchange stays inside the wave): the LDS executes a wave's
// instructions in issue order, so only the compiler has to be kept from reordering them.
__device__ __forceinline__ void lds_wave_fence() { asm volatile("" ::: "memory"); }

}  // namespace
#include "cfft_fast.cuh"
namespace {

// One register stage: G consecutive layers on LDS bits [q, q+G).  Twiddles come from the tile's LDS
// heap `twl` (doubled values): layer bit b lives at twl[2^(logt-1-b) + (e >> (b+1))].
// CIRCLE: bit 0 of this stage is the circle layer (only when q == 0 and lo == 0; needs G >= 3).
template <int G, bool INV, bool CIRCLE>
__device__ __forceinline__ void run_stage(u32 *lds, const u32 *twl, const u32 q, const u32 logt) {
    const u32 ngroups = 1u << (logt - G);
    for (u32 gid = threadIdx.x; gid < ngroups; gid += kThreads) {
        const u32 low = gid & ((1u << q) - 1u), high = gid >> q;
        const u32 e0 = (high << (q + G)) | low;
        u32 v[1 << G];
#pragma unroll
        for (int m = 0; m < (1 << G); m++) v[m] = lds[phys(e0 + ((u32)m << q))];
#pragma unroll
        for (int step = 0; step < G; step++) {
            const int l = INV ? step : (G - 1 - step);
            const u32 b = q + (u32)l;                       // LDS bit of this layer
            if (CIRCLE && l == 0) {
                // tw(0,h) = +-tw(1,(h>>1)^1), negative iff (h ^ (h>>1)) & 1   (backend/cpu/circle.ts:270-278)
                const u32 *t1 = twl + (1u << (logt - 2)) + (high << (G - 2));
#pragma unroll
                for (int j = 0; j < (1 << (G - 1)); j++) {
                    u32 t2 = t1[(j >> 1) ^ 1];
                    if ((j ^ (j >> 1)) & 1) t2 = 0xFFFFFFFEu - t2;      // 2(P - t)
                    if (INV) ibf_dbl(v[2 * j], v[2 * j + 1], t2);
                    else bf_dbl(v[2 * j], v[2 * j + 1], t2);
                }
            } else {
                const u32 *tl = twl + (1u << (logt - 1 - b)) + (high << (G - 1 - l));
#pragma unroll
                for (int j = 0; j < (1 << (G - 1 - l)); j++) {
                    const u32 t2 = tl[j];
#pragma unroll
                    for (int r = 0; r < (1 << l); r++) {
                        const int m0 = (j << (l + 1)) | r;
                        if (INV) ibf_dbl(v[m0], v[m0 + (1 << l)], t2);
                        else bf_dbl(v[m0], v[m0 + (1 << l)], t2);
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < (1 << G); m++) lds[phys(e0 + ((u32)m << q))] = v[m];
    }
}

template <bool INV, bool CIRCLE>
__device__ __forceinline__ void dispatch_stage(int g, u32 *lds, const u32 *twl, u32 q, u32 logt) {
    switch (g) {
        case 5: run_stage<5, INV, CIRCLE>(lds, twl, q, logt); break;
        case 4: run_stage<4, INV, CIRCLE>(lds, twl, q, logt); break;
        case 3: run_stage<3, INV, CIRCLE>(lds, twl, q, logt); break;
        case 2: if (!CIRCLE) run_stage<2, INV, false>(lds, twl, q, logt); break;
        case 1: if (!CIRCLE) run_stage<1, INV, false>(lds, twl, q, logt); break;
        default: break;
    }
}

// Stage schedule for the layer bits [c, logt) of a tile: the bottom pass (lo == 0) spends min(5, k)
// layers on a conflict-free radix-32 stage at q = 0, everything else is cut into balanced stages of <= 5
// layers (q >= 5 there, so lanes read unit-stride runs).  Returned low -> high.
__device__ __forceinline__ int plan_stages(const PassParams &pp, int *g_out) {
    int cnt = 0;
    u32 rem = pp.k;
    if (pp.lo == 0) {
        u32 g0 = rem < 5 ? rem : 5;
        g_out[cnt++] = (int)g0;
        rem -= g0;
    }
    if (rem) {
        u32 stages = (rem + 4) / 5;
        u32 base = rem / stages, extra = rem % stages;
        for (u32 s = 0; s < stages; s++) g_out[cnt++] = (int)(base + (s < extra ? 1 : 0));
    }
    return cnt;
}

// One workgroup = one tile position x `cols_per_wg` columns.  The tile's twiddles are staged once
// in LDS and reused for every column; the next column's tile is prefetched into registers while
// the current one is transformed, so HBM latency overlaps the butterflies inside the workgroup.
// Only the bottom pass of a column that is one tile (3 <= n <= 12: lo = 0, c = 0) is ever launched; its tile and heap stay below 64 KiB.
template <bool INV>
__global__ void __launch_bounds__(kThreads, 3) k_cfft_pass(ColPtrs cols, u32 n_cols, PassParams pp) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const u32 tile_words = 1u << pp.logt;
    u32 *twl = lds + ((tile_words + (tile_words >> 5) + 3u) & ~3u);     // twiddle heap behind the padded tile

    // column group is the fastest-varying block coordinate: blocks sharing a tile (hence twiddles) are adjacent
    const u32 groups = (n_cols + pp.cols_per_wg - 1) / pp.cols_per_wg;
    const u32 cgroup = blockIdx.x % groups;
    const u32 tile = blockIdx.x / groups;
    const u32 col0 = cgroup * pp.cols_per_wg;
    const u32 col1 = min(col0 + pp.cols_per_wg, n_cols);

    const u32 mid_bits = pp.lo - pp.c;                     // 0 for the bottom pass
    const u32 mid = tile & ((1u << mid_bits) - 1u);
    const u32 hi = tile >> mid_bits;
    const size_t base = ((size_t)hi << (pp.lo + pp.k)) | ((size_t)mid << pp.c);
    const u32 cmask = (1u << pp.c) - 1u;

    // ---- prefetch the first column's tile (16 bytes per lane per access)
    uint4 pf[kMaxV4];
    {
        const u32 *__restrict__ data = colp_u(cols, col0);
#pragma unroll
        for (int it = 0; it < kMaxV4; it++) {
            const u32 e = 4u * (threadIdx.x + (u32)it * kThreads);
            if (e < tile_words) pf[it] = gload4(data + base + ((size_t)(e >> pp.c) << pp.lo) + (e & cmask));
        }
    }
    // ---- twiddle heap: level lv (2^lv entries at twl[2^lv ..]) holds layer bit b = logt-1-lv, i.e. global
    //      layer i = lo + b - c, entries tree[L - 2^(n-i) + (hi << lv) + hl]; stored doubled.
    {
        const u32 skip = (pp.lo == 0) ? 1u : 0u;            // the circle layer has no entries of its own
        const u32 heap = 1u << (pp.k - skip);
        for (u32 idx = threadIdx.x + 1; idx < heap; idx += kThreads) {
            const u32 lv = 31u - (u32)__clz(idx);
            const u32 b = pp.logt - 1u - lv;
            const u32 i = pp.lo + b - pp.c;
            const u32 t = pp.tw_end[-(ptrdiff_t)(1u << (pp.n - i)) + (ptrdiff_t)((hi << lv) + (idx - (1u << lv)))];
            twl[idx] = t + t;
        }
    }

    int gs[8];
    const int n_stages = plan_stages(pp, gs);

    for (u32 col = col0; col < col1; col++) {
        // ---- registers -> LDS
#pragma unroll
        for (int it = 0; it < kMaxV4; it++) {
            const u32 e = 4u * (threadIdx.x + (u32)it * kThreads);
            if (e < tile_words) {
                const u32 p = phys(e);
                lds[p] = pf[it].x; lds[p + 1] = pf[it].y; lds[p + 2] = pf[it].z; lds[p + 3] = pf[it].w;
            }
        }
        __syncthreads();
        // ---- prefetch the next column while this one is transformed
        if (col + 1 < col1) {
            const u32 *__restrict__ next = colp_u(cols, col + 1);
#pragma unroll
            for (int it = 0; it < kMaxV4; it++) {
                const u32 e = 4u * (threadIdx.x + (u32)it * kThreads);
                if (e < tile_words) pf[it] = gload4(next + base + ((size_t)(e >> pp.c) << pp.lo) + (e & cmask));
            }
        }
        if (!INV) {
            u32 q = pp.logt;
            for (int s = n_stages - 1; s >= 0; s--) {
                q -= (u32)gs[s];
                if (pp.lo == 0 && q == 0) dispatch_stage<false, true>(gs[s], lds, twl, q, pp.logt);
                else dispatch_stage<false, false>(gs[s], lds, twl, q, pp.logt);
                __syncthreads();
            }
        } else {
            u32 q = pp.c;
            for (int s = 0; s < n_stages; s++) {
                if (pp.lo == 0 && q == 0) dispatch_stage<true, true>(gs[s], lds, twl, q, pp.logt);
                else dispatch_stage<true, false>(gs[s], lds, twl, q, pp.logt);
                q += (u32)gs[s];
                __syncthreads();
            }
        }
        // ---- LDS -> global (fused 2^-n scaling on interpolate's last pass)
        u32 *__restrict__ data = colp_u(cols, col);
#pragma unroll
        for (int it = 0; it < kMaxV4; it++) {
            const u32 e = 4u * (threadIdx.x + (u32)it * kThreads);
            if (e < tile_words) {
                const u32 p = phys(e);
                uint4 x = make_uint4(lds[p], lds[p + 1], lds[p + 2], lds[p + 3]);
                if (INV && pp.scale) {
                    x.x = m31_mul(x.x, pp.scale); x.y = m31_mul(x.y, pp.scale);
                    x.z = m31_mul(x.z, pp.scale); x.w = m31_mul(x.w, pp.scale);
                }
                gstore4(data + base + ((size_t)(e >> pp.c) << pp.lo) + (e & cmask), x);
            }
        }
        __syncthreads();
    }
}

// log_size 1 and 2 (backend/cpu/circle.ts:93-110,153-185): twiddles are coordinates of the half
// coset's initial point, supplied by the host.  tx/ty (and the scale) are already inverted for INV.
template <bool INV>
__global__ void k_cfft_small(ColPtrs cols, u32 n_cols, u32 n, u32 tx, u32 ty, u32 scale) {
    u32 col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n_cols) return;
    u32 *v = colp(cols, col);
    if (n == 1) {
        u32 v0 = gload1(v), v1 = gload1(v + 1);
        if (!INV) m31_butterfly(v0, v1, ty);
        else { m31_ibutterfly(v0, v1, ty); v0 = m31_mul(v0, scale); v1 = m31_mul(v1, scale); }
        gstore1(v, v0); gstore1(v + 1, v1);
    } else {
        u32 v0 = gload1(v), v1 = gload1(v + 1), v2 = gload1(v + 2), v3 = gload1(v + 3);
        if (!INV) {
            m31_butterfly(v0, v2, tx); m31_butterfly(v1, v3, tx);
            m31_butterfly(v0, v1, ty); m31_butterfly(v2, v3, m31_neg(ty));
        } else {
            m31_ibutterfly(v0, v1, ty); m31_ibutterfly(v2, v3, m31_neg(ty));
            m31_ibutterfly(v0, v2, tx); m31_ibutterfly(v1, v3, tx);
            v0 = m31_mul(v0, scale); v1 = m31_mul(v1, scale); v2 = m31_mul(v2, scale); v3 = m31_mul(v3, scale);
        }
        gstore1(v, v0); gstore1(v + 1, v1); gstore1(v + 2, v2); gstore1(v + 3, v3);
    }
}

// ---- host.  cfft_plan.h decides what is launched — route, passes, kernels, tiles, LDS — before anything is; what follows
// checks the arguments, sizes the grids and launches.

// The kernel of one (kind, K, LOGT) of kCfftShapes, and the walk over the table that finds a pass's: only shapes of the table
// are instantiated, and the planner names no other.
template <CfftKind KIND, int K, int LOGT>
const void *shape_kernel(bool inverse, u32 ext) {
    if constexpr (KIND == CFFT_BOTTOM) return inverse ? (const void *)fast::k_cfft_b<true, LOGT> : (const void *)fast::k_cfft_b<false, LOGT>;
    else if constexpr (KIND == CFFT_BOTTOM_STREAM) return (const void *)fast::k_cfft_b_stream<LOGT>;
    else if constexpr (KIND == CFFT_BOTTOM_OOP) return (const void *)fast::k_cfft_b<true, LOGT, true>;
    else if constexpr (KIND == CFFT_STRIDED) return inverse ? (const void *)fast::k_cfft_a<true, K, 0, LOGT> : (const void *)fast::k_cfft_a<false, K, 0, LOGT>;
    else if constexpr (KIND == CFFT_STRIDED_STREAM) { static_assert(LOGT == 15, "k_cfft_a_stream is the 2^15 tile"); return (const void *)fast::k_cfft_a_stream<K>; }
    else return ext == 1 ? (const void *)fast::k_cfft_a<false, K, 1, LOGT> : (const void *)fast::k_cfft_a<false, K, 2, LOGT>;
}
constexpr int first_k(size_t row) { return row < kCfftShapeRows ? kCfftShapes[row].k_lo : 0; }
template <size_t ROW = 0, int K = first_k(0)>
const void *kernel_for(const CfftPass &ps, bool inverse, u32 ext) {
    if constexpr (ROW == kCfftShapeRows) return nullptr;
    else {
        constexpr CfftShape S = kCfftShapes[ROW];
        if (ps.kind == S.kind && ps.logt == S.logt && ps.k == (u32)K) return shape_kernel<S.kind, K, S.logt>(inverse, ext);
        if constexpr (K < S.k_hi) return kernel_for<ROW, K + 1>(ps, inverse, ext);
        else return kernel_for<ROW + 1, first_k(ROW + 1)>(ps, inverse, ext);
    }
}

// Grid of a pass kernel: its (tile, column) work items are dealt in equal contiguous shares to as many workgroups as the
// chip holds at once (CUs x resident workgroups per CU for this kernel's registers / LDS), so the whole pass is ONE round of
// workgroups with no tail round and each workgroup stages a tile's twiddles once for all of its columns of that tile.
// (32 x 2^22: 2048 workgroups of 8 columns on 768 resident slots made 2.67 rounds, i.e. 11 % of the slots idle in the last
// one, and paid the twiddle / first-load prologue 2048 times instead of 768.)  TSTWO_CFFT_ROUNDS=k asks for k x that many
// workgroups (dynamic balance against the extra prologues); fewer items than slots: one item per workgroup.
unsigned plan_grid(const void *kernel, int threads, size_t lds_bytes, size_t total_items) {
    static std::unordered_map<const void *, int> resident;        // workgroups per CU, per kernel
    auto it = resident.find(kernel);
    if (it == resident.end()) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        it = resident.emplace(kernel, per_cu).first;
    }
    size_t slots = (size_t)ctx().n_cus * (size_t)it->second;
    slots *= (size_t)knobs().cfft_rounds;
    const int cap = knobs().cfft_maxwg;      // experiments
    if (cap && slots > (size_t)cap) slots = (size_t)cap;
    return (unsigned)(total_items < slots ? total_items : slots);
}

// Tiles above 64 KiB of LDS need a per-kernel opt-in (160 KiB per CU on gfx950); done once per kernel, not per launch.
int allow_big_lds(const void *kernel) {
    static std::unordered_set<const void *> done;
    if (done.insert(kernel).second)
        TSTWO_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return TSTWO_OK;
}

// What every launch shares: the pointer table of `cols` (more than 64 columns: in device memory) and, where the kernel reads a
// second one, of `src`; the grid (`blocks` for the small and generic routes; for a tiled kernel plan_grid sizes it for the
// ps.tiles x n_cols work items); the launch and its check.  `args` are the kernel's arguments behind tables and counts.
template <typename... Args>
int launch(const void *kernel, const CfftPass &ps, unsigned blocks, u32 *const *cols, const u32 *const *src, size_t n_cols, Args... args) {
    const bool tiled = ps.kind != CFFT_WHOLE;
    size_t lds_bytes = ps.lds_bytes;
    if (tiled) {
        lds_bytes += (size_t)knobs().cfft_lds_pad;     // experiments: extra (unused) dynamic LDS per workgroup lowers the resident workgroups per CU
        if (int rc = allow_big_lds(kernel)) return rc;
    }
    if (knobs().cfft_trace) {
        hipFuncAttributes fa;
        hipError_t e = hipFuncGetAttributes(&fa, kernel);
        fprintf(stderr, "[cfft] kernel %p threads %u lds %zu: getattr=%d maxDynamicSharedSizeBytes=%d sharedSizeBytes=%zu numRegs=%d maxThreadsPerBlock=%d\n",
                kernel, ps.threads, lds_bytes, (int)e, fa.maxDynamicSharedSizeBytes, fa.sharedSizeBytes, fa.numRegs, fa.maxThreadsPerBlock);
    }
    ColPtrs cp, sp;
    fast::NoSrc none;
    int rc = fill_col_table(cp, cols, n_cols, 0);
    if (!rc && src) rc = fill_col_table(sp, src, n_cols, 1);
    if (rc) return rc;
    u32 cnt = (u32)n_cols, items = (u32)(ps.tiles * n_cols);         // (the planner refused what does not fit 32 bits)
    if (tiled) blocks = plan_grid(kernel, (int)ps.threads, lds_bytes, items);
    // kernel signatures: tiled (ColPtrs cols, <ColPtrs | NoSrc> src, n_cols, total_items, args...); the others (ColPtrs cols, n_cols, args...)
    void *argv[4 + sizeof...(Args)], *behind[] = {(void *)&args...};
    int na = 0;
    argv[na++] = &cp;
    if (tiled) argv[na++] = src ? (void *)&sp : (void *)&none;
    argv[na++] = &cnt;
    if (tiled) argv[na++] = &items;
    for (void *a : behind) argv[na++] = a;
    (void)hipLaunchKernel(kernel, dim3(blocks), dim3(ps.threads), argv, lds_bytes, ctx().stream);
    TSTWO_LAUNCH_CHECK();
    if (knobs().cfft_sync) TSTWO_HIP(hipStreamSynchronize(ctx().stream));
    return TSTWO_OK;
}

// log_size 1 and 2: the twiddles are coordinates of the half coset's initial point, inverted here for the inverse
int run_small(const CfftPlan &plan, bool inverse, u32 *const *cols, size_t n_cols, u32 n, u32 half_initial, u32 n_inv) {
    u32 px, py;
    host::point(half_initial, &px, &py);
    u32 tx = px, ty = py, scale = 1;
    if (inverse) {
        if (py == 0 || (n == 2 && px == 0)) return set_error(TSTWO_ERR_ZERO_INVERSE, "0 has no inverse");
        ty = host::inv(py);
        tx = n == 2 ? host::inv(px) : 0;
        scale = n_inv;
    }
    const void *kernel = inverse ? (const void *)k_cfft_small<true> : (const void *)k_cfft_small<false>;
    return launch(kernel, plan.pass[0], plan.blocks, cols, nullptr, n_cols, n, tx, ty, scale);
}

// Runs a plan of the generic or the tiled route on `cols`; the first pass of interpolate_to / evaluate_extended reads `src`.
// All columns go through a pass in one launch.  (Measured on MI355X, 32 x 2^22: running the passes back to back
// on Infinity-Cache-sized column groups is slower — 688 us ungrouped vs 724/771/879 us for groups of 16/8/4 —
// the extra launch tails cost more than MALL residency of the intermediate returns.)
int run_plan(const CfftPlan &plan, bool inverse, u32 ext, u32 *const *cols, const u32 *const *src, size_t n_cols, u32 n, const u32 *tw, u32 tw_log, u32 n_inv) {
    const u32 *tw_end = tw + ((size_t)1 << tw_log);
    if (plan.route == CFFT_GENERIC) {
        const PassParams pp = {n, 0, n, 0, n, inverse ? n_inv : 0, plan.cols_per_wg, tw_end};
        const void *kernel = inverse ? (const void *)k_cfft_pass<true> : (const void *)k_cfft_pass<false>;
        return launch(kernel, plan.pass[0], plan.blocks, cols, nullptr, n_cols, pp);
    }
    for (u32 i = 0; i < plan.n_passes; i++) {       // execution order: high -> low layers forward, low -> high inverse
        const CfftPass &ps = plan.pass[i];
        const void *kernel = kernel_for(ps, inverse, ext);
        const u32 *const *from = ps.kind == CFFT_BOTTOM_OOP || ps.kind == CFFT_STRIDED_EXT ? src : nullptr;
        const u32 scale = ps.scale ? n_inv : 0;
        const int rc = ps.lo == 0 ? launch(kernel, ps, 0, cols, from, n_cols, n, tw_end, scale) : launch(kernel, ps, 0, cols, from, n_cols, n, ps.lo, tw_end, scale);
        if (rc) return rc;
    }
    return TSTWO_OK;
}

const char *plan_for(CfftEntry entry, u32 ext, u32 n, size_t n_cols, CfftPlan &plan) {
    const Knobs &kn = knobs();      // experiments build only: bottom-pass size, strided-pass limit, strided tile
    return cfft_plan(entry, ext, n, n_cols, (u32)ctx().n_cus, {(u32)kn.cfft_kb, (u32)kn.cfft_ka, (u32)kn.cfft_logta}, plan);
}

// The arguments of every route that reads a twiddle tree; src: the read-only second table of the out-of-place entries, or null.
int check_tiled_args(u32 *const *cols, const u32 *const *src, size_t n_cols, u32 n, const u32 *tw, u32 tw_log) {
    if (!tw) return set_error(TSTWO_ERR_BAD_ARG, "cfft: null twiddle buffer");
    if (tw_log > 31 || ((size_t)1 << (n - 1)) > ((size_t)1 << tw_log)) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");
    for (size_t i = 0; i < n_cols; i++)
        if (!aligned16(cols[i]) || (src && !aligned16(src[i]))) return set_error(TSTWO_ERR_BAD_ARG, "cfft: columns must be 16-byte aligned");
    if (!aligned16(tw)) return set_error(TSTWO_ERR_BAD_ARG, "cfft: twiddle buffer must be 16-byte aligned");
    return TSTWO_OK;
}
int check_log_size(u32 n) {
    if (n == 0 || n > 31) return set_error(TSTWO_ERR_BAD_ARG, "cfft: log_size out of range");
    if (n > kCfftMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "cfft: log_size > 30 exceeds MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4)");
    return TSTWO_OK;
}

// Arguments, then the plan's own refusal, then the launches: an entry that fails has launched nothing.
int cfft_planned(CfftEntry entry, u32 ext, u32 *const *cols, const u32 *const *src, size_t n_cols, u32 n, u32 half_initial, const u32 *tw, u32 tw_log,
                 const CfftPlan &plan, const char *refused) {
    const bool inverse = entry == CFFT_INTERPOLATE || entry == CFFT_INTERPOLATE_TO;
    const u32 n_inv = host::inv((1u << n) % M31_P);
    if (!refused && plan.route == CFFT_SMALL) return run_small(plan, inverse, cols, n_cols, n, half_initial, n_inv);
    if (int rc = check_tiled_args(cols, src, n_cols, n, tw, tw_log)) return rc;
    if (refused) return set_error(TSTWO_ERR_BAD_ARG, refused);
    return run_plan(plan, inverse, ext, cols, src, n_cols, n, tw, tw_log, n_inv);
}

int cfft(bool inverse, u32 *const *cols, size_t n_cols, u32 n, u32 half_initial, const u32 *tw, u32 tw_log) {
    TSTWO_REQUIRE_READY();
    if (int rc = check_log_size(n)) return rc;
    if (n_cols == 0) return TSTWO_OK;
    if (!cols) return set_error(TSTWO_ERR_BAD_ARG, "cfft: null column table");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    const CfftEntry entry = inverse ? CFFT_INTERPOLATE : CFFT_EVALUATE;
    CfftPlan plan;
    const char *refused = plan_for(entry, 0, n, n_cols, plan);
    return cfft_planned(entry, 0, cols, nullptr, n_cols, n, half_initial, tw, tw_log, plan, refused);
}

}  // namespace

extern "C" {

int tstwo_cfft_evaluate(u32 *const *cols, size_t n_cols, u32 log_size, u32 half_initial, const u32 *tw, u32 tw_log) {
    return cfft(false, cols, n_cols, log_size, half_initial, tw, tw_log);
}
int tstwo_cfft_interpolate(u32 *const *cols, size_t n_cols, u32 log_size, u32 half_initial, const u32 *itw, u32 tw_log) {
    return cfft(true, cols, n_cols, log_size, half_initial, itw, tw_log);
}

// The launches of an in-place transform (bench.py takes its launch count from here): the count of the plan cfft() runs.
int tstwo_cfft_plan_passes(u32 log_size, size_t n_cols, u32 *n_passes) {
    TSTWO_REQUIRE_READY();          // (the planner asks the context for the CU count)
    if (!n_passes) return set_error(TSTWO_ERR_BAD_ARG, "cfft: null output");
    if (log_size == 0 || log_size > kCfftMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "cfft: log_size out of range");
    CfftPlan plan;
    if (const char *refused = plan_for(CFFT_EVALUATE, 0, log_size, n_cols, plan)) return set_error(TSTWO_ERR_BAD_ARG, refused);
    *n_passes = plan.n_passes;
    return TSTWO_OK;
}

// Out-of-place interpolation: src[i] (evaluations, left untouched) -> dst[i] (coefficients).  On the tiled path the first
// (bottom) pass reads src and writes dst, so the clone the value-semantics API needs costs no extra pass over HBM.
int tstwo_cfft_interpolate_to(const u32 *const *src, u32 *const *dst, size_t n_cols, u32 log_size, u32 half_initial, const u32 *itw, u32 tw_log) {
    TSTWO_REQUIRE_READY();
    if (n_cols == 0) return TSTWO_OK;
    if (!src || !dst) return set_error(TSTWO_ERR_BAD_ARG, "cfft: null column table");
    TSTWO_REQUIRE_TABLE(src, n_cols); TSTWO_REQUIRE_TABLE(dst, n_cols);
    if (int rc = check_log_size(log_size)) return rc;
    CfftPlan plan;
    const char *refused = plan_for(CFFT_INTERPOLATE_TO, 0, log_size, n_cols, plan);
    if (refused || plan.route != CFFT_FALLBACK)
        return cfft_planned(CFFT_INTERPOLATE_TO, 0, dst, src, n_cols, log_size, half_initial, itw, tw_log, plan, refused);
    for (size_t i = 0; i < n_cols; i++) {
        int rc = tstwo_copy(dst[i], src[i], (size_t)4 << log_size);
        if (rc) return rc;
    }
    return cfft(true, dst, n_cols, log_size, half_initial, itw, tw_log);
}

// CirclePoly.extend + evaluate (backend/cpu/circle.ts:71-134) in one call: polys[i] holds 2^log_poly coefficients,
// out[i] receives the 2^log_size evaluations.  When the extension is by 1 or 2 bits and the transform takes the tiled
// path, the zero padding is never materialised: the first pass reads the small polynomial and skips the replicating
// layers.  Otherwise: tstwo_poly_extend into out[i], then the in-place transform.
int tstwo_cfft_evaluate_extended(const u32 *const *polys, u32 log_poly, u32 *const *out, size_t n_cols, u32 log_size, u32 half_initial,
                                 const u32 *tw, u32 tw_log) {
    TSTWO_REQUIRE_READY();
    if (n_cols == 0) return TSTWO_OK;
    if (!polys || !out) return set_error(TSTWO_ERR_BAD_ARG, "cfft: null column table");
    TSTWO_REQUIRE_TABLE(polys, n_cols); TSTWO_REQUIRE_TABLE(out, n_cols);
    if (log_size < log_poly) return set_error(TSTWO_ERR_LOG_SIZE, "log size too small");
    if (int rc = check_log_size(log_size)) return rc;
    const u32 ext = log_size - log_poly;
    CfftPlan plan;
    const char *refused = plan_for(CFFT_EVALUATE_EXTENDED, ext, log_size, n_cols, plan);
    if (refused || plan.route != CFFT_FALLBACK)
        return cfft_planned(CFFT_EVALUATE_EXTENDED, ext, out, polys, n_cols, log_size, half_initial, tw, tw_log, plan, refused);
    for (size_t i = 0; i < n_cols; i++) {
        int rc = tstwo_poly_extend(polys[i], log_poly, out[i], log_size);
        if (rc) return rc;
    }
    return cfft(false, out, n_cols, log_size, half_initial, tw, tw_log);
}

}  // extern "C"

// logup.hip — the LogUp interaction trace on the device (Rust stwo constraint_framework/logup.rs, LogupTraceGenerator and
// LogupColGenerator; the framework side is tstwo_amd/logup.py).
//
// k_logup_column<W>: one interaction column, out[r] = prev[r] + sum_b num_b[r] / den_b[r], where every denominator is a linear
// form over M31 columns, den_b[r] = sum_t coeff_bt cols_bt[r] + constant_b with QM31 coefficients (Relation::combine).  One lane
// owns W = 4 consecutive rows (16-byte loads) when every column is 16-byte aligned, else one row.  The denominators are combined
// in registers (64-bit sums of M31 x M31 products, folded every fourth term); the fractions of a row are added as
// a/b + c/d = (ad + cb)/(bd), so a row needs one inversion whatever the number of fractions, and the W inversions of a lane share
// one (Montgomery's trick over the lane's rows: 3 (W - 1) QM31 products and one qm31_inv).  A zero denominator raises the
// library's zero flag (as the *_async batch inverses do) and is treated as 1.  The fraction descriptors (pointers,
// coefficients, constants) are uploaded through the small-upload ring and read with scalar loads (wave-uniform index).
//
// Coset-order prefix sum (tstwo_logup_finalize_last).  Rows are stored bit-reversed on the circle domain; "previous row" (mask
// offset -1) is the coset order.  With L = log_size - 1, j = k >> 1 and rev = bit reversal over L bits, coset row k lives at
// coset_pos(k, L) (coset_order.cuh): 2 rev(j) for even k (the A part of j), 2 (2^L - 1 - rev(j)) + 1 for odd k (the B part).
// A block is a run of 2^R consecutive j (2^(R+1) coset rows); with j = top 2^R + low its A parts sit at
// rev(j) = rev_R(low) 2^(L-R) + rev_{L-R}(top), a stride of 2^(L-R).  A tile takes the G blocks whose rev(top) are g G + y, y < G:
// 2^R runs of 2G contiguous words (G A parts and G B parts interleaved).  The B parts in those words belong to the blocks of the
// mirrored tile ~g, so a workgroup loads tiles g and ~g and owns 2G whole blocks (as k_bit_reverse_tiled pairs tile m with
// rev(m)).  The coordinates are independent (one M31 prefix sum each, blockIdx.y).  Three launches, no hand-off between
// workgroups inside a launch (MI355X_MICROARCH: cross-XCD visibility):
//   k_logup_tile<false>  the sum of every block -> sums[coord][top]
//   k_logup_block_scan   one workgroup per coordinate: claimed = the sum of the block sums, s = claimed / 2^log_size, and the
//                        exclusive prefix of (block sum - 2^(R+1) s) in place
//   k_logup_tile<true>   the scan of each block from its prefix, written back in place
// Up to 2^12 rows (fewer than two tiles) one workgroup per coordinate holds the whole column in LDS (k_logup_small).
#include <string>

#include "common.h"
#include "coset_order.cuh"

using namespace tstwo;

namespace {

constexpr u32 kMaxFracs = TSTWO_LOGUP_MAX_FRACS;
constexpr u32 kMaxTerms = TSTWO_LOGUP_MAX_TERMS;
constexpr u32 kMaxLog = TSTWO_LOGUP_MAX_LOG;
constexpr int kThreads = 256;

// fraction descriptor as uploaded (u32 words; the pointers are 8-byte aligned)
constexpr u32 kDescNum = 0;                              // u64: numerator column (0: the constant)
constexpr u32 kDescNumConst = 2, kDescNTerms = 3;
constexpr u32 kDescConst = 4;                            // 4 words
constexpr u32 kDescCoeff = 8;                            // 4 words per term
constexpr u32 kDescCols = kDescCoeff + 4 * kMaxTerms;    // u64 per term
constexpr u32 kDescWords = kDescCols + 2 * kMaxTerms;
static_assert(kDescCols % 2 == 0 && kDescWords % 2 == 0, "descriptor pointers must stay 8-byte aligned");
static_assert(kMaxFracs * kDescWords * 4 <= kUpSlotBytes, "the descriptors must fit one upload slot");

typedef const u32 __attribute__((address_space(4))) *k32;
typedef const unsigned long long __attribute__((address_space(4))) *k64;

__device__ __forceinline__ u32 uni(u32 x) { return (u32)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ const u32 *desc_ptr(const u32 *desc, u32 word) { return (const u32 *)((k64)desc)[uni(word) >> 1]; }

// x = t1 + 2^31 t2 + 2^63 t3 == t1 + t2 + 2 t3 (mod P), < 2^33: room for four more products of canonical values
__device__ __forceinline__ u64 fold64(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 t2 = __builtin_amdgcn_alignbit(hi, lo, 31);
    return (u64)((lo & M31_P) + ((hi >> 31) << 1)) + t2;
}

template <int W>
__device__ __forceinline__ void load_w(const u32 *col, u32 row, u32 (&x)[W]) {
    if constexpr (W == 4) {
        const uint4 v = gload4(col, row);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = gload1(col, row);
    }
}

struct ColArgs {
    const u32 *desc;                 // n_fracs descriptors of kDescWords
    CSoa4 prev;
    Soa4 out;
    u32 n_fracs, n_rows, has_prev;
    u32 *flag;
};

template <int W>
__global__ void __launch_bounds__(kThreads) k_logup_column(ColArgs a) {
    const u32 t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= a.n_rows / W) return;
    const u32 row = t * W;
    const k32 d = (k32)a.desc;
    qm31 num[W], den[W];
#pragma unroll 1
    for (u32 b = 0; b < a.n_fracs; b++) {
        const u32 base = uni(b * kDescWords);
        const u32 n_terms = d[base + kDescNTerms];
        u64 acc[W][4];
#pragma unroll
        for (int e = 0; e < W; e++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[e][j] = 0;
#pragma unroll 1
        for (u32 k = 0; k < n_terms; k++) {
            const u32 c = uni(base + kDescCoeff + 4 * k);
            const u32 q0 = d[c], q1 = d[c + 1], q2 = d[c + 2], q3 = d[c + 3];
            u32 x[W];
            load_w<W>(desc_ptr(a.desc, base + kDescCols + 2 * k), row, x);
#pragma unroll
            for (int e = 0; e < W; e++) {
                acc[e][0] += (u64)q0 * x[e];
                acc[e][1] += (u64)q1 * x[e];
                acc[e][2] += (u64)q2 * x[e];
                acc[e][3] += (u64)q3 * x[e];
            }
            if ((k & 3) == 3) {
#pragma unroll
                for (int e = 0; e < W; e++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[e][j] = fold64(acc[e][j]);
            }
        }
        const u32 k0 = d[base + kDescConst], k1 = d[base + kDescConst + 1], k2 = d[base + kDescConst + 2], k3 = d[base + kDescConst + 3];
        u32 nv[W];
        const u32 *ncol = desc_ptr(a.desc, base + kDescNum);
        if (ncol) {
            load_w<W>(ncol, row, nv);
        } else {
            const u32 nc = d[base + kDescNumConst];
#pragma unroll
            for (int e = 0; e < W; e++) nv[e] = nc;
        }
#pragma unroll
        for (int e = 0; e < W; e++) {
            const qm31 de = {m31_add(m31_reduce_u64(acc[e][0]), k0), m31_add(m31_reduce_u64(acc[e][1]), k1),
                             m31_add(m31_reduce_u64(acc[e][2]), k2), m31_add(m31_reduce_u64(acc[e][3]), k3)};
            if (b == 0) {
                num[e] = qm31_from_m31(nv[e]);
                den[e] = de;
            } else {                               // num/den + nv/de = (num de + nv den) / (den de)
                num[e] = qm31_add(qm31_mul(num[e], de), qm31_mul_m31(den[e], nv[e]));
                den[e] = qm31_mul(den[e], de);
            }
        }
    }
    // one inversion for the lane's W rows
    bool zero = false;
#pragma unroll
    for (int e = 0; e < W; e++)
        if (qm31_is_zero(den[e])) { zero = true; den[e] = qm31_from_m31(1u); }
    if (zero) raise_flag(a.flag);
    qm31 pre[W];
#pragma unroll
    for (int e = 0; e < W; e++) pre[e] = e == 0 ? den[0] : qm31_mul(pre[e - 1], den[e]);
    qm31 cur = qm31_inv(pre[W - 1]);
    qm31 r[W];
#pragma unroll
    for (int e = W - 1; e >= 0; e--) {
        const qm31 inv = e == 0 ? cur : qm31_mul(pre[e - 1], cur);
        cur = qm31_mul(cur, den[e]);
        r[e] = qm31_mul(num[e], inv);
    }
    if (a.has_prev) {
        u32 p0[W], p1[W], p2[W], p3[W];
        load_w<W>(a.prev.p[0], row, p0); load_w<W>(a.prev.p[1], row, p1);
        load_w<W>(a.prev.p[2], row, p2); load_w<W>(a.prev.p[3], row, p3);
#pragma unroll
        for (int e = 0; e < W; e++) r[e] = qm31_add(r[e], qm31{p0[e], p1[e], p2[e], p3[e]});
    }
    if constexpr (W == 4) {
        gstore4(a.out.p[0], row, make_uint4(r[0].a, r[1].a, r[2].a, r[3].a));
        gstore4(a.out.p[1], row, make_uint4(r[0].b, r[1].b, r[2].b, r[3].b));
        gstore4(a.out.p[2], row, make_uint4(r[0].c, r[1].c, r[2].c, r[3].c));
        gstore4(a.out.p[3], row, make_uint4(r[0].d, r[1].d, r[2].d, r[3].d));
    } else {
        gstore1(a.out.p[0], row, r[0].a); gstore1(a.out.p[1], row, r[0].b);
        gstore1(a.out.p[2], row, r[0].c); gstore1(a.out.p[3], row, r[0].d);
    }
}

// ---------------------------------------------------------------- denominators of a LogUp-GKR input layer
// tstwo_gkr_logup_denominators: out[r] = sum_t coeff_t cols_t[r] + constant, the linear form above written out as a secure MLE
// instead of being inverted.  W rows per lane as in k_logup_column; the column pointers and the coefficients are kernel arguments
// read at a wave-uniform index (scalar loads).  64-bit sums of canonical M31 x M31 products, folded after every fourth term: a
// folded sum is below 2^33 and four more products add less than 4 (P - 1)^2, so 16 terms of (P - 1) (P - 1) stay below 2^64.
struct DenCoef { qm31 c[kMaxTerms]; };

template <int W>
__global__ void __launch_bounds__(kThreads) k_gkr_logup_den(ColPtrs cols, DenCoef coef, qm31 constant, u32 n_terms, Soa4 out, u32 n_rows) {
    const u32 t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_rows / W) return;
    const u32 row = t * W;
    u64 acc[W][4];
#pragma unroll
    for (int e = 0; e < W; e++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[e][j] = 0;
#pragma unroll 1
    for (u32 k = 0; k < n_terms; k++) {
        const qm31 q = coef.c[uni(k)];
        u32 x[W];
        load_w<W>(colp_u(cols, k), row, x);
#pragma unroll
        for (int e = 0; e < W; e++) {
            acc[e][0] += (u64)q.a * x[e];
            acc[e][1] += (u64)q.b * x[e];
            acc[e][2] += (u64)q.c * x[e];
            acc[e][3] += (u64)q.d * x[e];
        }
        if ((k & 3) == 3) {
#pragma unroll
            for (int e = 0; e < W; e++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[e][j] = fold64(acc[e][j]);
        }
    }
    u32 r[4][W];
#pragma unroll
    for (int e = 0; e < W; e++) {
        r[0][e] = m31_add(m31_reduce_u64(acc[e][0]), constant.a); r[1][e] = m31_add(m31_reduce_u64(acc[e][1]), constant.b);
        r[2][e] = m31_add(m31_reduce_u64(acc[e][2]), constant.c); r[3][e] = m31_add(m31_reduce_u64(acc[e][3]), constant.d);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (W == 4) gstore4(out.p[j], row, make_uint4(r[j][0], r[j][1], r[j][2], r[j][3]));
        else gstore1(out.p[j], row, r[j][0]);
    }
}

// ---------------------------------------------------------------- coset-order prefix sum
constexpr u32 kR = 7, kG = 16;                          // blocks of 2^7 j (256 coset rows), 16 blocks per tile
constexpr u32 kRuns = 1u << kR, kRunWords = 2 * kG;      // a tile: 128 runs of 32 words
constexpr u32 kRunStride = kRunWords + 1;                // LDS row pitch (odd: the lanes of a block walk down a column)
constexpr u32 kTileWords = kRuns * kRunStride;
constexpr u32 kMinTiledLog = 1 + kR + 4 + 1;             // L - R - log2 G >= 1: at least two tiles
constexpr u32 kSmallMax = 1u << (kMinTiledLog - 1);      // up to here the whole column sits in LDS (16 KiB)
constexpr u32 kLanesPerBlock = 8;
static_assert(kThreads == 2 * kG * kLanesPerBlock, "8 lanes per block, 2G blocks per workgroup");
static_assert((1u << 4) == kG, "kMinTiledLog assumes G = 16");

// 2^(-log) mod P = 2^(31 - log) (2^31 = 1 mod P)
__device__ __forceinline__ u32 inv_pow2(u32 log) { return log == 0 ? 1u : (1u << (31 - log)); }

// inclusive scan of v over the workgroup's lanes (LDS, Hillis-Steele); *total = the sum of all lanes.  Every lane calls it.
__device__ u32 wg_scan(u32 v, u32 *sh, u32 *total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (u32 o = 1; o < kThreads; o <<= 1) {
        const u32 x = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
        __syncthreads();
        sh[threadIdx.x] = m31_add(sh[threadIdx.x], x);
        __syncthreads();
    }
    const u32 r = sh[threadIdx.x];
    *total = sh[kThreads - 1];
    __syncthreads();
    return r;
}

// one workgroup per coordinate, the whole column (at most kSmallMax words) in LDS; claimed[coord] = its sum
__global__ void __launch_bounds__(kThreads) k_logup_small(Soa4 col, u32 log_n, u32 *claimed) {
    __shared__ u32 v[kSmallMax];
    __shared__ u32 sh[kThreads];
    u32 *c = col.p[blockIdx.y];
    const u32 n = 1u << log_n, L = log_n - 1;
    for (u32 i = threadIdx.x; i < n; i += kThreads) v[i] = gload1(c, i);
    __syncthreads();
    const u32 per = (n + kThreads - 1) / kThreads;      // coset rows per lane
    const u32 k0 = min(n, threadIdx.x * per), k1 = min(n, k0 + per);
    u64 part = 0;
    for (u32 k = k0; k < k1; k++) part += v[k];          // the plain sum, in any order
    u32 total;
    (void)wg_scan(m31_reduce_u64(part), sh, &total);
    const u32 s = m31_mul(total, inv_pow2(log_n));
    u32 mine = 0;
    for (u32 k = k0; k < k1; k++) mine = m31_add(mine, m31_sub(v[coset_pos(k, L)], s));
    u32 unused;
    u32 run = m31_sub(wg_scan(mine, sh, &unused), mine);
    for (u32 k = k0; k < k1; k++) {
        const u32 p = coset_pos(k, L);
        run = m31_add(run, m31_sub(v[p], s));
        v[p] = run;
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < n; i += kThreads) gstore1(c, i, v[i]);
    if (threadIdx.x == 0) claimed[blockIdx.y] = total;
}

struct TileArgs {
    Soa4 col;
    u32 *sums;                       // [4][n_blocks] block sums, then prefixes; then s of each coordinate at [4 n_blocks + coord]
    u32 L, n_blocks, n_tiles;        // n_blocks = 2^(L - R), n_tiles = n_blocks / G
};

// tiles g0 and n_tiles - 1 - g0 <-> t[0], t[1]: run x of tile g holds words [2 (x 2^(L-R) + g G), + 2G)
template <bool VEC>
__device__ __forceinline__ void tile_io(u32 *c, u32 (*t)[kTileWords], const TileArgs &a, u32 g0, bool store) {
    const u32 stride = a.n_blocks;
    for (u32 w = 0; w < 2; w++) {
        const u32 g = w ? a.n_tiles - 1u - g0 : g0;
        if constexpr (VEC) {
            for (u32 q = threadIdx.x; q < kRuns * kRunWords / 4; q += kThreads) {
                const u32 x = q / (kRunWords / 4), o = (q % (kRunWords / 4)) * 4;
                const u32 gi = 2u * (x * stride + g * kG) + o;
                u32 *l = &t[w][x * kRunStride + o];
                if (store) {
                    gstore4(c, gi, make_uint4(l[0], l[1], l[2], l[3]));
                } else {
                    const uint4 v = gload4(c, gi);
                    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
                }
            }
        } else {
            for (u32 q = threadIdx.x; q < kRuns * kRunWords; q += kThreads) {
                const u32 x = q / kRunWords, o = q % kRunWords;
                const u32 gi = 2u * (x * stride + g * kG) + o;
                if (store) gstore1(c, gi, t[w][x * kRunStride + o]);
                else t[w][x * kRunStride + o] = gload1(c, gi);
            }
        }
    }
}

// Block (which, y) of the workgroup (8 lanes, 16 lows each in coset order): the A part of low (x = rev_R(low)) at
// t[which][x][2y], the B part at t[1 - which][2^R - 1 - x][2 (G - 1 - y) + 1].
template <bool SCAN, bool VEC>
__global__ void __launch_bounds__(kThreads) k_logup_tile(TileArgs a) {
    __shared__ u32 t[2][kTileWords];
    u32 *c = a.col.p[blockIdx.y];
    u32 *sums = a.sums + (size_t)blockIdx.y * a.n_blocks;
    const u32 g0 = blockIdx.x;
    tile_io<VEC>(c, t, a, g0, false);
    __syncthreads();
    const u32 blk = threadIdx.x / kLanesPerBlock, lane = threadIdx.x % kLanesPerBlock;
    const u32 which = blk / kG, y = blk % kG;
    const u32 g = which ? a.n_tiles - 1u - g0 : g0;
    const u32 top = rev_bits(g * kG + y, a.L - kR);
    u32 *ta = t[which], *tb = t[1 - which];
    constexpr u32 per = kRuns / kLanesPerBlock;
    const u32 lo0 = lane * per;
    const u32 ya = 2 * y, yb = 2 * (kG - 1 - y) + 1;
    if constexpr (!SCAN) {
        u64 part = 0;
        for (u32 low = lo0; low < lo0 + per; low++) {
            const u32 x = rev_bits(low, kR);
            part += ta[x * kRunStride + ya];
            part += tb[(kRuns - 1 - x) * kRunStride + yb];
        }
        u32 v = m31_reduce_u64(part);
#pragma unroll
        for (u32 o = kLanesPerBlock / 2; o >= 1; o >>= 1) v = m31_add(v, __shfl_xor(v, o, kLanesPerBlock));
        if (lane == 0) sums[top] = v;
    } else {
        const u32 s = a.sums[4 * a.n_blocks + blockIdx.y];
        u32 mine = 0;
        for (u32 low = lo0; low < lo0 + per; low++) {
            const u32 x = rev_bits(low, kR);
            mine = m31_add(mine, m31_sub(ta[x * kRunStride + ya], s));
            mine = m31_add(mine, m31_sub(tb[(kRuns - 1 - x) * kRunStride + yb], s));
        }
        u32 incl = mine;
#pragma unroll
        for (u32 o = 1; o < kLanesPerBlock; o <<= 1) {
            const u32 x = __shfl_up(incl, o, kLanesPerBlock);
            if (lane >= o) incl = m31_add(incl, x);
        }
        u32 run = m31_add(sums[top], m31_sub(incl, mine));
        for (u32 low = lo0; low < lo0 + per; low++) {
            const u32 x = rev_bits(low, kR);
            u32 *pa = &ta[x * kRunStride + ya], *pb = &tb[(kRuns - 1 - x) * kRunStride + yb];
            run = m31_add(run, m31_sub(*pa, s));
            *pa = run;
            run = m31_add(run, m31_sub(*pb, s));
            *pb = run;
        }
        __syncthreads();
        tile_io<VEC>(c, t, a, g0, true);
    }
}

// one workgroup per coordinate (blockIdx.x): claimed = the sum of the block sums, s = claimed / 2^log_n, and the block sums
// replaced by the exclusive prefix of (block sum - 2^(R+1) s)
__global__ void __launch_bounds__(kThreads) k_logup_block_scan(u32 *sums, u32 n_blocks, u32 log_n, u32 *claimed) {
    __shared__ u32 sh[kThreads];
    u32 *b = sums + (size_t)blockIdx.x * n_blocks;
    const u32 per = (n_blocks + kThreads - 1) / kThreads;
    const u32 k0 = min(n_blocks, threadIdx.x * per), k1 = min(n_blocks, k0 + per);
    u64 part = 0;
    for (u32 k = k0; k < k1; k++) part += b[k];
    const u32 raw = m31_reduce_u64(part);
    u32 total;
    const u32 incl = wg_scan(raw, sh, &total);
    const u32 s = m31_mul(total, inv_pow2(log_n));
    const u32 bs = m31_mul(s, 1u << (kR + 1));
    u32 run = m31_sub(incl, raw);
    for (u32 k = k0; k < k1; k++) {
        const u32 v = b[k];
        b[k] = m31_sub(run, m31_mul(k, bs));
        run = m31_add(run, v);
    }
    if (threadIdx.x == 0) {
        sums[4 * (size_t)n_blocks + blockIdx.x] = s;
        claimed[blockIdx.x] = total;
    }
}

// ---------------------------------------------------------------- host
int bad(const std::string &msg) { return set_error(TSTWO_ERR_BAD_ARG, msg); }

}  // namespace

extern "C" {

int tstwo_logup_column(const tstwo_logup_frac *fracs, size_t n_fracs, const u32 *const prev[4], u32 log_size, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    if (!fracs) return bad("logup column: null fraction table");
    if (n_fracs == 0 || n_fracs > kMaxFracs) return bad("logup column: 1 to 8 fractions per column");
    if (log_size > kMaxLog) return bad("logup column: log_size above 28");
    TSTWO_REQUIRE_TABLE(out, 4);
    if (prev) TSTWO_REQUIRE_TABLE(prev, 4);
    // the descriptors travel through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the logup fraction descriptors cannot be recorded)");
    const u32 n = 1u << log_size;
    bool vec = n % 4 == 0;
    for (int j = 0; j < 4; j++) vec = vec && aligned16(out[j]) && (!prev || aligned16(prev[j]));
    u32 staged[kMaxFracs * kDescWords] = {};
    for (size_t b = 0; b < n_fracs; b++) {
        const tstwo_logup_frac &f = fracs[b];
        u32 *w = staged + b * kDescWords;
        if (f.n_terms == 0 || f.n_terms > kMaxTerms) return bad("logup column: 1 to 16 terms per fraction");
        if (!f.cols || !f.coeffs) return bad("logup column: null host argument");
        TSTWO_REQUIRE_TABLE(f.cols, f.n_terms);
        for (int j = 0; j < 4; j++) {
            if (f.constant[j] >= M31_P) return bad("logup column: constant out of range");
            w[kDescConst + j] = f.constant[j];
        }
        for (u32 k = 0; k < 4 * f.n_terms; k++) {
            if (f.coeffs[k] >= M31_P) return bad("logup column: coefficient word out of range");
            w[kDescCoeff + k] = f.coeffs[k];
        }
        for (u32 k = 0; k < f.n_terms; k++) {
            const uint64_t p = (uint64_t)(uintptr_t)f.cols[k];
            w[kDescCols + 2 * k] = (u32)p;
            w[kDescCols + 2 * k + 1] = (u32)(p >> 32);
            vec = vec && aligned16(f.cols[k]);
        }
        if (f.num) {
            const uint64_t p = (uint64_t)(uintptr_t)f.num;
            w[kDescNum] = (u32)p;
            w[kDescNum + 1] = (u32)(p >> 32);
            vec = vec && aligned16(f.num);
        } else if (f.num_const >= M31_P) {
            return bad("logup column: constant numerator out of range");
        }
        w[kDescNumConst] = f.num_const;
        w[kDescNTerms] = f.n_terms;
    }
    const size_t bytes = n_fracs * kDescWords * sizeof(u32);
    if (int rc = ensure_scratch(bytes)) return rc;
    if (int rc = small_h2d(ctx().scratch, staged, bytes)) return rc;
    ColArgs a = {};
    a.desc = ctx().scratch;
    for (int j = 0; j < 4; j++) {
        a.prev.p[j] = prev ? prev[j] : nullptr;
        a.out.p[j] = out[j];
    }
    a.n_fracs = (u32)n_fracs;
    a.n_rows = n;
    a.has_prev = prev ? 1u : 0u;
    a.flag = ctx().flag;
    if (vec) hipLaunchKernelGGL(k_logup_column<4>, dim3(ceil_div(n / 4, kThreads)), dim3(kThreads), 0, ctx().stream, a);
    else hipLaunchKernelGGL(k_logup_column<1>, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, ctx().stream, a);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_gkr_logup_denominators(const u32 *const *cols, const u32 *coeffs, size_t n_terms, const u32 constant[4], u32 log_n,
                                 u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    if (n_terms == 0 || n_terms > kMaxTerms) return bad("logup denominators: 1 to 16 terms");
    if (log_n > kMaxLog) return bad("logup denominators: log_n above 28");
    if (!cols || !coeffs || !constant) return bad("logup denominators: null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_terms); TSTWO_REQUIRE_TABLE(out, 4);
    const u32 n = 1u << log_n;
    bool vec = n % 4 == 0;
    DenCoef coef = {};
    for (size_t k = 0; k < n_terms; k++) {
        for (int j = 0; j < 4; j++)
            if (coeffs[4 * k + j] >= M31_P) return bad("logup denominators: coefficient word out of range");
        coef.c[k] = to_q(coeffs + 4 * k);
        for (int j = 0; j < 4; j++)
            if (out[j] < cols[k] + n && cols[k] < out[j] + n) return bad("logup denominators: an output column is also an input");
        vec = vec && aligned16(cols[k]);
    }
    for (int j = 0; j < 4; j++) {
        if (constant[j] >= M31_P) return bad("logup denominators: constant out of range");
        vec = vec && aligned16(out[j]);
    }
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_terms, 0)) return rc;
    const Soa4 o = {{out[0], out[1], out[2], out[3]}};
    if (vec) hipLaunchKernelGGL(k_gkr_logup_den<4>, dim3(ceil_div(n / 4, kThreads)), dim3(kThreads), 0, ctx().stream, cp, coef, to_q(constant), (u32)n_terms, o, n);
    else hipLaunchKernelGGL(k_gkr_logup_den<1>, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, ctx().stream, cp, coef, to_q(constant), (u32)n_terms, o, n);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_logup_finalize_last(u32 *const col[4], u32 log_size, u32 claimed_sum[4]) {
    TSTWO_REQUIRE_READY();
    if (log_size < 1 || log_size > kMaxLog) return bad("logup finalize: log_size must be 1 to 28");
    TSTWO_REQUIRE_TABLE(col, 4);
    if (!claimed_sum) return bad("logup finalize: null host argument");
    if (stream_is_capturing()) return bad("host read-back during graph capture (the logup claimed sum cannot be recorded)");
    Soa4 c4 = {{col[0], col[1], col[2], col[3]}};
    if (log_size < kMinTiledLog) {
        if (int rc = ensure_scratch(4 * sizeof(u32))) return rc;
        hipLaunchKernelGGL(k_logup_small, dim3(1, 4), dim3(kThreads), 0, ctx().stream, c4, log_size, ctx().scratch);
        TSTWO_LAUNCH_CHECK();
        return small_d2h(claimed_sum, ctx().scratch, 4 * sizeof(u32));
    }
    TileArgs a = {};
    a.col = c4;
    a.L = log_size - 1;
    a.n_blocks = 1u << (a.L - kR);
    a.n_tiles = a.n_blocks / kG;
    const size_t words = 4 * (size_t)a.n_blocks + 8;      // block sums, s per coordinate, claimed
    if (int rc = ensure_scratch(words * sizeof(u32))) return rc;
    a.sums = ctx().scratch;
    u32 *claimed = a.sums + 4 * (size_t)a.n_blocks + 4;
    bool vec = true;
    for (int j = 0; j < 4; j++) vec = vec && aligned16(col[j]);
    const dim3 grid(a.n_tiles / 2, 4);
    if (vec) hipLaunchKernelGGL((k_logup_tile<false, true>), grid, dim3(kThreads), 0, ctx().stream, a);
    else hipLaunchKernelGGL((k_logup_tile<false, false>), grid, dim3(kThreads), 0, ctx().stream, a);
    TSTWO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_logup_block_scan, dim3(4), dim3(kThreads), 0, ctx().stream, a.sums, a.n_blocks, log_size, claimed);
    TSTWO_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL((k_logup_tile<true, true>), grid, dim3(kThreads), 0, ctx().stream, a);
    else hipLaunchKernelGGL((k_logup_tile<true, false>), grid, dim3(kThreads), 0, ctx().stream, a);
    TSTWO_LAUNCH_CHECK();
    return small_d2h(claimed_sum, claimed, 4 * sizeof(u32));
}

}  // extern "C"

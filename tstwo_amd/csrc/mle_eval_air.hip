// mle_eval_air.hip — the device side of the mle_eval AIR component (tstwo_amd/mle_eval.py), which proves
//     sum_p eq(p, r) L[p] = v,      L[p] = w_0 + sum_k w_k c_k[p]
// over committed base columns c_k: the statement that ties a claim on a LogUp-GKR input layer to the trace.  The eq table is
// tstwo_gkr_gen_eq_evals over the whole point and the running sum is tstwo_logup_finalize_last; this file adds the two steps
// between and beside them.  Both are streams: a grid-stride loop at 256 lanes, W = 4 consecutive rows per lane (16-byte
// accesses) when every column is 16-byte aligned, else one row; the grid is capped at kMaxBlocks workgroups.
//
// k_mle_eval_selectors<W>: the 2n + 2 preprocessed 0/1 columns of log size n.  With d = the bit reversal of the storage
// position p over n bits (the circle-domain index of the row), h = 2^(n-1), d' = d mod h and t = the number of trailing one
// bits of d' (n - 1 when d' = h - 1):
//     G_t[p] = [d < h and t(p) = t]      K_t[p] = [d >= h and t(p) = t]      F0[p] = [d = 0]      F1[p] = [d = h]
// in the order G_0 .. G_{n-1}, K_0 .. K_{n-1}, F0, F1.  A mask offset of +2 moves d to d + 1 (mod h) inside the first half
// and to d - 1 (mod h) inside the second, and bit j of d is variable j of the eq table, so t says which coordinates of the
// point the step from a row to its neighbour exchanges.  A lane works out the one column of G u K that holds a 1 on each of
// its rows and then walks the columns (a wave-uniform index: the pointer is one scalar load), storing the comparison: every
// word of every column is written exactly once, nothing is read.
//
// k_mle_eval_terms<W>: out[p] = eq[p] (constant + sum_k coeffs_k cols_k[p]), QM31 eq, coefficients and constant, M31 columns.
// The linear form is accumulated as in k_gkr_logup_den (logup.hip): 64-bit sums of canonical M31 x M31 products, folded after
// every fourth term (a folded sum is below 2^33 and four more products add less than 4 (P - 1)^2: 16 terms of (P - 1) (P - 1)
// stay below 2^64), then one QM31 product per row.  A lane loads its rows of eq before it stores them, and no other lane
// touches them: out may be eq itself, column for column.  Nothing is inverted, so the zero flag is not touched.
// Algorithmic bytes per row: 16 (eq) + 4 n_terms (columns) + 16 (out).
#include <string>

#include "common.h"
#include "coset_order.cuh"

using namespace tstwo;

namespace {

constexpr u32 kMaxTerms = TSTWO_LOGUP_MAX_TERMS;
constexpr u32 kMinLog = 2, kMaxLog = TSTWO_LOGUP_MAX_LOG;
constexpr int kThreads = 256;
// Workgroups per launch: 32 per CU of the MI355X (fri.hip, field_ops.hip: streams of this shape run 5-6 % faster at 32+
// workgroups per CU than at 8).  A constant, so that the size at which the loop takes a second trip is the same everywhere:
// 2^21 lanes per trip, i.e. log_size 24 at 4 rows per lane and 22 at one.
constexpr u32 kMaxBlocks = 8192;
static_assert(2 * kMaxLog + 2 <= (u32)kMaxColsPerLaunch, "the selector columns must fit the by-value pointer table");

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

template <int W>
__device__ __forceinline__ void store_w(u32 *col, u32 row, const u32 (&x)[W]) {
    if constexpr (W == 4) gstore4(col, row, make_uint4(x[0], x[1], x[2], x[3]));
    else gstore1(col, row, x[0]);
}

// (ColPtrs first: colp_u reads the by-value table at the start of the kernel-argument segment)
template <int W>
__global__ void __launch_bounds__(kThreads) k_mle_eval_selectors(ColPtrs out, u32 log_n, u32 n_lanes) {
    const u32 stride = gridDim.x * kThreads;
    const u32 h = 1u << (log_n - 1);
#pragma unroll 1
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < n_lanes; t += stride) {
        const u32 row = t * W;
        u32 code[W], f0[W], f1[W];                 // code: the column of G (0 .. n-1) or K (n .. 2n-1) that is 1 on the row
#pragma unroll
        for (int e = 0; e < W; e++) {
            const u32 d = rev_bits(row + (u32)e, log_n);
            const u32 dp = d & (h - 1u);
            const u32 ones = dp == h - 1u ? log_n - 1u : (u32)__builtin_ctz(~dp);
            code[e] = d < h ? ones : log_n + ones;
            f0[e] = d == 0u ? 1u : 0u;
            f1[e] = d == h ? 1u : 0u;
        }
#pragma unroll 1
        for (u32 c = 0; c < 2 * log_n; c++) {
            u32 v[W];
#pragma unroll
            for (int e = 0; e < W; e++) v[e] = code[e] == c ? 1u : 0u;
            store_w<W>(colp_u(out, c), row, v);
        }
        store_w<W>(colp_u(out, 2 * log_n), row, f0);
        store_w<W>(colp_u(out, 2 * log_n + 1), row, f1);
    }
}

struct TermCoef { qm31 c[kMaxTerms]; };

template <int W>
__global__ void __launch_bounds__(kThreads) k_mle_eval_terms(ColPtrs cols, TermCoef coef, qm31 constant, u32 n_terms, CSoa4 eq, Soa4 out,
                                                             u32 n_lanes) {
    const u32 stride = gridDim.x * kThreads;
#pragma unroll 1
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < n_lanes; t += stride) {
        const u32 row = t * W;
        u32 e0[W], e1[W], e2[W], e3[W];           // in flight while the form is summed
        load_w<W>(eq.p[0], row, e0); load_w<W>(eq.p[1], row, e1);
        load_w<W>(eq.p[2], row, e2); load_w<W>(eq.p[3], row, e3);
        u64 acc[W][4];
#pragma unroll
        for (int e = 0; e < W; e++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[e][j] = 0;
#pragma unroll 1
        for (u32 k = 0; k < n_terms; k++) {
            const qm31 q = coef.c[(u32)__builtin_amdgcn_readfirstlane((int)k)];
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
            const qm31 form = {m31_add(m31_reduce_u64(acc[e][0]), constant.a), m31_add(m31_reduce_u64(acc[e][1]), constant.b),
                               m31_add(m31_reduce_u64(acc[e][2]), constant.c), m31_add(m31_reduce_u64(acc[e][3]), constant.d)};
            const qm31 v = qm31_mul(qm31{e0[e], e1[e], e2[e], e3[e]}, form);
            r[0][e] = v.a; r[1][e] = v.b; r[2][e] = v.c; r[3][e] = v.d;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) store_w<W>(out.p[j], row, r[j]);
    }
}

unsigned grid_of(u32 n_lanes) {
    const unsigned blocks = ceil_div(n_lanes, kThreads);
    return blocks < kMaxBlocks ? blocks : kMaxBlocks;
}

bool overlap(const u32 *a, const u32 *b, size_t n) { return a < b + n && b < a + n; }

}  // namespace

extern "C" {

int tstwo_mle_eval_selectors(u32 log_size, u32 *const *out) {
    TSTWO_REQUIRE_READY();
    if (log_size < kMinLog || log_size > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "mle eval selectors: log_size must be 2 to 28");
    const size_t n_cols = 2 * (size_t)log_size + 2;
    if (!out) return set_error(TSTWO_ERR_BAD_ARG, "mle eval selectors: null host argument");
    TSTWO_REQUIRE_TABLE(out, n_cols);
    const u32 n = 1u << log_size;
    bool vec = true;
    for (size_t c = 0; c < n_cols; c++) {
        vec = vec && aligned16(out[c]);
        for (size_t b = 0; b < c; b++)
            if (overlap(out[b], out[c], n)) return set_error(TSTWO_ERR_BAD_ARG, "mle eval selectors: two output columns overlap");
    }
    ColPtrs cp;
    if (int rc = fill_col_table(cp, out, n_cols, 0)) return rc;
    if (vec) hipLaunchKernelGGL(k_mle_eval_selectors<4>, dim3(grid_of(n / 4)), dim3(kThreads), 0, ctx().stream, cp, log_size, n / 4);
    else hipLaunchKernelGGL(k_mle_eval_selectors<1>, dim3(grid_of(n)), dim3(kThreads), 0, ctx().stream, cp, log_size, n);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_mle_eval_terms(const u32 *const eq[4], const u32 *const *cols, const u32 *coeffs, size_t n_terms, const u32 constant[4],
                         u32 log_size, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    auto bad = [](const char *msg) { return set_error(TSTWO_ERR_BAD_ARG, std::string("mle eval terms: ") + msg); };
    if (n_terms == 0 || n_terms > kMaxTerms) return bad("1 to 16 terms");
    if (log_size > kMaxLog) return bad("log_size above 28");
    if (!eq || !cols || !coeffs || !constant || !out) return bad("null host argument");
    TSTWO_REQUIRE_TABLE(eq, 4); TSTWO_REQUIRE_TABLE(cols, n_terms); TSTWO_REQUIRE_TABLE(out, 4);
    const u32 n = 1u << log_size;
    bool vec = n % 4 == 0;
    TermCoef coef = {};
    for (size_t k = 0; k < n_terms; k++) {
        for (int j = 0; j < 4; j++)
            if (coeffs[4 * k + j] >= M31_P) return bad("coefficient word out of range");
        coef.c[k] = to_q(coeffs + 4 * k);
        for (int j = 0; j < 4; j++)
            if (overlap(out[j], cols[k], n)) return bad("an output column is also an input");
        vec = vec && aligned16(cols[k]);
    }
    for (int j = 0; j < 4; j++) {
        if (constant[j] >= M31_P) return bad("constant out of range");
        vec = vec && aligned16(out[j]) && aligned16(eq[j]);
        // a lane reads its rows of eq before it writes them: out[j] == eq[j] is safe, any other overlap is not
        for (int i = 0; i < 4; i++) {
            if (i == j && out[j] == eq[i]) continue;
            if (overlap(out[j], eq[i], n)) return bad("out may alias eq only column for column");
            if (i < j && overlap(out[j], out[i], n)) return bad("two output columns overlap");
        }
    }
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_terms, 0)) return rc;
    const CSoa4 e = {{eq[0], eq[1], eq[2], eq[3]}};
    const Soa4 o = {{out[0], out[1], out[2], out[3]}};
    if (vec) hipLaunchKernelGGL(k_mle_eval_terms<4>, dim3(grid_of(n / 4)), dim3(kThreads), 0, ctx().stream, cp, coef, to_q(constant), (u32)n_terms, e, o, n / 4);
    else hipLaunchKernelGGL(k_mle_eval_terms<1>, dim3(grid_of(n)), dim3(kThreads), 0, ctx().stream, cp, coef, to_q(constant), (u32)n_terms, e, o, n);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // extern "C"

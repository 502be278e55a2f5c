// air.hip — constraint evaluation of an AIR over its trace on the evaluation domain (the device form of Rust stwo's
// FrameworkComponent::evaluate_constraint_quotients_on_domain, constraint_framework/component.rs; the reference carries the shapes in
// constraint_framework/index.ts and air/accumulator.ts) for constraints that read only their own row (mask offset 0), and the wide
// Fibonacci trace generator (examples/fibonacci.ts generateTrace, Rust examples/wide_fibonacci generate_trace).
//
// Constraint kinds:
//   TSTWO_AIR_WIDE_FIB  N >= 3 columns, c_i = x_{i+2} - (x_i^2 + x_{i+1}^2), i < N - 2  (WideFibonacciEval<N>)
//   TSTWO_AIR_MUL_ADD   3 columns,      c_0 = x_0 x_1 + x_0 - x_2                        (TestEval of the Rust tutorial's example 05)
// Row r (bit-reversed order on CanonicCoset(trace_log + log_expand).circle_domain()):
//   row_res = sum_i coeff_i c_i(r),   accum[r] += row_res * denom_inv[r >> trace_log]
//
// One lane owns W = 4 consecutive rows (16-byte loads: a wave reads 1 KiB of one column at a time, coalesced) and sweeps the columns
// once: every column is squared once, the last two squares stay in registers.  The four coordinates of row_res are sums of
// M31 x M31 products, kept in 64 bits: a product of canonical values is < 2^62, so four of them and a folded remainder (< 2^33) fit;
// the sum is folded (and/alignbit, no reduction to canonical) after every fourth constraint and reduced once per row at the end.
// The coefficients and the denominators travel in the kernel argument segment and are read with scalar loads (wave-uniform index).
#include "common.h"

using namespace tstwo;

namespace {

constexpr int kThreads = 256;
constexpr u32 kMaxConstraints = 128;         // 4 x 128 coefficient words in the kernel argument (N <= 130 wide-Fibonacci columns)
constexpr u32 kMaxLogExpand = 4;
constexpr u32 kMaxDenoms = 1u << kMaxLogExpand;
constexpr u32 kMaxLog = 28;                  // word offsets of gload*/gstore* stay below 2^30

struct AirArgs {
    u32 coeff[4 * kMaxConstraints];          // QM31 coefficient of constraint i at [4i, 4i + 4)
    u32 denom_inv[kMaxDenoms];
    Soa4 acc;
    u32 n_cols, n_constraints, trace_log, n_denoms, n_rows;
};
// AirArgs is the second kernel argument, directly behind the ColPtrs table (both 8-byte aligned)
constexpr int kArgsOff = (int)sizeof(ColPtrs);
static_assert(sizeof(ColPtrs) % 8 == 0, "AirArgs must follow ColPtrs without padding");
static_assert(sizeof(ColPtrs) + sizeof(AirArgs) <= 4096, "kernel arguments exceed 4 KiB");

// coefficient word j of constraint i straight from the kernel argument segment: one scalar load (no copy of the array to scratch)
__device__ __forceinline__ u32 coeff_word(u32 i, u32 j) {
    typedef const u32 __attribute__((address_space(4))) *k32;
    typedef const char __attribute__((address_space(4))) *kbytes;
    const k32 c = (k32)((kbytes)__builtin_amdgcn_kernarg_segment_ptr() + kArgsOff + offsetof(AirArgs, coeff));
    return c[(u32)__builtin_amdgcn_readfirstlane((int)(4 * i + j))];
}

template <int W>
__device__ __forceinline__ void load_rows(const u32 *col, u32 row, u32 (&x)[W]) {
    if (W == 4) {
        const uint4 v = gload4(col, row);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = gload1(col, row);
    }
}

// acc[e][j] += coeff_i[j] * c[e]
template <int W>
__device__ __forceinline__ void accumulate(u64 (&acc)[W][4], u32 i, const u32 (&c)[W]) {
    const u32 q0 = coeff_word(i, 0), q1 = coeff_word(i, 1), q2 = coeff_word(i, 2), q3 = coeff_word(i, 3);
#pragma unroll
    for (int e = 0; e < W; e++) {
        acc[e][0] += (u64)q0 * c[e];
        acc[e][1] += (u64)q1 * c[e];
        acc[e][2] += (u64)q2 * c[e];
        acc[e][3] += (u64)q3 * c[e];
    }
}
// x = t1 + 2^31 t2 + 2^63 t3 == t1 + t2 + 2 t3 (mod P), < 2^31 + 2 + 2^32 < 2^33: room for four more products
__device__ __forceinline__ u64 fold64(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 t2 = __builtin_amdgcn_alignbit(hi, lo, 31);
    return (u64)((lo & M31_P) + ((hi >> 31) << 1)) + t2;
}
template <int W>
__device__ __forceinline__ void fold_all(u64 (&acc)[W][4]) {
#pragma unroll
    for (int e = 0; e < W; e++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[e][j] = fold64(acc[e][j]);
}

// row_res of rows [row, row + W) into acc (unreduced)
template <int KIND, int W>
__device__ __forceinline__ void eval_rows(const ColPtrs &cols, const AirArgs &a, u32 row, u64 (&acc)[W][4]) {
    if (KIND == TSTWO_AIR_MUL_ADD) {
        u32 x0[W], x1[W], x2[W], c[W];
        load_rows<W>(colp_u(cols, 0), row, x0);
        load_rows<W>(colp_u(cols, 1), row, x1);
        load_rows<W>(colp_u(cols, 2), row, x2);
#pragma unroll
        for (int e = 0; e < W; e++) c[e] = m31_sub(m31_add(m31_mul(x0[e], x1[e]), x0[e]), x2[e]);
        accumulate<W>(acc, 0, c);
        return;
    }
    // TSTWO_AIR_WIDE_FIB: constraint i reads columns i, i + 1 (as squares) and i + 2
    u32 s2[W], s1[W], x[W];
    load_rows<W>(colp_u(cols, 0), row, x);
#pragma unroll
    for (int e = 0; e < W; e++) s2[e] = m31_sqr(x[e]);
    load_rows<W>(colp_u(cols, 1), row, x);
#pragma unroll
    for (int e = 0; e < W; e++) s1[e] = m31_sqr(x[e]);
    const u32 n_c = a.n_constraints;
#pragma unroll 1
    for (u32 i0 = 0; i0 < n_c; i0 += 4) {
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const u32 i = i0 + j;
            if (i < n_c) {                      // wave-uniform
                u32 c[W];
                load_rows<W>(colp_u(cols, i + 2), row, x);
#pragma unroll
                for (int e = 0; e < W; e++) {
                    c[e] = m31_sub(x[e], m31_add(s2[e], s1[e]));
                    s2[e] = s1[e];
                    s1[e] = m31_sqr(x[e]);
                }
                accumulate<W>(acc, i, c);
            }
        }
        fold_all<W>(acc);
    }
}

template <int KIND, int W>
__global__ void __launch_bounds__(kThreads) k_constraint_quotients(ColPtrs cols, AirArgs a) {
    const u32 stride = gridDim.x * kThreads;
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < a.n_rows / W; t += stride) {
        const u32 row = t * W;
        u64 acc[W][4];
#pragma unroll
        for (int e = 0; e < W; e++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[e][j] = 0;
        eval_rows<KIND, W>(cols, a, row, acc);
        u32 r[4][W];
#pragma unroll
        for (int e = 0; e < W; e++) {
            // denom_inv[(row + e) >> trace_log]: a select over the (<= 16, wave-uniform) table, no indexed private array
            const u32 di = (row + e) >> a.trace_log;
            u32 d = a.denom_inv[0];
#pragma unroll
            for (u32 k = 1; k < kMaxDenoms; k++)
                if (k < a.n_denoms && di == k) d = a.denom_inv[k];
#pragma unroll
            for (int j = 0; j < 4; j++) r[j][e] = m31_mul(m31_reduce_u64(acc[e][j]), d);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (W == 4) {
                const uint4 o = gload4(a.acc.p[j], row);
                gstore4(a.acc.p[j], row, make_uint4(m31_add(o.x, r[j][0]), m31_add(o.y, r[j][1]), m31_add(o.z, r[j][2]), m31_add(o.w, r[j][3])));
            } else {
                gstore1(a.acc.p[j], row, m31_add(gload1(a.acc.p[j], row), r[j][0]));
            }
        }
    }
}

// ---------------------------------------------------------------- wide Fibonacci trace
// out[0] = a, out[1] = b, out[k] = out[k-2]^2 + out[k-1]^2
template <int W>
__global__ void __launch_bounds__(kThreads) k_wide_fib_trace(ColPtrs out, const u32 *a, const u32 *b, u32 n, u32 n_cols) {
    const u32 stride = gridDim.x * kThreads;
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < n / W; t += stride) {
        const u32 row = t * W;
        u32 x0[W], x1[W], s2[W], s1[W];
        load_rows<W>(a, row, x0);
        load_rows<W>(b, row, x1);
#pragma unroll
        for (int e = 0; e < W; e++) { s2[e] = m31_sqr(x0[e]); s1[e] = m31_sqr(x1[e]); }
        if (W == 4) {
            gstore4(colp_u(out, 0), row, make_uint4(x0[0], x0[1], x0[2], x0[3]));
            gstore4(colp_u(out, 1), row, make_uint4(x1[0], x1[1], x1[2], x1[3]));
        } else {
            gstore1(colp_u(out, 0), row, x0[0]);
            gstore1(colp_u(out, 1), row, x1[0]);
        }
#pragma unroll 1
        for (u32 k = 2; k < n_cols; k++) {
            u32 x[W];
#pragma unroll
            for (int e = 0; e < W; e++) {
                x[e] = m31_add(s2[e], s1[e]);
                s2[e] = s1[e];
                s1[e] = m31_sqr(x[e]);
            }
            if (W == 4) gstore4(colp_u(out, k), row, make_uint4(x[0], x[1], x[2], x[3]));
            else gstore1(colp_u(out, k), row, x[0]);
        }
    }
}

unsigned grid_for(size_t work) {
    unsigned b = ceil_div(work, kThreads);
    const unsigned cap = (unsigned)ctx().n_cus * 16;
    if (b > cap) b = cap;
    return b ? b : 1;
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool table_aligned16(const u32 *const *t, size_t n) {
    for (size_t i = 0; i < n; i++) if (!aligned16(t[i])) return false;
    return true;
}

template <int KIND>
int launch_quotients(const ColPtrs &cp, const AirArgs &a, bool vec) {
    if (vec) hipLaunchKernelGGL((k_constraint_quotients<KIND, 4>), dim3(grid_for(a.n_rows / 4)), dim3(kThreads), 0, ctx().stream, cp, a);
    else hipLaunchKernelGGL((k_constraint_quotients<KIND, 1>), dim3(grid_for(a.n_rows)), dim3(kThreads), 0, ctx().stream, cp, a);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // namespace

extern "C" {

int tstwo_air_wide_fib_trace(const u32 *a, const u32 *b, u32 log_n, u32 *const *cols, size_t n_cols) {
    TSTWO_REQUIRE_READY();
    if (n_cols < 2) return set_error(TSTWO_ERR_BAD_ARG, "wide Fibonacci needs at least 2 columns");
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "trace too large");
    TSTWO_REQUIRE_PTRS(a, b);
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    const u32 n = 1u << log_n;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, (const u32 *const *)cols, n_cols, 0)) return rc;
    const bool vec = n % 4 == 0 && aligned16(a) && aligned16(b) && table_aligned16((const u32 *const *)cols, n_cols);
    if (vec) hipLaunchKernelGGL(k_wide_fib_trace<4>, dim3(grid_for(n / 4)), dim3(kThreads), 0, ctx().stream, cp, a, b, n, (u32)n_cols);
    else hipLaunchKernelGGL(k_wide_fib_trace<1>, dim3(grid_for(n)), dim3(kThreads), 0, ctx().stream, cp, a, b, n, (u32)n_cols);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_air_constraint_quotients(u32 kind, const u32 *const *cols, size_t n_cols, u32 trace_log_size, u32 log_expand,
                                   const u32 *coeffs, size_t n_constraints, const u32 *denom_inv, u32 *const accum[4]) {
    TSTWO_REQUIRE_READY();
    if (kind == TSTWO_AIR_WIDE_FIB) {
        if (n_cols < 3 || n_constraints != n_cols - 2) return set_error(TSTWO_ERR_BAD_ARG, "wide Fibonacci: N >= 3 columns, N - 2 constraints");
    } else if (kind == TSTWO_AIR_MUL_ADD) {
        if (n_cols != 3 || n_constraints != 1) return set_error(TSTWO_ERR_BAD_ARG, "mul-add: 3 columns, 1 constraint");
    } else {
        return set_error(TSTWO_ERR_BAD_ARG, "unknown constraint kind");
    }
    if (n_constraints > kMaxConstraints) return set_error(TSTWO_ERR_BAD_ARG, "too many constraints in one component");
    if (log_expand > kMaxLogExpand) return set_error(TSTWO_ERR_BAD_ARG, "log_expand too large");
    if (trace_log_size + log_expand > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "evaluation domain too large");
    if (!coeffs || !denom_inv) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    TSTWO_REQUIRE_TABLE(accum, 4);
    AirArgs a = {};
    for (size_t i = 0; i < 4 * n_constraints; i++) {
        if (coeffs[i] >= M31_P) return set_error(TSTWO_ERR_BAD_ARG, "coefficient word out of range");
        a.coeff[i] = coeffs[i];
    }
    a.n_denoms = 1u << log_expand;
    for (u32 i = 0; i < a.n_denoms; i++) {
        if (denom_inv[i] >= M31_P) return set_error(TSTWO_ERR_BAD_ARG, "denominator out of range");
        a.denom_inv[i] = denom_inv[i];
    }
    for (int j = 0; j < 4; j++) a.acc.p[j] = accum[j];
    a.n_cols = (u32)n_cols;
    a.n_constraints = (u32)n_constraints;
    a.trace_log = trace_log_size;
    a.n_rows = 1u << (trace_log_size + log_expand);
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    bool vec = a.n_rows % 4 == 0 && table_aligned16(cols, n_cols);
    for (int j = 0; j < 4; j++) vec = vec && aligned16(accum[j]);
    return kind == TSTWO_AIR_WIDE_FIB ? launch_quotients<TSTWO_AIR_WIDE_FIB>(cp, a, vec) : launch_quotients<TSTWO_AIR_MUL_ADD>(cp, a, vec);
}

}  // extern "C"

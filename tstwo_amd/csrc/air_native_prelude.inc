R"AIRN(// The device helpers of every generated AIR kernel (csrc/air_codegen.h puts this text in front of the kernels it writes;
// csrc/air_native.hip compiles the whole with hipRTC).  It restates, for a compiler that sees no header of the library, what
// air.hip, m31.cuh and common.h give k_air_program: the same arithmetic on the same words, so results are bit-identical.
// No LDS and no run-time indexed array: every value is a local variable, and the compiler allocates VGPRs and schedules loads.
typedef unsigned int u32;
typedef unsigned long long u64;
#define M31_P 2147483647u
#define AIRN_DEV __device__ inline __attribute__((always_inline))
#define AIRN_GLOBAL __attribute__((address_space(1)))
#define AIRN_CONST __attribute__((address_space(4)))

namespace airn {

typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
typedef const u32 AIRN_CONST *k32;
typedef const u64 AIRN_CONST *k64;

// the kernel arguments, as csrc/common.h (ColPtrs) and csrc/air_native.hip (NativeArgs) fill them
struct ColPtrs { u32 *p[64]; u32 *const *ext; };
struct Soa4 { u32 *p[4]; };
struct NativeArgs {
    const u32 *coeff;                        // device: 4 coefficient words per constraint
    u32 denom_inv[16];
    Soa4 acc;
    u32 n_rows, trace_log, eval_log, log_expand, n_denoms, stride;   // stride: lanes of the whole grid
};

// ---------------------------------------------------------------- M31 (canonical in, canonical out)
AIRN_DEV u32 min_u32(u32 a, u32 b) { return a < b ? a : b; }
AIRN_DEV u32 m31_add(u32 a, u32 b) { const u32 s = a + b; return min_u32(s, s - M31_P); }
AIRN_DEV u32 m31_sub(u32 a, u32 b) { const u32 d = a - b; return min_u32(d, d + M31_P); }
AIRN_DEV u32 m31_neg(u32 a) { return m31_sub(0u, a); }
AIRN_DEV u32 m31_reduce64(u64 p) {            // p < 2^62
    const u32 s = ((u32)p & M31_P) + (u32)(p >> 31);
    return min_u32(s, s - M31_P);
}
AIRN_DEV u32 m31_mul(u32 a, u32 b) { return m31_reduce64((u64)a * (u64)b); }
AIRN_DEV u32 m31_sqr(u32 a) { return m31_mul(a, a); }
// any x < 2^64: x = t1 + 2^31 t2 + 2^63 t3 == t1 + (t2 & P) + (t2 >> 31) + 2 t3 (mod P)
AIRN_DEV u32 m31_reduce_u64(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 t2 = __builtin_amdgcn_alignbit(hi, lo, 31), t3 = hi >> 31;
    u32 s = (lo & M31_P) + (t2 & M31_P);
    s = min_u32(s, s - M31_P);
    s = s + (t2 >> 31) + t3 + t3;
    return min_u32(s, s - M31_P);
}
// x == t1 + t2 + 2 t3 (mod P), < 2^33: room for four more products of canonical values
AIRN_DEV u64 fold64(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 t2 = __builtin_amdgcn_alignbit(hi, lo, 31);
    return (u64)((lo & M31_P) + ((hi >> 31) << 1)) + t2;
}

// ---------------------------------------------------------------- column accesses: a scalar base and a 32-bit word offset < 2^30
AIRN_DEV u32 gload1(const u32 *base, u32 word_off) { return *(const AIRN_GLOBAL u32 *)((const AIRN_GLOBAL char *)base + (word_off << 2)); }
AIRN_DEV u32x4_t gload4(const u32 *base, u32 word_off) { return *(const AIRN_GLOBAL u32x4_t *)((const AIRN_GLOBAL char *)base + (word_off << 2)); }
AIRN_DEV void gstore1(u32 *base, u32 word_off, u32 x) { *(AIRN_GLOBAL u32 *)((AIRN_GLOBAL char *)base + (word_off << 2)) = x; }
AIRN_DEV void gstore4(u32 *base, u32 word_off, u32x4_t x) { *(AIRN_GLOBAL u32x4_t *)((AIRN_GLOBAL char *)base + (word_off << 2)) = x; }

// The column table through the constant address space: the device table (more than 64 columns) or the by-value table at the
// start of the kernel-argument segment.  Column indices are constants of the generated text, so column i is one scalar load at
// an immediate offset.
AIRN_DEV k64 col_table(const ColPtrs &c) { return c.ext ? (k64)(u64)c.ext : (k64)__builtin_amdgcn_kernarg_segment_ptr(); }
AIRN_DEV u32 *col_at(k64 tab, u32 i) { return (u32 *)tab[i]; }

// ---------------------------------------------------------------- the W rows of one lane
template <int W> struct Rows { u32 v[W]; };

template <int W> AIRN_DEV Rows<W> load_rows(const u32 *col, u32 row) {
    Rows<W> r;
    if constexpr (W == 4) {
        const u32x4_t x = gload4(col, row);
        r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
    } else {
        r.v[0] = gload1(col, row);
    }
    return r;
}
template <int W> AIRN_DEV Rows<W> load_at(const u32 *col, const Rows<W> &rows) {
    Rows<W> r;
#pragma unroll
    for (int e = 0; e < W; e++) r.v[e] = gload1(col, rows.v[e]);
    return r;
}
// offset_bit_reversed_circle_domain_index: the bit-reversed position of the row `off` trace steps away from row r (air.hip)
AIRN_DEV u32 neighbour_row(u32 r, u32 eval_log, u32 log_expand, int off) {
    const u32 i = __builtin_bitreverse32(r) >> (32 - eval_log);
    const u32 half = 1u << (eval_log - 1);
    const u32 step = (u32)off << (log_expand - 1);
    const u32 hi = i & half;
    const u32 j = ((hi ? i - step : i + step) & (half - 1)) | hi;
    return __builtin_bitreverse32(j) >> (32 - eval_log);
}
template <int W> AIRN_DEV Rows<W> neighbour_rows(u32 row, u32 eval_log, u32 log_expand, int off) {
    Rows<W> r;
#pragma unroll
    for (int e = 0; e < W; e++) r.v[e] = neighbour_row(row + e, eval_log, log_expand, off);
    return r;
}
template <int W> AIRN_DEV Rows<W> r_const(u32 c) {
    Rows<W> r;
#pragma unroll
    for (int e = 0; e < W; e++) r.v[e] = c;
    return r;
}
#define AIRN_BINARY(name, fn)                                                       \
    template <int W> AIRN_DEV Rows<W> name(const Rows<W> &a, const Rows<W> &b) {    \
        Rows<W> r;                                                                  \
        _Pragma("unroll") for (int e = 0; e < W; e++) r.v[e] = fn(a.v[e], b.v[e]); \
        return r;                                                                   \
    }
#define AIRN_UNARY(name, fn)                                                 \
    template <int W> AIRN_DEV Rows<W> name(const Rows<W> &a) {               \
        Rows<W> r;                                                           \
        _Pragma("unroll") for (int e = 0; e < W; e++) r.v[e] = fn(a.v[e]);  \
        return r;                                                            \
    }
AIRN_BINARY(r_add, m31_add)
AIRN_BINARY(r_sub, m31_sub)
AIRN_BINARY(r_mul, m31_mul)
AIRN_UNARY(r_sqr, m31_sqr)
AIRN_UNARY(r_neg, m31_neg)

// acc[e][j] += q_j * v[e]: a product of canonical values is < 2^62, so four of them and a folded remainder fit 64 bits
template <int W> AIRN_DEV void accumulate(u64 (&acc)[W][4], const Rows<W> &v, u32 q0, u32 q1, u32 q2, u32 q3) {
#pragma unroll
    for (int e = 0; e < W; e++) {
        acc[e][0] += (u64)q0 * v.v[e];
        acc[e][1] += (u64)q1 * v.v[e];
        acc[e][2] += (u64)q2 * v.v[e];
        acc[e][3] += (u64)q3 * v.v[e];
    }
}
template <int W> AIRN_DEV void fold_all(u64 (&acc)[W][4]) {
#pragma unroll
    for (int e = 0; e < W; e++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[e][j] = fold64(acc[e][j]);
}

}  // namespace airn

// The row epilogue: accum[row + e] += reduce(acc[e]) * denom_inv[(row + e) >> trace_log].  A macro on the kernel argument itself,
// as the row epilogue of air.hip (a function changes how the scalar loads of the table and the pointers are scheduled); the
// denominator is a select over the wave-uniform table, no indexed private array.
#define AIRN_ADD_ROWS(W, a, row, acc)                                                                                     \
    do {                                                                                                                  \
        u32 r_[4][W];                                                                                                     \
        _Pragma("unroll") for (int e = 0; e < W; e++) {                                                                   \
            const u32 di = ((row) + e) >> (a).trace_log;                                                                  \
            u32 d = (a).denom_inv[0];                                                                                     \
            _Pragma("unroll") for (u32 k = 1; k < 16; k++)                                                                \
                if (k < (a).n_denoms && di == k) d = (a).denom_inv[k];                                                    \
            _Pragma("unroll") for (int j = 0; j < 4; j++) r_[j][e] = m31_mul(m31_reduce_u64((acc)[e][j]), d);             \
        }                                                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                   \
            if constexpr (W == 4) {                                                                                       \
                const u32x4_t o = gload4((a).acc.p[j], row);                                                              \
                u32x4_t s;                                                                                                \
                s.x = m31_add(o.x, r_[j][0]); s.y = m31_add(o.y, r_[j][1]);                                               \
                s.z = m31_add(o.z, r_[j][2]); s.w = m31_add(o.w, r_[j][3]);                                               \
                gstore4((a).acc.p[j], row, s);                                                                            \
            } else {                                                                                                      \
                gstore1((a).acc.p[j], row, m31_add(gload1((a).acc.p[j], row), r_[j][0]));                                 \
            }                                                                                                             \
        }                                                                                                                 \
    } while (0)
)AIRN"

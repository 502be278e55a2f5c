// air.hip — constraint evaluation of an AIR over its trace on the evaluation domain (the device form of Rust stwo's
// FrameworkComponent::evaluate_constraint_quotients_on_domain, constraint_framework/component.rs; the reference carries the shapes in
// constraint_framework/index.ts and air/accumulator.ts), and the wide Fibonacci trace generator (examples/fibonacci.ts
// generateTrace, Rust examples/wide_fibonacci generate_trace).  Two kernels evaluate constraints, with one contract:
//   k_constraint_quotients<KIND, W>  hand-written constraints that read only their own row (mask offset 0):
//     TSTWO_AIR_WIDE_FIB  N >= 3 columns, c_i = x_{i+2} - (x_i^2 + x_{i+1}^2), i < N - 2  (WideFibonacciEval<N>)
//     TSTWO_AIR_MUL_ADD   3 columns,      c_0 = x_0 x_1 + x_0 - x_2                        (TestEval of the Rust tutorial's example 05)
//   k_air_program<W>  any constraints, as a straight-line program (tstwo_amd/constraint_framework.py compiles a FrameworkEval's
//     `evaluate` into it) interpreted for every row, with loads at row offsets (Rust stwo constraint_framework:
//     next_interaction_mask with offsets, utils.rs offset_bit_reversed_circle_domain_index).
//   k_air_columns<W>  the same programs on the trace domain itself, with STORE in place of ACC: every stored register becomes
//     one output column (tstwo_air_eval_columns: the numerators and denominator terms of a LogUp interaction trace, derived
//     from `evaluate` by tstwo_amd/logup.py derive_interaction_trace).  It shares the interpreter with k_air_program
//     (fetch, exec_op, the LDS register file) and has no accumulators, coefficients or denominators.
//   k_air_check<W>  the same programs on the trace domain with a reduction in place of the store: per constraint the number of
//     rows on which it is non-zero and the first of them in coset order (tstwo_air_check_constraints: a trace satisfies the AIR
//     exactly when every count is 0).  The third user of the interpreter.
//   tstwo_air_eval_compiled  the contract and argument checks of k_air_program's entry, run by a kernel that air_native.hip
//     compiled from the program (air_codegen.h writes its source; the program validator of all three entries lives there).
//   tstwo_air_eval_columns_compiled  the same for k_air_columns: the entry's argument checks, a kernel compiled from the STORE
//     program (tstwo_air_columns_compile), and no upload at all, so it can be recorded into a graph.
// Row r (bit-reversed order on CanonicCoset(trace_log + log_expand).circle_domain()):
//   row_res = sum_i coeff_i c_i(r),   accum[r] += row_res * denom_inv[r >> trace_log]
//
// Launch shapes (W, grid, LDS, what is uploaded where) and the range checks of the arguments: csrc/air_plan.h, for every entry.
// Both: one lane owns W = 4 consecutive rows (16-byte loads: a wave reads 1 KiB of one column at a time, coalesced) or W = 1
// (air_plan.h says when).  The four coordinates of row_res are sums of M31 x M31 products, kept in
// 64 bits: a product of canonical values is < 2^62, so four of them and a folded remainder (< 2^33) fit; the sum is folded
// (and/alignbit, no reduction to canonical) after every fourth constraint and reduced once per row at the end.  The denominators
// travel in the kernel argument segment.
//
// k_constraint_quotients sweeps the columns once: every column is squared once, the last two squares stay in registers.  The
// coefficients travel in the kernel argument segment and are read with scalar loads (wave-uniform index).
//
// k_air_program reads the program words with scalar loads (constant address space, wave-uniform program counter), so the opcode
// lands in an SGPR and every dispatch is a scalar branch — no lane branches on an opcode.
// Temporaries: a register file in LDS, [reg][lane] of W-word vectors (one 16-byte slot per lane and register when W = 4).  A lane
// only touches its own slots, so no barrier is needed; registers indexed at run time never reach private (scratch) memory.
// Workgroups are one wave: the LDS a workgroup needs is n_regs KiB (W = 4), and residency falls with it, not with a block size.
// Loads at offset 0 of W = 4 rows are one 16-byte global load; loads at other offsets gather per row (the neighbour of four
// consecutive rows is not four consecutive rows: rows r and r + 1 sit in opposite halves of the circle domain and move in
// opposite directions), with the index computed per row.  Across a wave the gathered rows are still runs of consecutive rows
// (the offset moves the high bits of r), so the loads of one instruction cover the same cache lines as an offset-0 load.
#include <algorithm>
#include <string>

#include "air_codegen.h"
#include "air_native.h"
#include "air_plan.h"
#include "common.h"

using namespace tstwo;

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr u32 kMaxConstraints = kAirMaxConstraints;          // 4 x 128 coefficient words in the kernel argument (N <= 130 wide-Fibonacci columns)
constexpr u32 kMaxDenoms = 1u << kAirMaxLogExpand;
static_assert(TSTWO_AIR_PROGRAM_MAX_COLS <= 0x10000, "the column operand is 16 bits wide");

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

struct ProgArgs {
    const u32 *prog;                         // device: 2 words per instruction, then 4 coefficient words per constraint
    u32 denom_inv[kMaxDenoms];
    Soa4 acc;
    u32 n_instr, n_rows, trace_log, eval_log, log_expand, n_denoms;
};

struct ColArgs {
    const u32 *prog;                         // device: 2 words per instruction
    u32 n_instr, n_rows, log;
};
// k_air_columns(ColPtrs cols, ColPtrs out, ColArgs): the output table is the second kernel argument (kSecondTableOff)
static_assert(2 * sizeof(ColPtrs) + sizeof(ColArgs) <= 4096, "kernel arguments exceed 4 KiB");
static_assert(TSTWO_AIR_COLUMNS_MAX_OUT <= kMaxColsPerLaunch, "the output table travels by value");

struct CheckArgs {
    const u32 *prog;                         // device: 2 words per instruction; the host sets dst = 1 in the last ACC of a constraint
    u32 *report;                             // device: (failing rows, first failing coset row) per constraint
    u32 n_instr, n_rows, log, n_constraints;
    u32 tally;                               // word offset of the workgroup's (count, first row) pairs in LDS, behind the registers
};
static_assert(sizeof(ColPtrs) + sizeof(CheckArgs) <= 4096, "kernel arguments exceed 4 KiB");
constexpr u32 kNoRow = 0xffffffffu;          // the report's "no failing row"

// ---------------------------------------------------------------- shared by both kernels
template <int W>
__device__ __forceinline__ void load_rows(const u32 *col, u32 row, u32 (&x)[W]) {
    if constexpr (W == 4) {
        const uint4 v = gload4(col, row);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = gload1(col, row);
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

// The row epilogue of both kernels: accum[row + e] += reduce(acc[e]) * denom_inv[(row + e) >> trace_log], `a` the kernel's AirArgs
// or ProgArgs.  A macro, not a function: handing the kernel argument to a function, even a forced-inline one, changes how the
// compiler schedules the scalar loads of the denominator table and the accumulator pointers.
#define TSTWO_AIR_ADD_ROWS(W, a, row, acc)                                                                                      \
    do {                                                                                                                        \
        u32 r_[4][W];                                                                                                           \
        _Pragma("unroll") for (int e = 0; e < W; e++) {                                                                         \
            /* denom_inv[(row + e) >> trace_log]: a select over the (<= 16, wave-uniform) table, no indexed private array */   \
            const u32 di = ((row) + e) >> (a).trace_log;                                                                        \
            u32 d = (a).denom_inv[0];                                                                                           \
            _Pragma("unroll") for (u32 k = 1; k < kMaxDenoms; k++)                                                              \
                if (k < (a).n_denoms && di == k) d = (a).denom_inv[k];                                                          \
            _Pragma("unroll") for (int j = 0; j < 4; j++) r_[j][e] = m31_mul(m31_reduce_u64((acc)[e][j]), d);                   \
        }                                                                                                                       \
        _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                         \
            if constexpr (W == 4) {                                                                                             \
                const uint4 o = gload4((a).acc.p[j], row);                                                                      \
                gstore4((a).acc.p[j], row, make_uint4(m31_add(o.x, r_[j][0]), m31_add(o.y, r_[j][1]), m31_add(o.z, r_[j][2]),   \
                                                      m31_add(o.w, r_[j][3])));                                                 \
            } else {                                                                                                            \
                gstore1((a).acc.p[j], row, m31_add(gload1((a).acc.p[j], row), r_[j][0]));                                       \
            }                                                                                                                   \
        }                                                                                                                       \
    } while (0)

// ---------------------------------------------------------------- hand-written constraints
// coefficient word j of constraint i straight from the kernel argument segment: one scalar load (no copy of the array to scratch)
__device__ __forceinline__ u32 coeff_word(u32 i, u32 j) {
    typedef const u32 __attribute__((address_space(4))) *k32;
    typedef const char __attribute__((address_space(4))) *kbytes;
    const k32 c = (k32)((kbytes)__builtin_amdgcn_kernarg_segment_ptr() + kArgsOff + offsetof(AirArgs, coeff));
    return c[(u32)__builtin_amdgcn_readfirstlane((int)(4 * i + j))];
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
        TSTWO_AIR_ADD_ROWS(W, a, row, acc);
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

// ---------------------------------------------------------------- the program interpreter
typedef const u32 __attribute__((address_space(4))) *k32;

__device__ __forceinline__ u32 uni(u32 x) { return (u32)__builtin_amdgcn_readfirstlane((int)x); }

// offset_bit_reversed_circle_domain_index: the bit-reversed position of the row `off` trace steps away from row r.  One trace
// step is 2^(log_expand - 1) steps of the evaluation domain's half coset; the first half of the domain walks forward, the
// second (the conjugates) backward.
__device__ __forceinline__ u32 neighbour_row(u32 r, u32 eval_log, u32 log_expand, int off) {
    const u32 i = __builtin_bitreverse32(r) >> (32 - eval_log);
    const u32 half = 1u << (eval_log - 1);
    const u32 step = (u32)off << (log_expand - 1);
    const u32 hi = i & half;
    const u32 j = ((hi ? i - step : i + step) & (half - 1)) | hi;
    return __builtin_bitreverse32(j) >> (32 - eval_log);
}

// The same on the trace domain itself (the eval_log == trace_log case of offset_bit_reversed_circle_domain_index): one trace step
// crosses between the two halves of the circle domain, so the shift above does not apply.  In coset order the neighbour of row k
// is row (k + off) mod 2^log.  With L = log - 1 and rev the bit reversal over L bits, coset row k = 2 j + odd sits at position
// 2 t + odd where t = rev(j) for even k and ~rev(j) (over L bits) for odd k (csrc/logup.hip); the inverse is the same two steps
// backwards, so a neighbour costs two bit reversals.
__device__ __forceinline__ u32 rev_bits(u32 x, u32 bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0; }
// the coset row k of bit-reversed position r (k_air_check reports rows in this order: the trace as the user wrote it)
__device__ __forceinline__ u32 coset_row(u32 r, u32 log) {
    const u32 L = log - 1, mask = (1u << L) - 1;
    const u32 odd = r & 1, t = r >> 1;
    return 2 * rev_bits(odd ? ~t & mask : t, L) + odd;
}
__device__ __forceinline__ u32 trace_neighbour_row(u32 r, u32 log, int off) {
    const u32 L = log - 1, mask = (1u << L) - 1;
    const u32 k = coset_row(r, log);
    const u32 k2 = (k + (u32)off) & ((1u << log) - 1);
    const u32 odd2 = k2 & 1, t2 = rev_bits(k2 >> 1, L);
    return 2 * (odd2 ? ~t2 & mask : t2) + odd2;
}

template <int W>
__device__ __forceinline__ void lds_read(const u32 *regs, u32 reg, u32 (&v)[W]) {
    const u32 lane = threadIdx.x;
    if constexpr (W == 4) {
        const uint4 x = *(const uint4 *)(regs + (reg * kWave + lane) * 4);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        v[0] = regs[reg * kWave + lane];
    }
}
template <int W>
__device__ __forceinline__ void lds_write(u32 *regs, u32 reg, const u32 (&v)[W]) {
    const u32 lane = threadIdx.x;
    if constexpr (W == 4) *(uint4 *)(regs + (reg * kWave + lane) * 4) = make_uint4(v[0], v[1], v[2], v[3]);
    else regs[reg * kWave + lane] = v[0];
}

// One instruction, fetched with scalar loads (wave-uniform program counter): w0 = op | dst << 8 | x << 16, w1.
struct Instr { u32 op, dst, x, w1; };
__device__ __forceinline__ Instr fetch(k32 prog, u32 pc) {
    const u32 w0 = prog[uni(2 * pc)], w1 = prog[uni(2 * pc + 1)];
    return {w0 & 0xffu, (w0 >> 8) & 0xffu, w0 >> 16, w1};
}

// The row a LOAD at a non-zero offset reads: on the evaluation domain (k_air_program) or on the trace domain (k_air_columns).
struct EvalNeighbour {
    u32 eval_log, log_expand;
    __device__ __forceinline__ u32 operator()(u32 r, int off) const { return neighbour_row(r, eval_log, log_expand, off); }
};
struct TraceNeighbour {
    u32 log;
    __device__ __forceinline__ u32 operator()(u32 r, int off) const { return trace_neighbour_row(r, log, off); }
};

// Every instruction that writes a register (LOAD, CONST, ADD, SUB, MUL, SQR, NEG): r[dst] of rows [row, row + W).  The kernels
// handle their own terminal instruction (ACC, STORE) before they come here.
template <int W, class Neighbour>
__device__ __forceinline__ void exec_op(const ColPtrs &cols, u32 *regs, const Instr &in, u32 row, const Neighbour &nb) {
    const u32 op = in.op, x = in.x, w1 = in.w1;
    u32 v[W];
    if (op == TSTWO_AIR_OP_LOAD) {
        const u32 *col = colp_u(cols, x);
        const int off = (int)w1;
        if (off == 0) {
            load_rows<W>(col, row, v);
        } else {
#pragma unroll
            for (int e = 0; e < W; e++) v[e] = gload1(col, nb(row + e, off));
        }
    } else if (op == TSTWO_AIR_OP_CONST) {
#pragma unroll
        for (int e = 0; e < W; e++) v[e] = w1;
    } else {
        u32 p[W];
        lds_read<W>(regs, x, p);
        if (op == TSTWO_AIR_OP_SQR) {
#pragma unroll
            for (int e = 0; e < W; e++) v[e] = m31_sqr(p[e]);
        } else if (op == TSTWO_AIR_OP_NEG) {
#pragma unroll
            for (int e = 0; e < W; e++) v[e] = m31_neg(p[e]);
        } else {
            u32 q[W];
            lds_read<W>(regs, w1, q);
            if (op == TSTWO_AIR_OP_ADD) {
#pragma unroll
                for (int e = 0; e < W; e++) v[e] = m31_add(p[e], q[e]);
            } else if (op == TSTWO_AIR_OP_SUB) {
#pragma unroll
                for (int e = 0; e < W; e++) v[e] = m31_sub(p[e], q[e]);
            } else {
#pragma unroll
                for (int e = 0; e < W; e++) v[e] = m31_mul(p[e], q[e]);
            }
        }
    }
    lds_write<W>(regs, in.dst, v);
}

template <int W>
__global__ void __launch_bounds__(kWave) k_air_program(ColPtrs cols, ProgArgs a) {
    extern __shared__ u32 regs[];
    const k32 prog = (k32)a.prog;
    const u32 coeff_base = 2 * a.n_instr;
    const u32 stride = gridDim.x * kWave;
    const EvalNeighbour nb = {a.eval_log, a.log_expand};
    for (u32 t = blockIdx.x * kWave + threadIdx.x; t < a.n_rows / W; t += stride) {
        const u32 row = t * W;
        u64 acc[W][4];
#pragma unroll
        for (int e = 0; e < W; e++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[e][j] = 0;
        u32 n_acc = 0;
#pragma unroll 1
        for (u32 pc = 0; pc < a.n_instr; pc++) {
            const Instr in = fetch(prog, pc);
            if (in.op == TSTWO_AIR_OP_ACC) {
                u32 v[W];
                lds_read<W>(regs, in.x, v);
                const u32 k = uni(coeff_base + 4 * n_acc);
                const u32 q0 = prog[k], q1 = prog[k + 1], q2 = prog[k + 2], q3 = prog[k + 3];
#pragma unroll
                for (int e = 0; e < W; e++) {
                    acc[e][0] += (u64)q0 * v[e];
                    acc[e][1] += (u64)q1 * v[e];
                    acc[e][2] += (u64)q2 * v[e];
                    acc[e][3] += (u64)q3 * v[e];
                }
                if ((++n_acc & 3) == 0) fold_all<W>(acc);
                continue;
            }
            exec_op<W>(cols, regs, in, row, nb);
        }
        TSTWO_AIR_ADD_ROWS(W, a, row, acc);
    }
}

// The interpreter on the trace domain: STORE writes r[x] of the lane's W rows to output column w1 (16 bytes per lane at W = 4,
// coalesced: a wave writes 1 KiB of one column).  An output is never an input (the host refuses it), so a load at an offset
// never reads a row another lane has stored.
template <int W>
__global__ void __launch_bounds__(kWave) k_air_columns(ColPtrs cols, ColPtrs out, ColArgs a) {
    extern __shared__ u32 regs[];
    const k32 prog = (k32)a.prog;
    const u32 stride = gridDim.x * kWave;
    const TraceNeighbour nb = {a.log};
    for (u32 t = blockIdx.x * kWave + threadIdx.x; t < a.n_rows / W; t += stride) {
        const u32 row = t * W;
#pragma unroll 1
        for (u32 pc = 0; pc < a.n_instr; pc++) {
            const Instr in = fetch(prog, pc);
            if (in.op == TSTWO_AIR_OP_STORE) {
                u32 v[W];
                lds_read<W>(regs, in.x, v);
                u32 *dst = colp_u<kSecondTableOff>(out, in.w1);
                if constexpr (W == 4) gstore4(dst, row, make_uint4(v[0], v[1], v[2], v[3]));
                else gstore1(dst, row, v[0]);
                continue;
            }
            exec_op<W>(cols, regs, in, row, nb);
        }
    }
}

// The interpreter on the trace domain with a reduction in place of a store (tstwo_air_check_constraints): an ACC ORs r[x] of the
// lane's W rows into `nz`, and the last ACC of a constraint (marked by the host in dst; a secure constraint is four ACCs) takes
// one ballot over the wave.  A clean trace pays nothing more.  A non-zero ballot counts the failing rows, finds the smallest of
// them in coset order (coset_row: computed on this path only) and adds both to the workgroup's pair for the constraint in LDS,
// behind the registers; workgroups are one wave, so lane 0 updates the pairs plainly.  Behind the grid-stride loop the workgroup
// issues one atomic add and one atomic min per constraint that failed in it, so the global atomics are bounded by workgroups x
// constraints even when every row fails.  k_air_check_init has written (0, kNoRow) to every pair of the report before.
// Can a register hold 2^31 - 1?  CONST is refused from 2^31 - 1 on, and m31_add / _sub / _neg / _mul / _sqr give canonical values
// for canonical operands, but LOAD copies the column's word as it is: a column that holds P (zero, not canonical) puts P in a
// register, and an ACC may read that register directly.  So every value is reduced (min(v, v - P): P -> 0, canonical values
// stay) before it is ORed in.
// The trip count is wave-uniform and no lane leaves the loop: below 64 lanes of rows the others run row 0 and vote zero.
__global__ void __launch_bounds__(kThreads) k_air_check_init(u32 *report, u32 n_constraints) {
    const u32 c = threadIdx.x;
    if (c < n_constraints) { report[2 * c] = 0; report[2 * c + 1] = kNoRow; }
}
static_assert(TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS <= kThreads, "k_air_check_init is one workgroup");

template <int W>
__global__ void __launch_bounds__(kWave) k_air_check(ColPtrs cols, CheckArgs a) {
    extern __shared__ u32 regs[];
    u32 *tally = regs + a.tally;
    const k32 prog = (k32)a.prog;
    const u32 lane = threadIdx.x;
    for (u32 c = lane; c < a.n_constraints; c += kWave) { tally[2 * c] = 0; tally[2 * c + 1] = kNoRow; }
    __syncthreads();
    const u32 n_lanes = a.n_rows / W, stride = gridDim.x * kWave;
    const TraceNeighbour nb = {a.log};
    for (u32 t0 = blockIdx.x * kWave; t0 < n_lanes; t0 += stride) {
        const bool live = t0 + lane < n_lanes;
        const u32 row = live ? (t0 + lane) * W : 0;
        u32 nz[W];
#pragma unroll
        for (int e = 0; e < W; e++) nz[e] = 0;
#pragma unroll 1
        for (u32 pc = 0; pc < a.n_instr; pc++) {
            const Instr in = fetch(prog, pc);
            if (in.op == TSTWO_AIR_OP_ACC) {
                u32 v[W];
                lds_read<W>(regs, in.x, v);
#pragma unroll
                for (int e = 0; e < W; e++) nz[e] |= min(v[e], v[e] - M31_P);
                if (in.dst == 0) continue;          // more ACCs of this constraint follow
                u32 any = 0;
#pragma unroll
                for (int e = 0; e < W; e++) any |= nz[e];
                if (__ballot(live && any != 0)) {   // wave-uniform
                    u32 count = 0, first = kNoRow;
#pragma unroll
                    for (int e = 0; e < W; e++)
                        if (live && nz[e] != 0) { count++; first = min(first, coset_row(row + e, a.log)); }
#pragma unroll
                    for (int s = kWave / 2; s; s >>= 1) {
                        count += (u32)__shfl_xor((int)count, s);
                        first = min(first, (u32)__shfl_xor((int)first, s));
                    }
                    if (lane == 0) {
                        tally[2 * in.w1] += count;
                        tally[2 * in.w1 + 1] = min(tally[2 * in.w1 + 1], first);
                    }
                }
#pragma unroll
                for (int e = 0; e < W; e++) nz[e] = 0;
                continue;
            }
            exec_op<W>(cols, regs, in, row, nb);
        }
    }
    __syncthreads();
    for (u32 c = lane; c < a.n_constraints; c += kWave) {
        const u32 count = tally[2 * c];
        if (count) {
            __hip_atomic_fetch_add(a.report + 2 * c, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(a.report + 2 * c + 1, tally[2 * c + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------- host
// Every entry: the range checks of its arguments (air_refuse), its pointer checks, the plan (air_plan), the upload, one launch.
int bad(const std::string &msg) { return set_error(TSTWO_ERR_BAD_ARG, msg); }

AirInput input_of(AirEntry entry, u32 log, u32 log_expand, size_t n_cols, size_t n_terminal, size_t program_len) {
    AirInput in = {};
    in.entry = entry, in.log = log, in.log_expand = log_expand, in.n_cols = n_cols, in.n_terminal = n_terminal, in.program_len = program_len;
    in.n_cus = (u32)ctx().n_cus;
    return in;
}
int refused(const AirInput &in, const char *why) { return bad(std::string(air_prefix(in.entry)) + why); }

// The plan's `aligned`: every column and accumulator (for tstwo_air_eval_columns: its n_out output columns) is 16-byte aligned.
bool table_aligned16(const u32 *const *t, size_t n) {
    for (size_t i = 0; i < n; i++) if (!aligned16(t[i])) return false;
    return true;
}
bool all_aligned16(const u32 *const *cols, size_t n_cols, u32 *const *accum, size_t n_accum) {
    return table_aligned16(cols, n_cols) && table_aligned16((const u32 *const *)accum, n_accum);
}

// range-checks the coefficient words (copied to coeff_dst) and the 2^log_expand denominators (copied into the kernel argument)
template <class Args>
int take_coeffs_and_denoms(const u32 *coeffs, size_t n_constraints, u32 *coeff_dst, const u32 *denom_inv, u32 log_expand, Args &a) {
    for (size_t i = 0; i < 4 * n_constraints; i++) {
        if (coeffs[i] >= M31_P) return bad("coefficient word out of range");
        coeff_dst[i] = coeffs[i];
    }
    a.n_denoms = 1u << log_expand;
    for (u32 i = 0; i < a.n_denoms; i++) {
        if (denom_inv[i] >= M31_P) return bad("denominator out of range");
        a.denom_inv[i] = denom_inv[i];
    }
    return TSTWO_OK;
}

// The pointers of tstwo_air_eval_program and tstwo_air_eval_compiled, and their refusal during capture.
int check_eval_pointers(const u32 *const *cols, size_t n_cols, const u32 *coeffs, const u32 *denom_inv, u32 *const accum[4]) {
    if (!coeffs || !denom_inv) return bad("null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    TSTWO_REQUIRE_TABLE(accum, 4);
    // the coefficient words (and the interpreter's program) travel through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the air program and its coefficients cannot be recorded)");
    return TSTWO_OK;
}

// The two tables of tstwo_air_eval_columns and tstwo_air_eval_columns_compiled.
int check_columns_tables(const u32 *const *cols, size_t n_cols, u32 *const *out, size_t n_out) {
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    TSTWO_REQUIRE_TABLE(out, n_out);
    // a load at an offset reads rows that other lanes store: no output may be an input (or another output)
    for (size_t k = 0; k < n_out; k++) {
        for (size_t i = 0; i < n_cols; i++)
            if (out[k] == cols[i]) return bad("air columns: an output column is also an input column");
        for (size_t i = 0; i < k; i++)
            if (out[k] == out[i]) return bad("air columns: two outputs are the same column");
    }
    return TSTWO_OK;
}

// The plan's upload (at most one slot of the ring: no host synchronisation) into the scratch block.
static_assert(kAirMaxUploadWords * sizeof(u32) <= kUpSlotBytes, "an upload exceeds one ring slot");
int upload(const AirPlan &p, const u32 *words) {
    if (int rc = ensure_scratch(p.upload_words * sizeof(u32))) return rc;
    return small_h2d(ctx().scratch, words, p.upload_words * sizeof(u32));
}

// One launch as the plan says: the W = 4 or the W = 1 instance of a kernel.
template <class F, class... A>
int launch(const AirPlan &p, F *k4, F *k1, const A &...args) {
    F *const k = p.w == 4 ? k4 : k1;
    hipLaunchKernelGGL(k, dim3(p.grid), dim3(p.threads), p.lds_bytes, ctx().stream, args...);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}
static_assert(kThreads == (int)kAirWideThreads && kWave == (int)kAirWaveThreads, "the kernels count lanes as the plan does");
static_assert(kAirTableByValue == (size_t)kMaxColsPerLaunch, "the plan's by-value limit is fill_col_table's");

}  // namespace

extern "C" {

int tstwo_air_wide_fib_trace(const u32 *a, const u32 *b, u32 log_n, u32 *const *cols, size_t n_cols) {
    TSTWO_REQUIRE_READY();
    AirInput in = input_of(kAirWideFibTrace, log_n, 0, n_cols, 0, 0);
    if (const char *why = air_refuse(in)) return refused(in, why);
    TSTWO_REQUIRE_PTRS(a, b);
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    ColPtrs cp;
    if (int rc = fill_col_table(cp, (const u32 *const *)cols, n_cols, 0)) return rc;
    in.aligned = aligned16(a) && aligned16(b) && table_aligned16((const u32 *const *)cols, n_cols);
    return launch(air_plan(in), k_wide_fib_trace<4>, k_wide_fib_trace<1>, cp, a, b, 1u << log_n, (u32)n_cols);
}

int tstwo_air_constraint_quotients(u32 kind, const u32 *const *cols, size_t n_cols, u32 trace_log_size, u32 log_expand,
                                   const u32 *coeffs, size_t n_constraints, const u32 *denom_inv, u32 *const accum[4]) {
    TSTWO_REQUIRE_READY();
    AirInput in = input_of(kAirQuotients, trace_log_size + log_expand, log_expand, n_cols, n_constraints, 0);
    in.kind = kind;
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (!coeffs || !denom_inv) return bad("null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    TSTWO_REQUIRE_TABLE(accum, 4);
    AirArgs a = {};
    if (int rc = take_coeffs_and_denoms(coeffs, n_constraints, a.coeff, denom_inv, log_expand, a)) return rc;
    for (int j = 0; j < 4; j++) a.acc.p[j] = accum[j];
    a.n_cols = (u32)n_cols;
    a.n_constraints = (u32)n_constraints;
    a.trace_log = trace_log_size;
    a.n_rows = 1u << in.log;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    in.aligned = all_aligned16(cols, n_cols, accum, 4);
    const AirPlan p = air_plan(in);
    return kind == TSTWO_AIR_WIDE_FIB ? launch(p, k_constraint_quotients<TSTWO_AIR_WIDE_FIB, 4>, k_constraint_quotients<TSTWO_AIR_WIDE_FIB, 1>, cp, a)
                                      : launch(p, k_constraint_quotients<TSTWO_AIR_MUL_ADD, 4>, k_constraint_quotients<TSTWO_AIR_MUL_ADD, 1>, cp, a);
}

int tstwo_air_eval_program(const u32 *const *cols, size_t n_cols, u32 trace_log_size, u32 log_expand, const u32 *program,
                           size_t program_len, const u32 *coeffs, size_t n_constraints, const u32 *denom_inv, u32 *const accum[4]) {
    TSTWO_REQUIRE_READY();
    AirInput in = input_of(kAirEvalProgram, trace_log_size + log_expand, log_expand, n_cols, n_constraints, program_len);
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (!program) return bad("null host argument");
    if (int rc = check_eval_pointers(cols, n_cols, coeffs, denom_inv, accum)) return rc;
    if (const char *why = check_acc_program(program, program_len, n_cols, n_constraints, in.n_regs)) return refused(in, why);
    in.aligned = all_aligned16(cols, n_cols, accum, 4);
    const AirPlan p = air_plan(in);
    u32 staged[kAirMaxUploadWords];             // program words, then coefficient words
    ProgArgs a = {};
    if (int rc = take_coeffs_and_denoms(coeffs, n_constraints, staged + p.coeff_word, denom_inv, log_expand, a)) return rc;
    std::copy(program, program + 2 * program_len, staged);
    if (int rc = upload(p, staged)) return rc;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    for (int j = 0; j < 4; j++) a.acc.p[j] = accum[j];
    a.prog = ctx().scratch;
    a.n_instr = (u32)program_len;
    a.trace_log = trace_log_size;
    a.eval_log = in.log;
    a.log_expand = log_expand;
    a.n_rows = 1u << in.log;
    return launch(p, k_air_program<4>, k_air_program<1>, cp, a);
}

int tstwo_air_eval_compiled(uint64_t kernel_id, const u32 *const *cols, size_t n_cols, u32 trace_log_size, u32 log_expand,
                            const u32 *coeffs, size_t n_constraints, const u32 *denom_inv, u32 *const accum[4]) {
    TSTWO_REQUIRE_READY();
    AirKernelKind kind;
    u32 for_cols = 0, for_constraints = 0;
    if (int rc = air_native_shape(kernel_id, kind, for_cols, for_constraints)) return rc;
    if (kind != kAirKernelConstraints) return bad("air program: the kernel was compiled from a columns program");
    AirInput in = input_of(kAirEvalCompiled, trace_log_size + log_expand, log_expand, n_cols, n_constraints, 0);
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (int rc = check_eval_pointers(cols, n_cols, coeffs, denom_inv, accum)) return rc;
    if (n_cols != for_cols) return bad("air kernel: compiled for another number of columns");
    if (n_constraints != for_constraints) return bad("air kernel: compiled for another number of constraints");
    in.aligned = all_aligned16(cols, n_cols, accum, 4);
    const AirPlan p = air_plan(in);
    u32 staged[4 * TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS];      // the coefficient words
    NativeArgs a = {};
    if (int rc = take_coeffs_and_denoms(coeffs, n_constraints, staged + p.coeff_word, denom_inv, log_expand, a)) return rc;
    if (int rc = upload(p, staged)) return rc;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    for (int j = 0; j < 4; j++) a.acc.p[j] = accum[j];
    a.coeff = ctx().scratch;
    a.trace_log = trace_log_size;
    a.eval_log = in.log;
    a.log_expand = log_expand;
    a.n_rows = 1u << in.log;
    return air_native_launch(kernel_id, p, cp, a);
}

int tstwo_air_eval_columns(const u32 *const *cols, size_t n_cols, u32 log_size, const u32 *program, size_t program_len,
                           u32 *const *out, size_t n_out) {
    TSTWO_REQUIRE_READY();
    AirInput in = input_of(kAirEvalColumns, log_size, 0, n_cols, n_out, program_len);
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (!program) return bad("null host argument");
    if (int rc = check_columns_tables(cols, n_cols, out, n_out)) return rc;
    // the program words travel through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the air columns program cannot be recorded)");
    if (const char *why = check_store_program(program, program_len, n_cols, n_out, in.n_regs)) return refused(in, why);
    in.aligned = all_aligned16(cols, n_cols, out, n_out);
    const AirPlan p = air_plan(in);
    if (int rc = upload(p, program)) return rc;
    ColPtrs cp, op;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    if (int rc = fill_col_table(op, (const u32 *const *)out, n_out, 1)) return rc;      // at most 64: by value
    ColArgs a = {};
    a.prog = ctx().scratch;
    a.n_instr = (u32)program_len;
    a.log = log_size;
    a.n_rows = 1u << log_size;
    return launch(p, k_air_columns<4>, k_air_columns<1>, cp, op, a);
}

int tstwo_air_eval_columns_compiled(uint64_t kernel_id, const u32 *const *cols, size_t n_cols, u32 log_size, u32 *const *out, size_t n_out) {
    TSTWO_REQUIRE_READY();
    AirKernelKind kind;
    u32 for_cols = 0, for_out = 0;
    if (int rc = air_native_shape(kernel_id, kind, for_cols, for_out)) return rc;
    if (kind != kAirKernelColumns) return bad("air columns: the kernel was compiled from a constraint program");
    AirInput in = input_of(kAirEvalColumnsCompiled, log_size, 0, n_cols, n_out, 0);
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (int rc = check_columns_tables(cols, n_cols, out, n_out)) return rc;
    if (n_cols != for_cols) return bad("air kernel: compiled for another number of columns");
    if (n_out != for_out) return bad("air kernel: compiled for another number of outputs");
    // nothing is uploaded: with at most 64 input columns both tables travel by value and the launch can be captured
    ColPtrs cp, op;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    if (int rc = fill_col_table(op, (const u32 *const *)out, n_out, 1)) return rc;      // at most 64: by value
    ColumnsArgs a = {};
    a.log = log_size;
    a.n_rows = 1u << log_size;
    in.aligned = all_aligned16(cols, n_cols, out, n_out);
    return air_native_launch_columns(kernel_id, air_plan(in), cp, op, a);
}

int tstwo_air_check_constraints(const u32 *const *cols, size_t n_cols, u32 log_size, const u32 *program, size_t program_len,
                                size_t n_constraints, u32 *report) {
    TSTWO_REQUIRE_READY();
    AirInput in = input_of(kAirCheck, log_size, 0, n_cols, n_constraints, program_len);
    if (const char *why = air_refuse(in)) return refused(in, why);
    if (!program) return bad("null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    if (!report || !aligned16(report)) return bad("air check: null or misaligned report");
    // the program words travel through the small-upload ring, which a captured graph cannot replay
    if (stream_is_capturing()) return bad("host-array upload during graph capture (the air check program cannot be recorded)");
    if (const char *why = check_assert_program(program, program_len, n_cols, n_constraints, in.n_regs)) return refused(in, why);
    in.aligned = table_aligned16(cols, n_cols);
    const AirPlan p = air_plan(in);
    u32 staged[2 * TSTWO_AIR_PROGRAM_MAX_INSTR];            // the program with the last ACC of every constraint marked: the kernel votes there
    mark_last_acc(program, program_len, staged);
    if (int rc = upload(p, staged)) return rc;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    CheckArgs a = {};
    a.prog = ctx().scratch;
    a.report = report;
    a.n_instr = (u32)program_len;
    a.log = log_size;
    a.n_rows = 1u << log_size;
    a.n_constraints = (u32)n_constraints;
    a.tally = p.tally_word;
    // the report in a launch of its own: the kernel's workgroups add to it in any order, and the grid may wrap
    hipLaunchKernelGGL(k_air_check_init, dim3(1), dim3(kThreads), 0, ctx().stream, report, a.n_constraints);
    TSTWO_LAUNCH_CHECK();
    return launch(p, k_air_check<4>, k_air_check<1>, cp, a);
}

}  // extern "C"

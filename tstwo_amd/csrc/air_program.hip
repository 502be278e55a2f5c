// air_program.hip — constraint evaluation of a user-defined AIR on the evaluation domain: the constraints arrive as a
// straight-line program (tstwo_amd/constraint_framework.py compiles a FrameworkEval's `evaluate` into it) and one kernel interprets
// it for every row.  Same contract as tstwo_air_constraint_quotients (air.hip), with loads at row offsets (Rust stwo
// constraint_framework: next_interaction_mask with offsets, utils.rs offset_bit_reversed_circle_domain_index).
//
// Row r (bit-reversed order on CanonicCoset(trace_log + log_expand).circle_domain()):
//   row_res = sum_k coeff_k e_k(r),   accum[r] += row_res * denom_inv[r >> trace_log]
//
// Decoding: the program words are read with scalar loads (constant address space, wave-uniform program counter), so the opcode
// lands in an SGPR and every dispatch is a scalar branch — no lane branches on an opcode.
// Temporaries: a register file in LDS, [reg][lane] of W-word vectors (one 16-byte slot per lane and register when W = 4).  A lane
// only touches its own slots, so no barrier is needed; registers indexed at run time never reach private (scratch) memory.
// Workgroups are one wave: the LDS a workgroup needs is n_regs KiB (W = 4), and residency falls with it, not with a block size.
// Loads at offset 0 of W = 4 rows are one 16-byte global load; loads at other offsets gather per row (the neighbour of four
// consecutive rows is not four consecutive rows: rows r and r + 1 sit in opposite halves of the circle domain and move in
// opposite directions), with the index computed per row.  Across a wave the gathered rows are still runs of consecutive rows
// (the offset moves the high bits of r), so the loads of one instruction cover the same cache lines as an offset-0 load.
// Accumulation as in air.hip: 64-bit sums of M31 x M31 products, folded after every fourth constraint, reduced once per row.
#include <algorithm>

#include "common.h"

using namespace tstwo;

namespace {

constexpr int kWave = 64;
constexpr u32 kMaxLogExpand = 4;
constexpr u32 kMaxDenoms = 1u << kMaxLogExpand;
constexpr u32 kMaxLog = 28;                  // word offsets of gload*/gstore* stay below 2^30
static_assert(TSTWO_AIR_PROGRAM_MAX_COLS <= 0x10000, "the column operand is 16 bits wide");

struct ProgArgs {
    const u32 *prog;                         // device: 2 words per instruction, then 4 coefficient words per constraint
    u32 denom_inv[kMaxDenoms];
    Soa4 acc;
    u32 n_instr, n_rows, trace_log, eval_log, log_expand, n_denoms;
};

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

__device__ __forceinline__ u64 fold64(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 t2 = __builtin_amdgcn_alignbit(hi, lo, 31);
    return (u64)((lo & M31_P) + ((hi >> 31) << 1)) + t2;
}

template <int W>
__global__ void __launch_bounds__(kWave) k_air_program(ColPtrs cols, ProgArgs a) {
    extern __shared__ u32 regs[];
    const k32 prog = (k32)a.prog;
    const u32 coeff_base = 2 * a.n_instr;
    const u32 stride = gridDim.x * kWave;
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
            const u32 w0 = prog[uni(2 * pc)], w1 = prog[uni(2 * pc + 1)];
            const u32 op = w0 & 0xffu, dst = (w0 >> 8) & 0xffu, x = w0 >> 16;
            u32 v[W];
            if (op == TSTWO_AIR_OP_LOAD) {
                const u32 *col = colp_u(cols, x);
                const int off = (int)w1;
                if (off == 0) {
                    if constexpr (W == 4) {
                        const uint4 q = gload4(col, row);
                        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    } else {
                        v[0] = gload1(col, row);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < W; e++) v[e] = gload1(col, neighbour_row(row + e, a.eval_log, a.log_expand, off));
                }
            } else if (op == TSTWO_AIR_OP_CONST) {
#pragma unroll
                for (int e = 0; e < W; e++) v[e] = w1;
            } else if (op == TSTWO_AIR_OP_ACC) {
                lds_read<W>(regs, x, v);
                const u32 k = uni(coeff_base + 4 * n_acc);
                const u32 q0 = prog[k], q1 = prog[k + 1], q2 = prog[k + 2], q3 = prog[k + 3];
#pragma unroll
                for (int e = 0; e < W; e++) {
                    acc[e][0] += (u64)q0 * v[e];
                    acc[e][1] += (u64)q1 * v[e];
                    acc[e][2] += (u64)q2 * v[e];
                    acc[e][3] += (u64)q3 * v[e];
                }
                if ((++n_acc & 3) == 0) {
#pragma unroll
                    for (int e = 0; e < W; e++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[e][j] = fold64(acc[e][j]);
                }
                continue;
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
            lds_write<W>(regs, dst, v);
        }
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
            if constexpr (W == 4) {
                const uint4 o = gload4(a.acc.p[j], row);
                gstore4(a.acc.p[j], row, make_uint4(m31_add(o.x, r[j][0]), m31_add(o.y, r[j][1]), m31_add(o.z, r[j][2]), m31_add(o.w, r[j][3])));
            } else {
                gstore1(a.acc.p[j], row, m31_add(gload1(a.acc.p[j], row), r[j][0]));
            }
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int bad(const char *msg) { return set_error(TSTWO_ERR_BAD_ARG, msg); }

}  // namespace

extern "C" {

int tstwo_air_eval_program(const u32 *const *cols, size_t n_cols, u32 trace_log_size, u32 log_expand, const u32 *program,
                           size_t program_len, const u32 *coeffs, size_t n_constraints, const u32 *denom_inv, u32 *const accum[4]) {
    TSTWO_REQUIRE_READY();
    if (log_expand < 1) return bad("air program: log_expand must be at least 1 (the neighbour index needs eval > trace)");
    if (log_expand > kMaxLogExpand) return bad("air program: log_expand too large");
    if (trace_log_size + log_expand > kMaxLog) return bad("air program: evaluation domain too large");
    if (n_cols == 0 || n_cols > TSTWO_AIR_PROGRAM_MAX_COLS) return bad("air program: number of columns out of range");
    if (program_len == 0 || program_len > TSTWO_AIR_PROGRAM_MAX_INSTR) return bad("air program: program length out of range");
    if (n_constraints == 0 || n_constraints > TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS) return bad("air program: number of constraints out of range");
    if (!program || !coeffs || !denom_inv) return bad("null host argument");
    TSTWO_REQUIRE_TABLE(cols, n_cols);
    TSTWO_REQUIRE_TABLE(accum, 4);
    // the program and coefficient words travel through the small-upload ring, which a captured graph cannot replay
    {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx().stream, &st) != hipSuccess) (void)hipGetLastError();
        else if (st != hipStreamCaptureStatusNone)
            return bad("host-array upload during graph capture (the air program and its coefficients cannot be recorded)");
    }
    // validate every instruction: opcodes, registers (each read one written before), columns, offsets, constants; count ACCs
    bool written[TSTWO_AIR_PROGRAM_MAX_REGS] = {};
    u32 n_regs = 0;
    size_t n_acc = 0;
    auto reg_ok = [&](u32 reg) { return reg < TSTWO_AIR_PROGRAM_MAX_REGS && written[reg]; };
    for (size_t pc = 0; pc < program_len; pc++) {
        const u32 w0 = program[2 * pc], w1 = program[2 * pc + 1];
        const u32 op = w0 & 0xffu, dst = (w0 >> 8) & 0xffu, x = w0 >> 16;
        switch (op) {
            case TSTWO_AIR_OP_LOAD: {
                if (x >= n_cols) return bad("air program: column out of range");
                const int off = (int)w1;
                if (off > TSTWO_AIR_PROGRAM_MAX_OFFSET || off < -TSTWO_AIR_PROGRAM_MAX_OFFSET) return bad("air program: row offset beyond the limit");
                break;
            }
            case TSTWO_AIR_OP_CONST:
                if (w1 >= M31_P) return bad("air program: constant out of range");
                break;
            case TSTWO_AIR_OP_ADD: case TSTWO_AIR_OP_SUB: case TSTWO_AIR_OP_MUL:
                if (!reg_ok(x) || !reg_ok(w1)) return bad("air program: register out of range or read before written");
                break;
            case TSTWO_AIR_OP_SQR: case TSTWO_AIR_OP_NEG:
                if (!reg_ok(x)) return bad("air program: register out of range or read before written");
                break;
            case TSTWO_AIR_OP_ACC:
                if (!reg_ok(x)) return bad("air program: register out of range or read before written");
                n_acc++;
                continue;                   // writes no register
            default:
                return bad("air program: bad opcode");
        }
        if (dst >= TSTWO_AIR_PROGRAM_MAX_REGS) return bad("air program: register out of range or read before written");
        written[dst] = true;
        if (dst + 1 > n_regs) n_regs = dst + 1;
    }
    if (n_acc != n_constraints) return bad("air program: the number of ACC instructions differs from n_constraints");
    for (size_t i = 0; i < 4 * n_constraints; i++)
        if (coeffs[i] >= M31_P) return bad("coefficient word out of range");
    ProgArgs a = {};
    a.n_denoms = 1u << log_expand;
    for (u32 i = 0; i < a.n_denoms; i++) {
        if (denom_inv[i] >= M31_P) return bad("denominator out of range");
        a.denom_inv[i] = denom_inv[i];
    }
    // upload: program words, then coefficient words (at most 16 KiB: one slot of the ring, no host synchronisation)
    const size_t prog_words = 2 * program_len, words = prog_words + 4 * n_constraints;
    static_assert((2 * TSTWO_AIR_PROGRAM_MAX_INSTR + 4 * TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS) * 4 <= kUpSlotBytes, "program upload exceeds one ring slot");
    if (int rc = ensure_scratch(words * sizeof(u32))) return rc;
    u32 staged[2 * TSTWO_AIR_PROGRAM_MAX_INSTR + 4 * TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS];
    std::copy(program, program + prog_words, staged);
    std::copy(coeffs, coeffs + 4 * n_constraints, staged + prog_words);
    if (int rc = small_h2d(ctx().scratch, staged, words * sizeof(u32))) return rc;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    for (int j = 0; j < 4; j++) a.acc.p[j] = accum[j];
    a.prog = ctx().scratch;
    a.n_instr = (u32)program_len;
    a.trace_log = trace_log_size;
    a.eval_log = trace_log_size + log_expand;
    a.log_expand = log_expand;
    a.n_rows = 1u << a.eval_log;
    bool vec = a.n_rows % 4 == 0;
    for (size_t i = 0; i < n_cols && vec; i++) vec = aligned16(cols[i]);
    for (int j = 0; j < 4; j++) vec = vec && aligned16(accum[j]);
    const int W = vec ? 4 : 1;
    const size_t lds = (size_t)(n_regs ? n_regs : 1) * kWave * W * sizeof(u32);
    const size_t work = a.n_rows / W;
    unsigned grid = ceil_div(work, kWave);
    const unsigned cap = (unsigned)ctx().n_cus * 32;
    if (grid > cap) grid = cap;
    if (vec) hipLaunchKernelGGL(k_air_program<4>, dim3(grid), dim3(kWave), lds, ctx().stream, cp, a);
    else hipLaunchKernelGGL(k_air_program<1>, dim3(grid), dim3(kWave), lds, ctx().stream, cp, a);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // extern "C"

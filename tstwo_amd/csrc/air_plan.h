// air_plan.h — how the seven entries of air.hip launch for an input (host only: no HIP, no context): the range checks of their
// arguments, the rows per lane, the grid, the LDS and what is uploaded.  air.hip checks its pointers, asks here and launches what
// the plan says.  tests/air_plan.py restates this in Python; tests/test_cpu_air_plan.py compiles this header and compares.
//
// Two launch shapes:
//   wide         (the hand-written kernels and the compiled ones) workgroups of 256 lanes, at most 16 per CU, never fewer than one;
//                the compiled kernels take stride = grid * 256 as an argument, the hand-written ones read gridDim.
//   interpreter  (k_air_program, k_air_columns, k_air_check) one-wave workgroups, at most 32 per CU, with a register file in LDS:
//                max(n_regs, 1) x 64 lanes x W words; the check keeps its (count, first row) pair per constraint behind it.
// Lanes stride over what the grid does not cover.  W = 4 rows per lane when the caller found every pointer 16-byte aligned
// (`aligned`: air.hip has the pointers) and the rows split into fours, else W = 1.
// The upload goes through the scratch block: the program (2 words per instruction), then the coefficients (4 words per constraint).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/tstwo_hip.h"

namespace tstwo {

constexpr uint32_t kAirMaxLog = 28;                   // word offsets of gload*/gstore* stay below 2^30
constexpr uint32_t kAirMaxLogExpand = 4;
constexpr uint32_t kAirMaxConstraints = 128;          // hand-written kinds: 4 x 128 coefficient words in the kernel argument
constexpr uint32_t kAirWideThreads = 256, kAirWideCapPerCu = 16;
constexpr uint32_t kAirWaveThreads = 64, kAirWaveCapPerCu = 32;
constexpr size_t kAirTableByValue = 64;               // common.h: kMaxColsPerLaunch, the pointers a table carries in the kernel argument
constexpr size_t kAirMaxUploadWords = 2 * TSTWO_AIR_PROGRAM_MAX_INSTR + 4 * TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS;

enum AirEntry : uint32_t {
    kAirWideFibTrace,           // tstwo_air_wide_fib_trace
    kAirQuotients,              // tstwo_air_constraint_quotients
    kAirEvalProgram,            // tstwo_air_eval_program
    kAirEvalCompiled,           // tstwo_air_eval_compiled
    kAirEvalColumns,            // tstwo_air_eval_columns
    kAirEvalColumnsCompiled,    // tstwo_air_eval_columns_compiled
    kAirCheck,                  // tstwo_air_check_constraints
    kAirEntries
};

struct AirInput {
    AirEntry entry;
    uint32_t kind;              // kAirQuotients: TSTWO_AIR_WIDE_FIB or TSTWO_AIR_MUL_ADD
    uint32_t log;               // of the rows the kernel walks: trace_log_size + log_expand, or log_size
    uint32_t log_expand;        // the three entries on an evaluation domain
    size_t n_cols;
    size_t n_terminal;          // constraints, or output columns (kAirEvalColumns*)
    size_t program_len;         // the interpreter entries
    uint32_t n_regs;            // the interpreter entries, from the program validator (air_codegen.h)
    bool aligned;               // every column, accumulator and output of the call is 16-byte aligned
    uint32_t n_cus;
};

struct AirPlan {
    uint32_t w;                 // rows per lane: 4 or 1
    uint32_t threads, grid;
    uint32_t stride;            // the compiled entries: grid * threads, a kernel argument; else 0
    uint32_t lds_bytes;
    uint32_t tally_word;        // kAirCheck: the word offset of the (count, first row) pairs in LDS
    uint32_t upload_words;      // into the scratch block
    uint32_t coeff_word;        // the word offset of the coefficients inside the upload
    bool cols_by_value, out_by_value;       // the pointer tables: in the kernel argument, or through the table in device memory
    bool capturable;            // nothing is uploaded and every table travels by value
};

// What each entry's error texts begin with.
inline const char *air_prefix(AirEntry e) {
    switch (e) {
        case kAirEvalProgram: case kAirEvalCompiled: return "air program: ";
        case kAirEvalColumns: case kAirEvalColumnsCompiled: return "air columns: ";
        case kAirCheck: return "air check: ";
        default: return "";
    }
}

// The range checks, in the order the entries have always made them: the reason behind air_prefix, or nullptr.  It needs no n_regs,
// so that the interpreter entries can ask before they touch the program.
inline const char *air_refuse(const AirInput &in) {
    const bool cols_ok = in.n_cols != 0 && in.n_cols <= TSTWO_AIR_PROGRAM_MAX_COLS;
    const bool constraints_ok = in.n_terminal != 0 && in.n_terminal <= TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS;
    const bool program_ok = in.program_len != 0 && in.program_len <= TSTWO_AIR_PROGRAM_MAX_INSTR;
    switch (in.entry) {
        case kAirWideFibTrace:
            if (in.n_cols < 2) return "wide Fibonacci needs at least 2 columns";
            if (in.log > kAirMaxLog) return "trace too large";
            return nullptr;
        case kAirQuotients:
            if (in.kind == TSTWO_AIR_WIDE_FIB) {
                if (in.n_cols < 3 || in.n_terminal != in.n_cols - 2) return "wide Fibonacci: N >= 3 columns, N - 2 constraints";
            } else if (in.kind == TSTWO_AIR_MUL_ADD) {
                if (in.n_cols != 3 || in.n_terminal != 1) return "mul-add: 3 columns, 1 constraint";
            } else {
                return "unknown constraint kind";
            }
            if (in.n_terminal > kAirMaxConstraints) return "too many constraints in one component";
            if (in.log_expand > kAirMaxLogExpand) return "log_expand too large";
            if (in.log > kAirMaxLog) return "evaluation domain too large";
            return nullptr;
        case kAirEvalProgram: case kAirEvalCompiled:
            if (in.entry == kAirEvalProgram && !program_ok) return "program length out of range";
            if (in.log_expand < 1) return "log_expand must be at least 1 (the neighbour index needs eval > trace)";
            if (in.log_expand > kAirMaxLogExpand) return "log_expand too large";
            if (in.log > kAirMaxLog) return "evaluation domain too large";
            if (!cols_ok) return "number of columns out of range";
            if (!constraints_ok) return "number of constraints out of range";
            return nullptr;
        case kAirEvalColumns: case kAirEvalColumnsCompiled:
            if (in.log < 1 || in.log > kAirMaxLog) return "log_size out of range";
            if (!cols_ok) return "number of columns out of range";
            if (in.n_terminal == 0 || in.n_terminal > TSTWO_AIR_COLUMNS_MAX_OUT) return "number of outputs out of range";
            if (in.entry == kAirEvalColumns && !program_ok) return "program length out of range";
            return nullptr;
        case kAirCheck:
            if (in.log < 1 || in.log > kAirMaxLog) return "log_size out of range";
            if (!cols_ok) return "number of columns out of range";
            if (!constraints_ok) return "number of constraints out of range";
            if (!program_ok) return "program length out of range";
            return nullptr;
        default:
            return "unknown entry";
    }
}

// The plan of an input that air_refuse accepts.
inline AirPlan air_plan(const AirInput &in) {
    AirPlan p = {};
    const uint32_t rows = 1u << in.log;
    p.w = in.aligned && rows % 4 == 0 ? 4 : 1;
    const uint32_t lanes = rows / p.w;
    const bool interpreter = in.entry == kAirEvalProgram || in.entry == kAirEvalColumns || in.entry == kAirCheck;
    p.threads = interpreter ? kAirWaveThreads : kAirWideThreads;
    const uint32_t cap = in.n_cus * (interpreter ? kAirWaveCapPerCu : kAirWideCapPerCu);
    const uint32_t all = (lanes + p.threads - 1) / p.threads;
    p.grid = all <= cap ? all : cap ? cap : 1;
    if (in.entry == kAirEvalCompiled || in.entry == kAirEvalColumnsCompiled) p.stride = p.grid * p.threads;
    if (interpreter) {
        p.lds_bytes = (in.n_regs ? in.n_regs : 1) * kAirWaveThreads * p.w * 4;
        p.upload_words = 2 * (uint32_t)in.program_len;
    }
    if (in.entry == kAirCheck) {
        p.tally_word = p.lds_bytes / 4;
        p.lds_bytes += 2 * (uint32_t)in.n_terminal * 4;
    }
    if (in.entry == kAirEvalProgram || in.entry == kAirEvalCompiled) {
        p.coeff_word = p.upload_words;
        p.upload_words += 4 * (uint32_t)in.n_terminal;
    }
    p.cols_by_value = in.n_cols <= kAirTableByValue;
    p.out_by_value = true;                  // at most TSTWO_AIR_COLUMNS_MAX_OUT outputs; the other entries have no second table
    p.capturable = p.upload_words == 0 && p.cols_by_value && p.out_by_value;
    return p;
}
static_assert(TSTWO_AIR_COLUMNS_MAX_OUT <= kAirTableByValue, "the output table travels by value");

}  // namespace tstwo

// air_codegen.h — a constraint program (the words of tstwo_air_eval_program) as HIP source text (host only: no HIP, no context).
// check_program validates the programs of every entry (tstwo_air_eval_program, tstwo_air_eval_columns,
// tstwo_air_check_constraints, tstwo_air_program_compile, tstwo_air_columns_compile); air_codegen writes, for one program, two extern "C" kernels with the contract of k_air_program
// (air.hip): for every row r, accum[r] += (sum_k coeff_k e_k(r)) * denom_inv[r >> trace_log].  tests/test_cpu_air_codegen.py
// builds tests/air_codegen_main.cpp around this header alone.
//
// The text: air_native_prelude() (the device helpers, csrc/air_native_prelude.inc), then one function template over W, the rows
// per lane, and the kernels air_native_w4 / air_native_w1 that instantiate it.  Every instruction is one statement that defines
// a fresh local `t<pc>` (an ISA register written again gets a new name: the text is in SSA form, there is no register file),
// loads at offset 0 are the 16-byte row load, loads at another offset gather through the rows `n_p<k>` / `n_m<k>`, computed once
// per distinct offset; column and coefficient indices are constants of the text.  The accumulators fold after every fourth ACC
// and reduce once per row, as the interpreter's.  trace_log, log_expand and n_rows are kernel arguments: one text serves every
// domain size.  The same words give the same text.
//
// air_columns_codegen is the twin for the STORE programs of tstwo_air_eval_columns (check_store_program validates them for the
// interpreter entry and for the generator): the same statements, neighbours on the TRACE domain, `STORE k` as one store_rows
// to output column k, kernels air_columns_w4 / air_columns_w1 with the contract of k_air_columns.  Its device helpers
// (csrc/air_native_columns_prelude.inc) follow the prelude in column texts only: the text of an ACC program does not change.
#pragma once
#include <cstddef>
#include <cstdint>
#include <set>
#include <string>

#include "../../include/tstwo_hip.h"

namespace tstwo {

// Validates every instruction of a straight-line program: opcodes, registers (each read one written before), columns, offsets,
// constants.  `terminal` is the entry's own opcode that reads r[x] and writes no register (ACC or STORE; the other one is a bad
// opcode); on_terminal(w1) checks and counts it.  n_regs: the highest register written + 1.  Returns the reason (the entry puts
// its prefix in front) or nullptr.
template <class F>
const char *check_program(const uint32_t *program, size_t program_len, size_t n_cols, uint32_t terminal, uint32_t &n_regs, F on_terminal) {
    bool written[TSTWO_AIR_PROGRAM_MAX_REGS] = {};
    n_regs = 0;
    auto reg_ok = [&](uint32_t reg) { return reg < TSTWO_AIR_PROGRAM_MAX_REGS && written[reg]; };
    for (size_t pc = 0; pc < program_len; pc++) {
        const uint32_t w0 = program[2 * pc], w1 = program[2 * pc + 1];
        const uint32_t op = w0 & 0xffu, dst = (w0 >> 8) & 0xffu, x = w0 >> 16;
        switch (op) {
            case TSTWO_AIR_OP_LOAD: {
                if (x >= n_cols) return "column out of range";
                const int off = (int)w1;
                if (off > TSTWO_AIR_PROGRAM_MAX_OFFSET || off < -TSTWO_AIR_PROGRAM_MAX_OFFSET) return "row offset beyond the limit";
                break;
            }
            case TSTWO_AIR_OP_CONST:
                if (w1 >= 2147483647u) return "constant out of range";
                break;
            case TSTWO_AIR_OP_ADD: case TSTWO_AIR_OP_SUB: case TSTWO_AIR_OP_MUL:
                if (!reg_ok(x) || !reg_ok(w1)) return "register out of range or read before written";
                break;
            case TSTWO_AIR_OP_SQR: case TSTWO_AIR_OP_NEG:
                if (!reg_ok(x)) return "register out of range or read before written";
                break;
            case TSTWO_AIR_OP_ACC: case TSTWO_AIR_OP_STORE:
                if (op != terminal) return "bad opcode";
                if (!reg_ok(x)) return "register out of range or read before written";
                if (const char *why = on_terminal(w1)) return why;
                continue;                   // writes no register
            default:
                return "bad opcode";
        }
        if (dst >= TSTWO_AIR_PROGRAM_MAX_REGS) return "register out of range or read before written";
        written[dst] = true;
        if (dst + 1 > n_regs) n_regs = dst + 1;
    }
    return nullptr;
}

// What tstwo_air_eval_program and tstwo_air_program_compile accept: the limits, every instruction, one ACC per constraint.
inline const char *check_acc_program(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_constraints, uint32_t &n_regs) {
    if (n_cols == 0 || n_cols > TSTWO_AIR_PROGRAM_MAX_COLS) return "number of columns out of range";
    if (program_len == 0 || program_len > TSTWO_AIR_PROGRAM_MAX_INSTR) return "program length out of range";
    if (n_constraints == 0 || n_constraints > TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS) return "number of constraints out of range";
    size_t n_acc = 0;
    if (const char *why = check_program(program, program_len, n_cols, TSTWO_AIR_OP_ACC, n_regs, [&](uint32_t) { n_acc++; return (const char *)nullptr; }))
        return why;
    if (n_acc != n_constraints) return "the number of ACC instructions differs from n_constraints";
    return nullptr;
}

// What tstwo_air_check_constraints accepts: an ACC program whose ACCs carry, in w1, the index of the constraint they belong to
// (a secure constraint is four ACCs with one index).  The indices start at 0, never decrease, rise by at most 1 from one ACC to
// the next and end at n_constraints - 1; the number of ACCs is free.
inline const char *check_assert_program(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_constraints, uint32_t &n_regs) {
    if (n_cols == 0 || n_cols > TSTWO_AIR_PROGRAM_MAX_COLS) return "number of columns out of range";
    if (program_len == 0 || program_len > TSTWO_AIR_PROGRAM_MAX_INSTR) return "program length out of range";
    if (n_constraints == 0 || n_constraints > TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS) return "number of constraints out of range";
    size_t n_acc = 0;
    uint32_t last = 0;
    auto on_acc = [&](uint32_t c) -> const char * {
        if (n_acc == 0 && c != 0) return "first constraint index is not 0";
        if (c < last) return "constraint index decreases";
        if (c > last + 1) return "constraint index skips";
        if (c >= n_constraints) return "constraint index out of range";
        last = c;
        n_acc++;
        return (const char *)nullptr;
    };
    if (const char *why = check_program(program, program_len, n_cols, TSTWO_AIR_OP_ACC, n_regs, on_acc)) return why;
    if (n_acc == 0 || last != n_constraints - 1) return "last constraint index is not n_constraints - 1";
    return nullptr;
}

// The copy of a program check_assert_program accepted that tstwo_air_check_constraints uploads: dst (ignored by every other entry)
// is cleared in every ACC and set to 1 in the last ACC of every constraint index, where k_air_check votes.
inline void mark_last_acc(const uint32_t *program, size_t program_len, uint32_t *marked) {
    uint32_t *last_acc = nullptr;
    for (size_t pc = 0; pc < program_len; pc++) {
        uint32_t *w = marked + 2 * pc;
        w[0] = program[2 * pc], w[1] = program[2 * pc + 1];
        if ((w[0] & 0xffu) != TSTWO_AIR_OP_ACC) continue;
        w[0] &= ~0xff00u;
        if (last_acc && last_acc[1] != w[1]) last_acc[0] |= 1u << 8;
        last_acc = w;
    }
    if (last_acc) last_acc[0] |= 1u << 8;       // check_assert_program saw at least one ACC
}

// What tstwo_air_eval_columns and tstwo_air_columns_compile accept: the limits, every instruction, every output stored once.
inline const char *check_store_program(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_out, uint32_t &n_regs) {
    if (n_cols == 0 || n_cols > TSTWO_AIR_PROGRAM_MAX_COLS) return "number of columns out of range";
    if (n_out == 0 || n_out > TSTWO_AIR_COLUMNS_MAX_OUT) return "number of outputs out of range";
    if (program_len == 0 || program_len > TSTWO_AIR_PROGRAM_MAX_INSTR) return "program length out of range";
    bool stored[TSTWO_AIR_COLUMNS_MAX_OUT] = {};
    size_t n_stored = 0;
    auto on_store = [&](uint32_t k) -> const char * {
        if (k >= n_out) return "output index out of range";
        if (stored[k]) return "output stored twice";
        stored[k] = true;
        n_stored++;
        return (const char *)nullptr;
    };
    if (const char *why = check_program(program, program_len, n_cols, TSTWO_AIR_OP_STORE, n_regs, on_store)) return why;
    if (n_stored != n_out) return "an output is never stored";
    return nullptr;
}

inline const char *air_native_prelude() {
    static const char text[] =
#include "air_native_prelude.inc"
        ;
    return text;
}

// The helpers of column texts alone, behind air_native_prelude().
inline const char *air_native_columns_prelude() {
    static const char text[] =
#include "air_native_columns_prelude.inc"
        ;
    return text;
}

// The kernels of a compiled program, and what hipRTC is given besides --offload-arch=<the device's architecture>.
constexpr const char *kAirNativeKernelW4 = "air_native_w4";
constexpr const char *kAirNativeKernelW1 = "air_native_w1";
constexpr const char *kAirColumnsKernelW4 = "air_columns_w4";
constexpr const char *kAirColumnsKernelW1 = "air_columns_w1";
constexpr int kAirNativeThreads = 256;
constexpr const char *kAirNativeOptions[] = {"-O3", "-std=c++17"};

// An unsigned entry of a kernel's metadata in a code object (the msgpack note AMDGPU code objects carry: per kernel a map with
// sorted keys, ".name" before ".sgpr_count" / ".vgpr_count" / ".private_segment_fixed_size"): the value behind the first `key`
// that follows `.name = kernel`.  The HIP runtime reports registers and private bytes of a loaded function, but not its SGPRs.
// Returns false when the text is not there.
inline bool code_object_uint(const char *code, size_t size, const char *kernel, const char *key, uint32_t &value) {
    auto str = [](const std::string &s) { return (s.size() < 32 ? std::string(1, (char)(0xa0 | s.size())) : std::string("\xd9") + (char)s.size()) + s; };
    const std::string all(code, size), name = str(".name") + str(kernel), k = str(key);
    size_t at = all.find(name);
    if (at == std::string::npos || (at = all.find(k, at + name.size())) == std::string::npos) return false;
    const unsigned char *p = (const unsigned char *)code + at + k.size(), *end = (const unsigned char *)code + size;
    if (p >= end) return false;
    const int n = *p < 0x80 ? 0 : *p == 0xcc ? 1 : *p == 0xcd ? 2 : *p == 0xce ? 4 : -1;
    if (n < 0 || p + n >= end) return false;
    value = n ? 0 : *p;
    for (int i = 1; i <= n; i++) value = value << 8 | p[i];           // big-endian
    return true;
}

// The statements of a validated program, for the loop body of either generator: one `const V n_p<k> / n_m<k> = <neighbour(off)>;`
// per distinct non-zero offset (ordered: the text does not depend on where an offset first occurs), then one statement per
// instruction; terminal(reg name, w1) writes the statement(s) of the entry's own ACC or STORE.
template <class N, class T>
std::string program_statements(const uint32_t *program, size_t program_len, N neighbour, T terminal) {
    auto num = [](uint64_t v) { return std::to_string(v); };
    auto nb_name = [&](int off) { return std::string(off < 0 ? "n_m" : "n_p") + num((uint64_t)(off < 0 ? -off : off)); };
    std::set<int> offsets;
    for (size_t pc = 0; pc < program_len; pc++)
        if ((program[2 * pc] & 0xffu) == TSTWO_AIR_OP_LOAD && program[2 * pc + 1] != 0) offsets.insert((int)program[2 * pc + 1]);
    std::string body;
    for (int off : offsets) body += "        const V " + nb_name(off) + " = " + neighbour(std::to_string(off)) + ";\n";
    size_t name_of[TSTWO_AIR_PROGRAM_MAX_REGS] = {};     // the instruction whose result the register holds
    for (size_t pc = 0; pc < program_len; pc++) {
        const uint32_t w0 = program[2 * pc], w1 = program[2 * pc + 1];
        const uint32_t op = w0 & 0xffu, dst = (w0 >> 8) & 0xffu, x = w0 >> 16;
        auto reg = [&](uint32_t r) { return "t" + num(name_of[r]); };
        std::string rhs;
        switch (op) {
            case TSTWO_AIR_OP_ACC: case TSTWO_AIR_OP_STORE:
                body += terminal(reg(x), w1);
                continue;
            case TSTWO_AIR_OP_LOAD:
                if (w1 == 0) rhs = "load_rows<W>(col_at(tab, " + num(x) + "), row)";
                else rhs = "load_at<W>(col_at(tab, " + num(x) + "), " + nb_name((int)w1) + ")";
                break;
            case TSTWO_AIR_OP_CONST: rhs = "r_const<W>(" + num(w1) + "u)"; break;
            case TSTWO_AIR_OP_ADD: rhs = "r_add<W>(" + reg(x) + ", " + reg(w1) + ")"; break;
            case TSTWO_AIR_OP_SUB: rhs = "r_sub<W>(" + reg(x) + ", " + reg(w1) + ")"; break;
            case TSTWO_AIR_OP_MUL: rhs = "r_mul<W>(" + reg(x) + ", " + reg(w1) + ")"; break;
            case TSTWO_AIR_OP_SQR: rhs = "r_sqr<W>(" + reg(x) + ")"; break;
            default: rhs = "r_neg<W>(" + reg(x) + ")"; break;           // TSTWO_AIR_OP_NEG: check_program let nothing else through
        }
        body += "        const V t" + num(pc) + " = " + rhs + ";\n";
        name_of[dst] = pc;
    }
    return body;
}

// The source text of a program's two kernels into `out`.  Returns the reason (the texts of tstwo_air_eval_program, without
// its prefix) and leaves `out` empty for a program the interpreter would refuse.
inline const char *air_codegen(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_constraints, std::string &out) {
    out.clear();
    uint32_t n_regs = 0;
    if (const char *why = check_acc_program(program, program_len, n_cols, n_constraints, n_regs)) return why;
    auto num = [](uint64_t v) { return std::to_string(v); };
    size_t n_acc = 0;
    const std::string body = program_statements(
        program, program_len, [](const std::string &off) { return "neighbour_rows<W>(row, a.eval_log, a.log_expand, " + off + ")"; },
        [&](const std::string &reg, uint32_t) {
            const std::string k = num(4 * n_acc);
            std::string st = "        accumulate<W>(acc, " + reg + ", coeff[" + k + "], coeff[" + k + " + 1], coeff[" + k + " + 2], coeff[" + k + " + 3]);\n";
            if ((++n_acc & 3) == 0) st += "        fold_all<W>(acc);\n";
            return st;
        });
    const std::string threads = num(kAirNativeThreads);
    out = air_native_prelude();
    out += "\n// " + num(program_len) + " instructions, " + num(n_cols) + " columns, " + num(n_constraints) + " constraints\n"
           "template <int W>\n"
           "AIRN_DEV void air_native_rows(const airn::ColPtrs &cols, const airn::NativeArgs &a) {\n"
           "    using namespace airn;\n"
           "    typedef Rows<W> V;\n"
           "    const k64 tab = col_table(cols);\n"
           "    const k32 coeff = (k32)a.coeff;\n"
           "    for (u32 t = __builtin_amdgcn_workgroup_id_x() * " + threads + "u + __builtin_amdgcn_workitem_id_x(); t < a.n_rows / W; t += a.stride) {\n"
           "        const u32 row = t * W;\n"
           "        u64 acc[W][4] = {};\n";
    out += body;
    out += "        AIRN_ADD_ROWS(W, a, row, acc);\n"
           "    }\n"
           "}\n";
    for (int w : {4, 1})
        out += "extern \"C\" __global__ void __attribute__((amdgpu_flat_work_group_size(1, " + threads + "))) " + (w == 4 ? kAirNativeKernelW4 : kAirNativeKernelW1) +
               "(airn::ColPtrs cols, airn::NativeArgs a) { air_native_rows<" + num((uint64_t)w) + ">(cols, a); }\n";
    return nullptr;
}

// The same for a STORE program: the text of air_columns_w4 / air_columns_w1, which write n_out output columns on the trace domain
// (k_air_columns).  Returns the reason (the texts of tstwo_air_eval_columns, without its prefix) and leaves `out` empty for a
// program the interpreter would refuse.
inline const char *air_columns_codegen(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_out, std::string &out) {
    out.clear();
    uint32_t n_regs = 0;
    if (const char *why = check_store_program(program, program_len, n_cols, n_out, n_regs)) return why;
    auto num = [](uint64_t v) { return std::to_string(v); };
    const std::string body = program_statements(
        program, program_len, [](const std::string &off) { return "trace_neighbour_rows<W>(row, a.log, " + off + ")"; },
        [&](const std::string &reg, uint32_t k) { return "        store_rows<W>(out_at(otab, " + num(k) + "), row, " + reg + ");\n"; });
    const std::string threads = num(kAirNativeThreads);
    out = air_native_prelude();
    out += air_native_columns_prelude();
    out += "\n// " + num(program_len) + " instructions, " + num(n_cols) + " columns, " + num(n_out) + " outputs\n"
           "template <int W>\n"
           "AIRN_DEV void air_columns_rows(const airn::ColPtrs &cols, const airn::ColPtrs &out, const airn::ColumnsArgs &a) {\n"
           "    using namespace airn;\n"
           "    typedef Rows<W> V;\n"
           "    const k64 tab = col_table(cols);\n"
           "    const k64 otab = out_table(out);\n"
           "    for (u32 t = __builtin_amdgcn_workgroup_id_x() * " + threads + "u + __builtin_amdgcn_workitem_id_x(); t < a.n_rows / W; t += a.stride) {\n"
           "        const u32 row = t * W;\n";
    out += body;
    out += "    }\n"
           "}\n";
    for (int w : {4, 1})
        out += "extern \"C\" __global__ void __attribute__((amdgpu_flat_work_group_size(1, " + threads + "))) " + (w == 4 ? kAirColumnsKernelW4 : kAirColumnsKernelW1) +
               "(airn::ColPtrs cols, airn::ColPtrs out, airn::ColumnsArgs a) { air_columns_rows<" + num((uint64_t)w) + ">(cols, out, a); }\n";
    return nullptr;
}

}  // namespace tstwo

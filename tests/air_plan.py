"""The launch plan of the seven AIR entries restated in Python (csrc/air_plan.h is the statement the library runs;
tests/test_cpu_air_plan.py compiles that header and compares), the marker of the check program (csrc/air_codegen.h
mark_last_acc), the branches a plan reaches, the smallest size at which a kernel's lanes stride, and the shapes the -m gpu AIR
files run.  Plain Python: nothing here touches a GPU or imports the package under test."""
from __future__ import annotations

from collections import namedtuple

ENTRIES = ("wide_fib_trace", "quotients", "eval_program", "eval_compiled", "eval_columns", "eval_columns_compiled", "check")
INTERPRETED = ("eval_program", "eval_columns", "check")         # one-wave workgroups, a register file in LDS, the program uploaded
COMPILED = ("eval_compiled", "eval_columns_compiled")           # the stride is a kernel argument
ON_EVAL_DOMAIN = ("quotients", "eval_program", "eval_compiled")
PREFIX = {"eval_program": "air program: ", "eval_compiled": "air program: ", "eval_columns": "air columns: ",
          "eval_columns_compiled": "air columns: ", "check": "air check: "}
WIDE_FIB, MUL_ADD = 0, 1

MAX_LOG, MAX_LOG_EXPAND, MAX_HAND_CONSTRAINTS = 28, 4, 128
MAX_COLS, MAX_CONSTRAINTS, MAX_OUT, MAX_INSTR, MAX_REGS = 4096, 256, 64, 1536, 32
WIDE_THREADS, WIDE_CAP_PER_CU = 256, 16
WAVE_THREADS, WAVE_CAP_PER_CU = 64, 32
TABLE_BY_VALUE = 64
MAX_GPU_ROWS = 1 << 23          # no GPU test walks more rows than this in one call
OP_ACC = 7

Input = namedtuple("Input", "entry kind log log_expand n_cols n_terminal program_len n_regs aligned n_cus")
Plan = namedtuple("Plan", "w threads grid stride lds_bytes tally_word upload_words coeff_word cols_by_value out_by_value capturable")


class PlanError(ValueError):
    pass


def refuse(i: Input):
    """The reason behind the entry's prefix, or None: the range checks in the order the entries make them."""
    cols_ok = 0 < i.n_cols <= MAX_COLS
    constraints_ok = 0 < i.n_terminal <= MAX_CONSTRAINTS
    program_ok = 0 < i.program_len <= MAX_INSTR
    if i.entry == "wide_fib_trace":
        if i.n_cols < 2:
            return "wide Fibonacci needs at least 2 columns"
        return "trace too large" if i.log > MAX_LOG else None
    if i.entry == "quotients":
        if i.kind == WIDE_FIB:
            if i.n_cols < 3 or i.n_terminal != i.n_cols - 2:
                return "wide Fibonacci: N >= 3 columns, N - 2 constraints"
        elif i.kind == MUL_ADD:
            if i.n_cols != 3 or i.n_terminal != 1:
                return "mul-add: 3 columns, 1 constraint"
        else:
            return "unknown constraint kind"
        if i.n_terminal > MAX_HAND_CONSTRAINTS:
            return "too many constraints in one component"
        if i.log_expand > MAX_LOG_EXPAND:
            return "log_expand too large"
        return "evaluation domain too large" if i.log > MAX_LOG else None
    if i.entry in ("eval_program", "eval_compiled"):
        if i.entry == "eval_program" and not program_ok:
            return "program length out of range"
        if i.log_expand < 1:
            return "log_expand must be at least 1 (the neighbour index needs eval > trace)"
        if i.log_expand > MAX_LOG_EXPAND:
            return "log_expand too large"
        if i.log > MAX_LOG:
            return "evaluation domain too large"
        if not cols_ok:
            return "number of columns out of range"
        return None if constraints_ok else "number of constraints out of range"
    if i.entry in ("eval_columns", "eval_columns_compiled"):
        if not 1 <= i.log <= MAX_LOG:
            return "log_size out of range"
        if not cols_ok:
            return "number of columns out of range"
        if not 0 < i.n_terminal <= MAX_OUT:
            return "number of outputs out of range"
        return "program length out of range" if i.entry == "eval_columns" and not program_ok else None
    if i.entry == "check":
        if not 1 <= i.log <= MAX_LOG:
            return "log_size out of range"
        if not cols_ok:
            return "number of columns out of range"
        if not constraints_ok:
            return "number of constraints out of range"
        return None if program_ok else "program length out of range"
    raise KeyError(i.entry)


def plan(i: Input) -> Plan:
    why = refuse(i)
    if why is not None:
        raise PlanError(why)
    rows = 1 << i.log
    w = 4 if i.aligned and rows % 4 == 0 else 1
    interpreted = i.entry in INTERPRETED
    threads = WAVE_THREADS if interpreted else WIDE_THREADS
    cap = i.n_cus * (WAVE_CAP_PER_CU if interpreted else WIDE_CAP_PER_CU)
    grid = max(1, min(-(-(rows // w) // threads), cap))
    stride = grid * threads if i.entry in COMPILED else 0
    lds = tally = upload = coeff = 0
    if interpreted:
        lds = max(i.n_regs, 1) * WAVE_THREADS * w * 4
        upload = 2 * i.program_len
    if i.entry == "check":
        tally = lds // 4
        lds += 8 * i.n_terminal
    if i.entry in ("eval_program", "eval_compiled"):
        coeff = upload
        upload += 4 * i.n_terminal
    by_value = i.n_cols <= TABLE_BY_VALUE
    return Plan(w, threads, grid, stride, lds, tally, upload, coeff, by_value, True, upload == 0 and by_value)


def render(p: Plan) -> str:
    return " ".join(str(int(v)) for v in p)


def line(i: Input) -> str:
    """What tests/air_plan_main.cpp reads for an input."""
    return f"P {ENTRIES.index(i.entry)} {i.kind} {i.log} {i.log_expand} {i.n_cols} {i.n_terminal} {i.program_len} {i.n_regs} {int(i.aligned)} {i.n_cus}"


def strides(i: Input) -> bool:
    p = plan(i)
    return p.grid * p.threads * p.w < 1 << i.log


def first_striding_log(entry: str, w: int, n_cus: int) -> int:
    """The smallest log whose rows the grid does not cover at `w` rows per lane, so that lanes take a second turn.  Found by
    asking the plan, size by size."""
    for log in range(2 if w == 4 else 0, MAX_LOG + 1):
        le = 1 if entry in ON_EVAL_DOMAIN else 0
        i = Input(entry, MUL_ADD, log, le, 3, 1, 1 if entry in INTERPRETED else 0, 1, w == 4, n_cus)
        if refuse(i) is None and strides(i):
            assert plan(i).w == w
            return log
    raise ValueError((entry, w, n_cus))


def branches(i: Input) -> set:
    """What one call reaches: the entry's kernel at its width, wrapping round the grid or not; for W = 1 the cause; where the
    column table travels; for the check, the tally directly behind one register and behind all 32."""
    p = plan(i)
    out = {f"{i.entry}:w{p.w}:{'stride' if strides(i) else 'fit'}", "table:value" if p.cols_by_value else "table:device"}
    if p.w == 1:
        out.add("w1:short" if (1 << i.log) % 4 else "w1:misaligned")
    if i.entry == "check" and i.n_regs in (1, MAX_REGS):
        out.add(f"tally:{i.n_regs}")
    return out


def reachable_branches(n_cus=(64, 256, 304)) -> set:
    out = set()
    for entry in ENTRIES:
        for log in range(MAX_LOG + 1):
            for aligned in (False, True):
                for n_cols in (3, 65):
                    for n_regs in (1, 2, MAX_REGS):
                        for cus in n_cus:
                            le = 1 if entry in ON_EVAL_DOMAIN else 0
                            i = Input(entry, WIDE_FIB, log, le, n_cols, n_cols - 2, 1 if entry in INTERPRETED else 0, n_regs, aligned, cus)
                            if refuse(i) is None:
                                out |= branches(i)
    return out


# ---------------------------------------------------------------- the marker of the check program
def mark_last_acc(words):
    """csrc/air_codegen.h mark_last_acc: dst cleared in every ACC, 1 in the last ACC of every constraint index."""
    out = list(words)
    last = None
    for pc in range(len(out) // 2):
        if out[2 * pc] & 0xff != OP_ACC:
            continue
        out[2 * pc] &= ~0xff00 & 0xffffffff
        if last is not None and out[2 * last + 1] != out[2 * pc + 1]:
            out[2 * last] |= 1 << 8
        last = pc
    if last is not None:
        out[2 * last] |= 1 << 8
    return out


# ---------------------------------------------------------------- the shapes of the -m gpu files
def _shape(entry, log, n_cols, n_terminal, aligned=True, log_expand=None, kind=MUL_ADD, n_regs=8, n_ops=0, n_cus=256):
    """n_regs: 8 stands for "a random program's" where the test does not fix the number; n_ops: the program's other instructions."""
    le = (1 if entry in ON_EVAL_DOMAIN else 0) if log_expand is None else log_expand
    interpreted = entry in INTERPRETED
    return Input(entry, kind, log, le, n_cols, n_terminal, n_ops + n_terminal if interpreted else 0, n_regs if interpreted else 0, aligned, n_cus)


def gpu_shapes(n_cus: int = 256) -> dict:
    """{name: Input}: the calls the -m gpu files make at the seven entries themselves (tests/test_gpu_air*.py and the program
    cases of tests/test_gpu_constraint_framework.py), on a part of n_cus CUs.  The proofs those files also run reach the entries
    through the package at sizes among these."""
    s = {}

    def add(name, *a, **k):
        assert name not in s, name
        s[name] = _shape(*a, n_cus=n_cus, **k)

    # tests/test_gpu_air.py
    for log, n in [(2, 3), (3, 100), (5, 4), (8, 17), (12, 100), (16, 7), (20, 100)]:
        add(f"fib-{log}x{n}", "wide_fib_trace", log, n, 0)
    for kind, n, log, le in [(WIDE_FIB, 3, 2, 1), (WIDE_FIB, 4, 1, 1), (WIDE_FIB, 4, 6, 1), (WIDE_FIB, 17, 11, 1), (WIDE_FIB, 17, 20, 1), (WIDE_FIB, 100, 3, 1),
                             (WIDE_FIB, 100, 14, 1), (WIDE_FIB, 100, 18, 1), (WIDE_FIB, 17, 9, 2), (MUL_ADD, 3, 2, 1), (MUL_ADD, 3, 8, 2), (MUL_ADD, 3, 20, 1)]:
        add(f"quotients-{kind}-{n}x{log}+{le}", "quotients", log + le, n, n - 2 if kind == WIDE_FIB else 1, log_expand=le, kind=kind)
    add("fib-w1-small", "wide_fib_trace", 6, 5, 0, aligned=False)
    add("quotients-w1-small", "quotients", 6, 3, 1, aligned=False)
    for w in (4, 1):        # the grid-stride loops: STRIDE_CASES of tests/test_gpu_air.py
        add(f"fib-stride-w{w}", "wide_fib_trace", first_striding_log("wide_fib_trace", w, n_cus), 2, 0, aligned=w == 4)
        add(f"quotients-stride-w{w}", "quotients", first_striding_log("quotients", w, n_cus), 3, 1, aligned=w == 4)
        add(f"program-stride-w{w}", "eval_program", first_striding_log("eval_program", w, n_cus), 3, 1, aligned=w == 4, n_regs=3, n_ops=5)
    # tests/test_gpu_constraint_framework.py
    for tl in (2, 3, 5, 8, 11, 14, 17, 20):
        for le in (1, 2, 3):
            if tl + le <= 21:
                add(f"program-{tl}+{le}", "eval_program", tl + le, 6, 5, log_expand=le, n_ops=40)
    for tl, le in [(2, 1), (6, 2), (10, 3), (13, 1)]:
        add(f"program-unaligned-{tl}+{le}", "eval_program", tl + le, 5, 3, aligned=False, log_expand=le, n_ops=30)
    add("program-90-columns", "eval_program", 11, 90, 20, log_expand=2, n_ops=300)
    # tests/test_gpu_air_native.py: the compiled kernel, and the interpreter beside it where the grid strides
    for tl, le in [(1, 1), (2, 1), (3, 4), (6, 2), (10, 3)]:
        add(f"compiled-{tl}+{le}", "eval_compiled", tl + le, 6, 5, log_expand=le)
    for tl, le in [(2, 1), (6, 2), (10, 3), (13, 1)]:
        add(f"compiled-unaligned-{tl}+{le}", "eval_compiled", tl + le, 5, 3, aligned=False, log_expand=le)
    add("compiled-two-rows", "eval_compiled", 1, 3, 2, log_expand=1)
    add("compiled-90-columns", "eval_compiled", 11, 90, 7, log_expand=2)
    add("compiled-90-columns-unaligned", "eval_compiled", 6, 90, 7, aligned=False, log_expand=1)
    for aligned in (True, False):
        add(f"compiled-offsets-64-{int(aligned)}", "eval_compiled", 10, 2, 2, aligned=aligned, log_expand=2)
        add(f"compiled-64-constraints-{int(aligned)}", "eval_compiled", 4, 2, 64, aligned=aligned, log_expand=1)
    for w in (4, 1):
        log = first_striding_log("eval_compiled", w, n_cus)
        add(f"compiled-stride-w{w}", "eval_compiled", log, 3, 2, aligned=w == 4, log_expand=2)
        add(f"program-beside-compiled-w{w}", "eval_program", log, 3, 2, aligned=w == 4, log_expand=2, n_regs=5, n_ops=6)
    # tests/test_gpu_air_columns.py and tests/test_gpu_air_columns_native.py: the same shapes at both entries
    for entry, k in (("eval_columns", "columns"), ("eval_columns_compiled", "columns-compiled")):
        for log, n, n_out, n_ops in [(1, 3, 2, 24), (2, 3, 2, 24), (3, 4, 3, 30), (8, 6, 5, 40), (9, 6, 5, 40)]:
            add(f"{k}-{log}", entry, log, n, n_out, n_ops=n_ops)
        add(f"{k}-12-unaligned", entry, 12, 4, 3, aligned=False, n_ops=30)
        for log in (3, 9):
            add(f"{k}-{log}-unaligned", entry, log, 5, 4, aligned=False, n_ops=40)
        add(f"{k}-1-register", entry, 5, 3, 1, n_regs=1, n_ops=12)
        add(f"{k}-32-registers", entry, 5, 6, 4, n_regs=32, n_ops=80)
        add(f"{k}-1-output", entry, 4, 5, 1, n_ops=30)
        add(f"{k}-64-outputs", entry, 4, 5, 64, n_ops=40)
        add(f"{k}-65-columns", entry, 4, 65, 3, n_ops=120)
        add(f"{k}-offsets-64", entry, 9, 2, 2, n_regs=4, n_ops=5)
    add("columns-stride-w4", "eval_columns", first_striding_log("eval_columns", 4, n_cus), 2, 1, n_regs=3, n_ops=6)
    for w in (4, 1):
        log = first_striding_log("eval_columns_compiled", w, n_cus)
        add(f"columns-compiled-stride-w{w}", "eval_columns_compiled", log, 2, 1, aligned=w == 4)
        add(f"columns-beside-compiled-w{w}", "eval_columns", log, 2, 1, aligned=w == 4, n_regs=3, n_ops=6)
    # tests/test_gpu_air_check.py
    for log, n, n_ops, aligned in [(1, 3, 24, True), (2, 3, 24, True), (5, 4, 30, True), (8, 6, 40, True), (9, 6, 40, True), (10, 4, 30, False)]:
        for name, n_constraints in (("one", 8), ("four", 2), ("mixed", 4)):
            add(f"check-{log}-{name}", "check", log, n, n_constraints, aligned=aligned, n_ops=n_ops + 8 - n_constraints)
    for w in (4, 1):
        add(f"check-stride-w{w}", "check", first_striding_log("check", w, n_cus), 3, 1, aligned=w == 4, n_regs=2, n_ops=6)
    add("check-256-constraints", "check", 6, 2, 256, n_regs=3, n_ops=514)
    for n_regs in (1, MAX_REGS):            # REGISTER_CASES of tests/test_gpu_air_check.py: register_program below
        for aligned in (True, False):
            add(f"check-{n_regs}-registers-{int(aligned)}", "check", 5, 3, 2, aligned=aligned, n_regs=n_regs, n_ops=2 * n_regs - 1)
    return s


def register_program(n_regs: int, n_cols: int, terminals, terminal_op: int = OP_ACC):
    """A program that writes exactly registers 0 .. n_regs - 1 and reads every one of them: r0 = the first column one row back,
    r_k = r_(k-1) + column k (mod n_cols) for k < n_regs; terminal t of `terminals` (the w1 of each ACC or STORE) reads register
    n_regs - 1 - (t mod n_regs), so the first reads the sum of them all.  With one register the sum stays in r0."""
    def enc(op, dst, x, w1):
        return [op | dst << 8 | x << 16, w1 & 0xffffffff]
    words = enc(0, 0, 0, -1)
    for k in range(1, n_regs):
        words += enc(0, k, k % n_cols, 0) + enc(2, k, k, k - 1)
    for t, w1 in enumerate(terminals):
        words += enc(terminal_op, 0, n_regs - 1 - t % n_regs, w1)
    return words

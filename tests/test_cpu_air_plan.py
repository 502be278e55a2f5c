"""The launch plan of the seven AIR entries (no GPU): csrc/air_plan.h and the marker of csrc/air_codegen.h, compiled on their own
with the address and undefined behaviour sanitizers, against tests/air_plan.py over every entry, size, expansion, alignment and CU
count and the edges of every count; what any statement of the plan must satisfy; and what the shapes of the -m gpu files reach."""
import os
import shutil
import subprocess

import pytest

import air_plan as AP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")
N_CUS = (1, 64, 256, 304)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/air_plan_main.cpp — csrc/air_plan.h, csrc/air_codegen.h and nothing else of the library — under the sanitizers."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("air_plan") / "air_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "air_plan_main.cpp"), "-o", out])
    return out


def _library_lines(exe, lines):
    p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _own(i):
    try:
        return AP.render(AP.plan(i))
    except AP.PlanError as e:
        return f"error: {AP.PREFIX.get(i.entry, '')}{e}"


def _sweep():
    """Every entry x log x log_expand x aligned x n_cus at plain counts, then each count at its edges."""
    out = []
    for entry in AP.ENTRIES:
        program_len = 10 if entry in AP.INTERPRETED else 0
        for log in range(30):
            for le in range(6):
                for aligned in (False, True):
                    for n_cus in N_CUS:
                        out.append(AP.Input(entry, AP.MUL_ADD, log, le, 3, 1, program_len, 3, aligned, n_cus))
        for log, le in ((9, 1), (2, 0), (28, 4)):
            for n_cols in (0, 1, 2, 3, 64, 65, 130, 131, 4096, 4097):
                for n_terminal in (0, 1, 64, 65, 128, 129, 256, 257, n_cols - 2 if n_cols > 2 else 1):
                    for kind in (AP.WIDE_FIB, AP.MUL_ADD, 2):
                        out.append(AP.Input(entry, kind, log, le, n_cols, n_terminal, program_len, 3, True, 256))
            for plen in (0, 1, 1536, 1537):
                for n_regs in (0, 1, 32):
                    for aligned in (False, True):
                        out.append(AP.Input(entry, AP.MUL_ADD, log, le, 3, 1, plen, n_regs, aligned, 256))
                        out.append(AP.Input(entry, AP.WIDE_FIB, log, le, 65, 63, plen, n_regs, aligned, 304))
    return out


def test_header_constants(exe):
    got = [int(w) for w in _library_lines(exe, ["C"])[0].split()]
    assert got == [AP.MAX_LOG, AP.MAX_LOG_EXPAND, AP.MAX_HAND_CONSTRAINTS, AP.WIDE_THREADS, AP.WIDE_CAP_PER_CU, AP.WAVE_THREADS, AP.WAVE_CAP_PER_CU,
                   AP.TABLE_BY_VALUE, 2 * AP.MAX_INSTR + 4 * AP.MAX_CONSTRAINTS]
    assert got == [28, 4, 128, 256, 16, 64, 32, 64, 4096]


def test_air_plan_matches_the_library(exe):
    """Both statements give the same launch, LDS, upload and tables for every input, and the same reason for those without a plan;
    and every plan satisfies what any statement of it must."""
    inputs = _sweep()
    got = _library_lines(exe, [AP.line(i) for i in inputs])
    reasons, planned = set(), 0
    for i, text in zip(inputs, got):
        assert text == _own(i), i
        if text.startswith("error: "):
            reasons.add(text)
            continue
        planned += 1
        p, rows = AP.plan(i), 1 << i.log
        assert p.grid >= 1 and p.w in (1, 4) and p.threads in (64, 256)
        assert p.grid * p.threads * p.w >= rows or AP.strides(i)
        assert p.grid * p.threads * p.w < rows + p.threads * p.w or p.grid == 1     # no workgroup without a row, but the first
        assert p.lds_bytes <= (32 + 2) * 1024
        assert p.upload_words * 4 <= 16 * 1024 and p.coeff_word <= p.upload_words
        assert p.stride == (p.grid * p.threads if i.entry in AP.COMPILED else 0)
        assert p.w == 1 or rows % 4 == 0
        assert p.w == 1 or i.aligned                                               # 16-byte loads only where the caller saw alignment
        assert (p.lds_bytes > 0) == (i.entry in AP.INTERPRETED) and (p.tally_word > 0) == (i.entry == "check")
        assert p.tally_word * 4 + 8 * i.n_terminal == p.lds_bytes or i.entry != "check"
        assert p.capturable <= (i.entry in ("wide_fib_trace", "quotients", "eval_columns_compiled"))
    assert planned > 5000
    # every text an entry can give for a count or a size is among the refusals
    want = {"wide Fibonacci needs at least 2 columns", "trace too large", "wide Fibonacci: N >= 3 columns, N - 2 constraints",
            "mul-add: 3 columns, 1 constraint", "unknown constraint kind", "too many constraints in one component", "log_expand too large",
            "evaluation domain too large", "air program: program length out of range",
            "air program: log_expand must be at least 1 (the neighbour index needs eval > trace)", "air program: log_expand too large",
            "air program: evaluation domain too large", "air program: number of columns out of range",
            "air program: number of constraints out of range", "air columns: log_size out of range", "air columns: number of columns out of range",
            "air columns: number of outputs out of range", "air columns: program length out of range", "air check: log_size out of range",
            "air check: number of columns out of range", "air check: number of constraints out of range", "air check: program length out of range"}
    assert reasons == {"error: " + t for t in want}


def test_the_order_of_the_refusals(exe):
    """An input wrong in every way gets the first reason of its entry, on both sides."""
    first = {"wide_fib_trace": "wide Fibonacci needs at least 2 columns", "quotients": "wide Fibonacci: N >= 3 columns, N - 2 constraints",
             "eval_program": "air program: program length out of range",
             "eval_compiled": "air program: log_expand must be at least 1 (the neighbour index needs eval > trace)",
             "eval_columns": "air columns: log_size out of range", "eval_columns_compiled": "air columns: log_size out of range",
             "check": "air check: log_size out of range"}
    inputs = [AP.Input(e, AP.WIDE_FIB, 0, 0, 0, 0, 0, 0, True, 256) for e in AP.ENTRIES]
    got = _library_lines(exe, [AP.line(i) for i in inputs])
    assert got == ["error: " + first[e] for e in AP.ENTRIES] == [_own(i) for i in inputs]
    # and the later ones in their turn: log_expand before the domain, the domain before the counts
    i = AP.Input("eval_compiled", 0, 34, 5, 0, 0, 0, 0, True, 256)
    assert _own(i) == "error: air program: log_expand too large" and _own(i._replace(log_expand=4)) == "error: air program: evaluation domain too large"
    assert _own(i._replace(log_expand=4, log=28)) == "error: air program: number of columns out of range"
    assert _own(AP.Input("quotients", AP.WIDE_FIB, 34, 5, 131, 129, 0, 0, True, 256)) == "error: too many constraints in one component"


def test_plans_written_out():
    """A few plans by hand, from the kernels' own description (csrc/air.hip): 256 CUs."""
    P = AP.plan
    # 2^20 rows in fours: 1024 workgroups of 256 lanes, below the 4096 of 16 per CU; nothing uploaded, so it can be captured
    assert P(AP.Input("quotients", AP.MUL_ADD, 20, 1, 3, 1, 0, 0, True, 256)) == AP.Plan(4, 256, 1024, 0, 0, 0, 0, 0, True, True, True)
    # 2^23 rows in fours are 8192 workgroups: capped at 4096, every lane takes two turns
    assert P(AP.Input("wide_fib_trace", 0, 23, 0, 100, 0, 0, 0, True, 256)) == AP.Plan(4, 256, 4096, 0, 0, 0, 0, 0, False, True, False)
    # the interpreter: 5 registers x 64 lanes x 4 rows x 4 bytes; 40 instructions and 5 coefficients uploaded
    assert P(AP.Input("eval_program", 0, 10, 2, 6, 5, 40, 5, True, 256)) == AP.Plan(4, 64, 4, 0, 5120, 0, 100, 80, True, True, False)
    assert P(AP.Input("eval_compiled", 0, 21, 2, 3, 2, 0, 0, False, 256)) == AP.Plan(1, 256, 4096, 4096 * 256, 0, 0, 8, 0, True, True, False)
    # the check: the pairs of 3 constraints behind 2 registers of one-row lanes
    assert P(AP.Input("check", 0, 9, 0, 4, 3, 20, 2, False, 256)) == AP.Plan(1, 64, 8, 0, 512 + 24, 128, 40, 0, True, True, False)
    # a program that writes no register still has one slot per lane
    assert P(AP.Input("eval_columns", 0, 1, 0, 1, 1, 1, 0, True, 256)).lds_bytes == 256
    assert [AP.first_striding_log(e, w, 256) for e in ("quotients", "eval_program", "check") for w in (4, 1)] == [23, 21, 22, 20, 22, 20]
    assert AP.first_striding_log("wide_fib_trace", 4, 1) == 15 and AP.first_striding_log("eval_columns", 1, 1) == 12


# ---------------------------------------------------------------- the marker
def _acc(c, reg=0, dst=0):
    return [AP.OP_ACC | dst << 8 | reg << 16, c]


LOADS = [0 | 0 << 8 | 0 << 16, 0, 0 | 1 << 8 | 1 << 16, 1]            # r0 = column 0, r1 = column 1 one row on


def _marks(words):
    return [(w >> 8) & 0xff for w in words[::2] if w & 0xff == AP.OP_ACC]


@pytest.mark.parametrize("indices", [[0], [0, 0, 0, 0], [0, 0, 1, 2, 2, 2, 2, 3]], ids=["one", "secure", "mixed"])
def test_marker_matches_the_library(exe, indices):
    """The last ACC of every constraint index carries dst = 1 and every other ACC dst = 0, whatever dst they came with; every
    other word is as it was."""
    for dst_in in (0, 1, 0xff):
        words = list(LOADS)
        for k, c in enumerate(indices):
            words += _acc(c, k & 1, dst_in)
            if k == 1:
                words += [2 | 1 << 8 | 0 << 16, 1]                  # r1 = r0 + r1 between two ACCs: dst 1 stays
        want = AP.mark_last_acc(words)
        got = [int(w) for w in _library_lines(exe, [f"M {indices[-1] + 1} 2 " + " ".join(map(str, words))])[0].split()]
        assert got == want
        assert _marks(got) == [int(k + 1 == len(indices) or indices[k + 1] != c) for k, c in enumerate(indices)]
        assert [(a, b) for a, b in zip(got[::2], words[::2]) if a & 0xff != AP.OP_ACC and a != b] == [] and got[1::2] == words[1::2]


def test_marker_refuses_with_the_validator(exe):
    got = _library_lines(exe, ["M 2 2 " + " ".join(map(str, LOADS + _acc(1)))])
    assert got == ["error: first constraint index is not 0"]


def test_register_program_writes_the_registers_it_says(exe):
    """tests/air_plan.py register_program, which the GPU tests and tools run: the validator accepts it at 1 and at 32 registers."""
    for n_regs in (1, 2, 32):
        words = AP.register_program(n_regs, 3, [0, 1])
        assert len(words) // 2 == 2 * n_regs - 1 + 2
        assert {(w >> 8) & 0xff for w in words[::2] if w & 0xff != AP.OP_ACC} == set(range(n_regs))
        assert not _library_lines(exe, ["M 2 3 " + " ".join(map(str, words))])[0].startswith("error")


# ---------------------------------------------------------------- coverage
def test_gpu_shapes_reach_every_branch():
    """The coverage condition: the calls of the -m gpu files, none over 2^23 rows, reach every entry's kernel at W = 4 and at W = 1,
    each of them with and without a second turn round the grid, both causes of W = 1, the column table by value and in device
    memory, and the check's tally behind 1 and behind 32 registers — on a part of 256 CUs and on one of 304."""
    want = AP.reachable_branches()
    assert want == ({f"{e}:w{w}:{s}" for e in AP.ENTRIES for w in (4, 1) for s in ("fit", "stride")}
                    | {"w1:short", "w1:misaligned", "table:value", "table:device", "tally:1", "tally:32"})
    for n_cus in (256, 304):
        reached = set()
        for name, i in AP.gpu_shapes(n_cus).items():
            assert 1 << i.log <= AP.MAX_GPU_ROWS, name
            assert AP.refuse(i) is None, name
            reached |= AP.branches(i)
        assert reached == want, (n_cus, sorted(want - reached))
    # the stride shapes are the smallest that stride: one log less fits the grid
    for name, i in AP.gpu_shapes().items():
        if "stride" in name:
            assert AP.strides(i) and not AP.strides(i._replace(log=i.log - 1)), name

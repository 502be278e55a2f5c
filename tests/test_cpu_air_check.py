"""tstwo_air_check_constraints without a GPU: the validator check_assert_program of csrc/air_codegen.h in a stand-alone program
(tests/air_check_main.cpp, built with the address and undefined-behaviour sanitizers, no Python in the process); the integer model
tests/air_check_model.py tied to a second definition written out on integers (which constraints and rows a changed cell breaks,
and the wrap of a row offset); and the resource usage of k_air_check, compiled for gfx950 without a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import air_check_model as CK
import air_model as AM
import air_program_model as X
import logup_model as LM
from tstwo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")
P = X.P
STORE = 8
MAX_INSTR, MAX_REGS, MAX_CONSTRAINTS, MAX_COLS, MAX_OFFSET = 1536, 32, 256, 4096, 64


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("air_check") / "air_check_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "air_check_main.cpp"), "-o", out])
    return out


def _run(exe, cases, acc=False):
    """One answer per case (n_cols, n_constraints, words): the reason of a refusal, or ("ok", n_regs)."""
    text = "".join(f"{c} {k} " + " ".join(str(w & 0xffffffff) for w in words) + "\n" for c, k, words in cases)
    p = subprocess.run([exe] + (["acc"] if acc else []), input=text.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    return [ln[len("error: "):] if ln.startswith("error: ") else ("ok", int(ln.split()[1])) for ln in lines]


def accs(indices, reg=0):
    """one ACC of register `reg` per constraint index"""
    return [w for c in indices for w in X.encode(X.ACC, 0, reg, c)]


LOAD2 = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)


def test_valid_groupings_are_accepted(exe):
    rng = np.random.default_rng(5)
    largest = CK.with_groups(X.random_program(rng, MAX_COLS, 300, MAX_INSTR - 300, max_offset=MAX_OFFSET),
                             CK.grouping([1] * 212 + [2] * 44))                        # 300 ACCs in 256 constraints
    cases = [(2, 6, LOAD2 + accs(range(6))),                                         # the identity
             (2, 3, LOAD2 + accs(CK.grouping([1, 4, 1]))),
             (2, 1, LOAD2 + accs([0] * 7)),                                           # every ACC in one constraint
             (2, 1, LOAD2 + accs([0])),
             (2, 2, X.encode(X.LOAD, 0, 0, 0) + accs([0, 0]) + X.encode(X.LOAD, 1, 1, -1) + accs([1], reg=1)),
             (MAX_COLS, MAX_CONSTRAINTS, largest)]
    got = _run(exe, cases)
    assert [g[0] for g in got] == ["ok"] * len(cases), got
    assert got[0] == ("ok", 2) and got[-1] == ("ok", MAX_REGS)


def test_malformed_groupings_are_refused_each_with_its_reason(exe):
    bad = [("first constraint index is not 0", (2, 2, LOAD2 + accs([1, 1]))),
           ("constraint index decreases", (2, 2, LOAD2 + accs([0, 1, 0]))),
           ("constraint index decreases", (2, 3, LOAD2 + accs([0, 1, 2, 1, 2]))),
           ("constraint index skips", (2, 3, LOAD2 + accs([0, 2]))),
           ("constraint index skips", (2, 3, LOAD2 + accs([0, 0xffffffff]))),
           ("constraint index out of range", (2, 2, LOAD2 + accs([0, 1, 2]))),
           ("constraint index out of range", (2, 1, LOAD2 + accs([0, 1]))),
           ("last constraint index is not n_constraints - 1", (2, 3, LOAD2 + accs([0, 1]))),
           ("last constraint index is not n_constraints - 1", (2, 2, LOAD2 + accs([0, 0]))),
           ("last constraint index is not n_constraints - 1", (2, 1, LOAD2))]           # no ACC at all
    got = _run(exe, [c for _, c in bad])
    assert got == [why for why, _ in bad]


def test_everything_else_has_the_acc_programs_reasons(exe):
    """the same lines through check_assert_program and check_acc_program: one reason"""
    ok = X.encode(X.LOAD, 0, 1, -2) + accs([0])
    bad = [("bad opcode", (2, 1, LOAD2 + X.encode(STORE, 0, 0, 0))),                                  # STORE
           ("bad opcode", (2, 1, LOAD2 + X.encode(9, 1, 0, 0) + accs([0]))),
           ("register out of range or read before written", (2, 1, LOAD2 + accs([0], reg=2))),
           ("register out of range or read before written", (2, 1, X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ADD, 1, 0, 5) + accs([0], reg=1))),
           ("register out of range or read before written", (2, 1, X.encode(X.LOAD, MAX_REGS, 0, 0) + accs([0], reg=MAX_REGS))),   # too many registers
           ("register out of range or read before written", (2, 1, X.encode(X.ADD, 0, 31, 0xffffffff) + accs([0]))),
           ("column out of range", (2, 1, X.encode(X.LOAD, 0, 2, 0) + accs([0]))),
           ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, MAX_OFFSET + 1) + accs([0]))),
           ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, -MAX_OFFSET - 1) + accs([0]))),
           ("constant out of range", (2, 1, X.encode(X.CONST, 0, 0, P) + accs([0]))),
           ("program length out of range", (2, 1, [])),
           ("program length out of range", (2, 1, [7])),                                               # half an instruction
           ("program length out of range", (2, 1, X.encode(X.CONST, 0, 0, 1) * MAX_INSTR + accs([0]))),
           ("number of columns out of range", (0, 1, ok)),
           ("number of columns out of range", (MAX_COLS + 1, 1, ok)),
           ("number of constraints out of range", (2, 0, ok)),
           ("number of constraints out of range", (2, MAX_CONSTRAINTS + 1, ok))]
    cases = [c for _, c in bad]
    assert _run(exe, cases) == [why for why, _ in bad]
    assert _run(exe, cases, acc=True) == [why for why, _ in bad]
    assert _run(exe, [(2, 1, ok)]) == _run(exe, [(2, 1, ok)], acc=True) == [("ok", 1)]


# ------------------------------------------------------------------ the model against a second definition on integers
def wide_fib_words(n_cols):
    """constraint i = x_{i+2} - (x_i^2 + x_{i+1}^2), written instruction by instruction"""
    w = []
    for i in range(n_cols - 2):
        w += (X.encode(X.LOAD, 0, i, 0) + X.encode(X.SQR, 0, 0) + X.encode(X.LOAD, 1, i + 1, 0) + X.encode(X.SQR, 1, 1)
              + X.encode(X.ADD, 0, 0, 1) + X.encode(X.LOAD, 1, i + 2, 0) + X.encode(X.SUB, 0, 1, 0) + X.encode(X.ACC, 0, 0, i))
    return w


@pytest.mark.parametrize("j,k", [(0, 0), (1, 5), (4, 63), (6, 17), (7, 64), (3, 127)])
def test_a_changed_wide_fibonacci_cell_breaks_its_three_constraints_on_its_row(j, k):
    log, n_cols = 7, 8
    rng = np.random.default_rng(11)
    a, b = (rng.integers(1, P, size=1 << log, dtype=np.uint64) for _ in range(2))
    cols = [np.asarray(c, dtype=np.uint64).copy() for c in AM.wide_fib_trace(a, b, n_cols)]
    words, groups = wide_fib_words(n_cols), list(range(n_cols - 2))
    assert CK.report(words, cols, log, groups) == [(0, CK.NO_ROW)] * (n_cols - 2)
    pos = int(LM.positions(log)[k])                      # coset row k is stored there
    cols[j][pos] = (cols[j][pos] + 1) % P
    x = int(cols[j][pos])
    assert (2 * x - 1) % P != 0                          # x^2 - (x - 1)^2: the square changed as well
    want = [(1, k) if c in (j - 2, j - 1, j) else (0, CK.NO_ROW) for c in range(n_cols - 2)]
    assert sum(n for n, _ in want) == len({j - 2, j - 1, j} & set(range(n_cols - 2)))
    assert CK.report(words, cols, log, groups) == want


@pytest.mark.parametrize("log", [1, 2, 6])
def test_an_offset_wraps_from_the_last_row_to_the_first(log):
    """a[k + 1] - a[k] - b[k] in coset order, row 2^log - 1 reading row 0: a changed a[0] breaks rows 0 and 2^log - 1"""
    n = 1 << log
    rng = np.random.default_rng(12 + log)
    b_seq = rng.integers(0, P, size=n, dtype=np.uint64)
    b_seq[-1] = (P - int(b_seq[:-1].sum() % P)) % P        # the sums close the circle
    a_seq = np.empty(n, dtype=np.uint64)
    a_seq[0] = 12345
    for k in range(1, n):
        a_seq[k] = (a_seq[k - 1] + b_seq[k - 1]) % P
    assert (a_seq[-1] + b_seq[-1]) % P == a_seq[0]
    pos = LM.positions(log)
    a, b = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    a[pos], b[pos] = a_seq, b_seq
    words = (X.encode(X.LOAD, 0, 0, 1) + X.encode(X.LOAD, 1, 0, 0) + X.encode(X.SUB, 0, 0, 1) + X.encode(X.LOAD, 1, 1, 0)
             + X.encode(X.SUB, 0, 0, 1) + X.encode(X.ACC, 0, 0, 0))
    assert CK.report(words, [a, b], log, [0]) == [(0, CK.NO_ROW)]
    a[pos[0]] = (a[pos[0]] + 1) % P
    [value] = X.run_program(words, [a, b], log, 0)
    failing = sorted(int(CK.coset_rows(log)[r]) for r in np.flatnonzero(value))
    assert failing == sorted({0, n - 1})
    assert CK.report(words, [a, b], log, [0]) == [(len({0, n - 1}), 0)]


def test_a_constraint_of_several_accs_counts_a_row_once():
    log = 4
    pos = LM.positions(log)
    cols = [np.zeros(1 << log, dtype=np.uint64) for _ in range(4)]
    words = [w for i in range(4) for w in X.encode(X.LOAD, i, i, 0)] + [w for i in range(4) for w in X.encode(X.ACC, 0, i)]
    cols[3][pos[9]] = 5                                  # row 9: the last coordinate alone
    assert CK.report(words, cols, log, [0, 0, 0, 0]) == [(1, 9)]
    cols[0][pos[9]] = 7                                  # two coordinates on one row: still one row
    cols[1][pos[3]] = 1                                  # and another row in another coordinate
    assert CK.report(words, cols, log, [0, 0, 0, 0]) == [(2, 3)]
    assert CK.report(words, cols, log, [0, 1, 2, 3]) == [(1, 9), (1, 3), (0, CK.NO_ROW), (1, 9)]
    assert CK.report(words, cols, log, [0, 0, 1, 1]) == [(2, 3), (1, 9)]
    assert list(CK.report_words(words, cols, log, [0, 0, 1, 1])) == [2, 3, 1, 9]


# ------------------------------------------------------------------ the kernel compiles clean
def test_the_check_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    """csrc/air.hip for gfx950 without a device: k_air_check at W = 4 and W = 1 reports no scratch, and neither does any other
    kernel of the file."""
    p = subprocess.run([B._hipcc(), *B.FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "air.hip"), "-o", str(tmp_path / "air.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, kernel = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: \s*(.+?): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            kernel = usage.setdefault(m.group(2), {})
        elif kernel is not None:
            kernel[m.group(1)] = m.group(2)
    new = {k: u for k, u in usage.items() if "k_air_checkILi" in k}
    assert len(new) == 2 and any("ILi4E" in k for k in new) and any("ILi1E" in k for k in new), sorted(usage)
    for k, u in sorted(usage.items()):
        print(k, "VGPRs", u["VGPRs"], "SGPRs", u["TotalSGPRs"], "occupancy", u["Occupancy [waves/SIMD]"], "scratch", u["ScratchSize [bytes/lane]"])
        assert u["ScratchSize [bytes/lane]"] == "0", (k, u)

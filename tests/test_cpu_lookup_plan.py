"""The launch plan of tstwo_lookup_multiplicities (no GPU): csrc/lookup_plan.h, compiled on its own, against tests/lookup_plan.py
over every log_range, the lengths around each path's edges and every alignment; the numpy model of the counts against the host
functions it stands in for; and what the shapes of the -m gpu file reach."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lookup_plan as LP
from tstwo_amd import constraint_framework as F


def _library_plans(tmp_path, inputs):
    """One line of lookup_plan_main per input (log_range, order, addrs, lens)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lookup_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"),
                           os.path.join(here, "lookup_plan_main.cpp"), "-o", exe])
    text = "".join(f"{lg} {order} {' '.join(f'{a} {n}' for a, n in zip(addrs, lens))}\n" for lg, order, addrs, lens in inputs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(inputs)
    return got


def _own(lg, order, addrs, lens):
    try:
        return LP.render(LP.plan(lg, addrs, lens, order))
    except LP.PlanError as e:
        return f"error: {e}"


BASE = 0x7F0000001000            # a 16-byte aligned device address


def test_lookup_plan_matches_the_library(tmp_path):
    """Both statements give the same branch, workgroup, grid, wrap point and vec bits: a single column of every length around
    the unit, the workgroup and the wrap point at every alignment and every log_range, and calls of 2, 5 and 64 columns."""
    inputs = []
    for lg in range(1, LP.MAX_LOG + 1):
        w = LP.wrap(lg)
        for n in (0, 1, 3, 4, 5, 255, 256, 257, w - 1, w, w + 1):
            for off in (0, 4, 8, 12):
                inputs.append((lg, lg & 1, [BASE + off], [n]))
        for n_cols in (2, 5, 64):
            w = LP.wrap(lg, n_cols)
            lens = [(w + 1, 0, 5, 4 * LP._shape(lg, n_cols)[0] + 1, 3)[c % 5] for c in range(n_cols)]
            inputs.append((lg, 1, [BASE + 4 * (c % 4) for c in range(n_cols)], lens))
    got = _library_plans(tmp_path, inputs)
    branches = set()
    for (lg, order, addrs, lens), line in zip(inputs, got):
        assert line == _own(lg, order, addrs, lens), (lg, order, addrs, lens)
        p = LP.plan(lg, addrs, lens, order)
        branches.add(p.branch)
        # what any statement of the plan must satisfy: every unit of every column is some lane's, and the cap holds
        assert p.grid_x * p.grid_y <= max(LP.LDS_CAP if p.branch == "LDS" else LP.GLOBAL_CAP, p.grid_y)
        assert p.grid_x * p.threads * LP.UNIT <= p.wrap
        assert (p.grid_x == 0) == (sum(lens) == 0)
        for a, n, v in zip(addrs, lens, p.vec):
            assert not v or (a % 16 == 0 and n >= 4)
        if max(lens) <= p.wrap:
            assert p.grid_x * p.threads * LP.UNIT >= max(lens)               # below the wrap point no lane takes a second unit
    assert branches == {"LDS", "GLOBAL"}
    assert LP.plan(LP.LDS_MAX_LOG, [0], [1]).branch == "LDS" and LP.plan(LP.LDS_MAX_LOG + 1, [0], [1]).branch == "GLOBAL"


def test_lookup_plan_rejections(tmp_path):
    """the inputs without a plan, each with its reason, from both statements"""
    big = LP.MAX_VALUES
    cases = [(0, 1, [BASE], [8], "log_range must be 1 to 28"), (29, 1, [BASE], [8], "log_range must be 1 to 28"),
             (8, 1, [], [], "1 to 64 columns"), (8, 1, [BASE] * 65, [1] * 65, "1 to 64 columns"),
             (8, 2, [BASE], [8], "order must be 0 (natural) or 1 (coset)"),
             (8, 1, [BASE], [big + 1], "more than 2^31 - 2 values"), (8, 0, [BASE, BASE], [big, 1], "more than 2^31 - 2 values"),
             (8, 1, [BASE], [big], None), (28, 0, [BASE, BASE + 4], [big - 1, 1], None), (8, 1, [BASE] * 64, [1] * 64, None)]
    got = _library_plans(tmp_path, [c[:4] for c in cases])
    for (lg, order, addrs, lens, why), line in zip(cases, got):
        assert line == _own(lg, order, addrs, lens), (lg, order, lens)
        assert line == f"error: {why}" if why else not line.startswith("error")


@pytest.mark.parametrize("log_range", range(1, 11))
def test_model_matches_the_host_functions(log_range):
    """The numpy model is what the GPU tests compare with: in coset order it is F.range_check_multiplicities, in natural order
    np.bincount; its positions are the framework's; a word outside the range is left out and counted."""
    rng = np.random.default_rng(4200 + log_range)
    cols = [rng.integers(0, 1 << log_range, size=n) for n in (0, 1, 257, 4099)]
    got, rejected = LP.multiplicities(log_range, cols, "coset")
    assert rejected == 0 and np.array_equal(got, F.range_check_multiplicities(log_range, *cols))
    got, rejected = LP.multiplicities(log_range, cols, "natural")
    assert rejected == 0 and np.array_equal(got, np.bincount(np.concatenate(cols), minlength=1 << log_range))
    assert np.array_equal(LP.coset_positions(log_range), F._coset_positions(log_range))
    table = np.empty(1 << log_range, dtype=np.uint32)
    table[LP.coset_positions(log_range)] = np.arange(1 << log_range)
    assert np.array_equal(table, F.range_check_table_column(log_range))
    outside = np.array([1 << log_range, LP.MAX_VALUES, 0], dtype=np.uint32)
    with_out, rejected = LP.multiplicities(log_range, cols + [outside], "natural")
    assert rejected == 2 and with_out[0] == got[0] + 1 and np.array_equal(with_out[1:], got[1:])


def test_gpu_shapes_reach_every_path():
    """The shapes tests/test_gpu_lookup.py runs, with the addresses it gives them (a 16-byte aligned allocation, or one word
    into it), reach per branch: 16-byte units, a column read word by word, a partial last unit, an empty column, workgroups
    without work, and lanes that take a second unit."""
    reached = {"LDS": set(), "GLOBAL": set()}
    for name, (lg, cols) in LP.gpu_shapes().items():
        got = LP.reaches(lg, [BASE + 4 * off for _, off in cols], [n for n, _ in cols])
        reached[LP.branch(lg)] |= got
        if name.startswith("wrap"):
            assert "wrap" in got and sum(n for n, _ in cols) == LP.wrap(lg) + 1029, name
    for b, got in reached.items():
        assert got == {b, "vec", "scalar", "tail", "empty", "idle", "wrap"}, (b, sorted(got))
    assert {LP.LAST_LDS_LOG, LP.FIRST_GLOBAL_LOG, 1, 2, 8, 16} == set(LP.PARITY_LOGS)
    assert max(LP.wrap(lg) for lg in range(1, LP.MAX_LOG + 1)) <= 1 << 23         # the wrap is reached without a cap knob

"""The schedule of tstwo_fri_commit_layers_poseidon252 (no GPU): the unfused plan of csrc/fri_plan.h (fused = false), compiled on its
own with the sanitizers, against its restatement below; and the shape list of tests/test_gpu_fri_poseidon_commit.py held to both
sides of kP252CoopMaxLog (csrc/poseidon_plan.h), read from the compiled header."""
import itertools
import os
import shutil
import subprocess

import pytest

import fri_poseidon_shapes as S

UNFUSED = ("FIRST_TREE", "CIRCLE_WRITE", "COMMIT", "FOLD_LINE", "CIRCLE_ACCUM")


def plan(col_logs, last):
    """commitInnerLayers (fri.ts:676-716) step by step: tree, mix / draw, fold, one launch each.  Steps are
    (kind, layer, log, column, alpha_in, alpha_out); a string is the reason an input has no schedule."""
    if not col_logs:
        return "no columns"
    for i, c in enumerate(col_logs):
        if not 3 <= c <= 31:
            return "fri commit: circle evaluations of log size 3..31"
        if i and col_logs[i - 1] <= c:
            return "column sizes not decreasing"
    layer, log = 0, col_logs[0] - 1
    if last > log:
        return "fri commit: last layer larger than the first line layer"
    steps = [("FIRST_TREE", 0, col_logs[0], 0, 0, 0), ("CIRCLE_WRITE", 0, log, 0, 0, 0)]
    nxt = 1
    while log > last:
        steps.append(("COMMIT", layer, log, 0, 0, layer + 1))          # the tree of the layer, then alpha layer + 1 ...
        layer, log = layer + 1, log - 1
        steps.append(("FOLD_LINE", layer, log, 0, layer, 0))            # ... which folds it into the next
        if nxt < len(col_logs) and col_logs[nxt] - 1 == log:
            steps.append(("CIRCLE_ACCUM", layer, log, nxt, layer, 0))   # and the circle column of that size with it
            nxt += 1
    if nxt != len(col_logs):
        return "not all columns were consumed"
    return steps


def _library(tmp_path, inputs):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "fri_plan_poseidon_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"), os.path.join(here, "fri_plan_poseidon_main.cpp"),
            "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:        # a toolchain without the sanitizer runtimes
        subprocess.check_call(base)
    text = "".join(f"{last} {' '.join(map(str, col_logs))}\n" for col_logs, last in inputs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].startswith("kP252CoopMaxLog ") and len(out) == len(inputs) + 1
    return int(out[0].split()[1]), out[1:]


def _parse(line):
    if line.startswith("error: "):
        return line[len("error: "):]
    steps = []
    for word in line.split():
        kind, *nums = word.split(":")
        steps.append((kind, *(int(x) for x in nums)))
    return steps


def test_unfused_plan_matches_the_library(tmp_path):
    inputs = [(list(c), last) for n in (1, 2, 3) for c in itertools.combinations(range(12, 2, -1), n) for last in range(c[0])]
    inputs += [([15], 3), ([31, 30], 3), ([16, 15, 14, 13], 0)]
    _, got = _library(tmp_path, inputs)
    accepted = rejected = 0
    for (col_logs, last), line in zip(inputs, got):
        lib, own = _parse(line), plan(col_logs, last)
        assert lib == own, (col_logs, last, line)
        if isinstance(lib, str):
            rejected += 1
            continue
        accepted += 1
        assert {s[0] for s in lib} <= set(UNFUSED)                       # no FOLD_COMMIT, no TAIL
        n_inner = col_logs[0] - 1 - last
        assert [s[5] for s in lib if s[0] in ("FIRST_TREE", "COMMIT")] == list(range(n_inner + 1))     # alpha k behind the k-th tree
        assert sum(s[0] == "CIRCLE_ACCUM" for s in lib) == len(col_logs) - 1
    assert accepted and rejected


@pytest.mark.parametrize("col_logs,last,steps", [
    ([5], 1, "FIRST_TREE:0:5:0:0:0 CIRCLE_WRITE:0:4:0:0:0 COMMIT:0:4:0:0:1 FOLD_LINE:1:3:0:1:0 COMMIT:1:3:0:0:2 FOLD_LINE:2:2:0:2:0 "
                "COMMIT:2:2:0:0:3 FOLD_LINE:3:1:0:3:0"),                                    # one column
    ([6, 5, 3], 1, "FIRST_TREE:0:6:0:0:0 CIRCLE_WRITE:0:5:0:0:0 COMMIT:0:5:0:0:1 FOLD_LINE:1:4:0:1:0 CIRCLE_ACCUM:1:4:1:1:0 COMMIT:1:4:0:0:2 "
                   "FOLD_LINE:2:3:0:2:0 COMMIT:2:3:0:0:3 FOLD_LINE:3:2:0:3:0 CIRCLE_ACCUM:3:2:2:3:0 COMMIT:3:2:0:0:4 FOLD_LINE:4:1:0:4:0"),   # joining columns
    ([5], 4, "FIRST_TREE:0:5:0:0:0 CIRCLE_WRITE:0:4:0:0:0"),                               # the last layer is the first line layer
])
def test_unfused_plan_spelled_out(tmp_path, col_logs, last, steps):
    _, got = _library(tmp_path, [(col_logs, last)])
    assert got[0] == steps
    assert _parse(got[0]) == plan(col_logs, last)


def test_refusals(tmp_path):
    cases = [([], 0, "no columns"), ([2], 0, "log size 3..31"), ([32], 5, "log size 3..31"), ([8, 8], 2, "column sizes not decreasing"),
             ([8, 9], 2, "column sizes not decreasing"), ([8], 8, "last layer larger than the first line layer"),
             ([8, 5], 5, "not all columns were consumed")]
    _, got = _library(tmp_path, [(c, last) for c, last, _ in cases])
    for (col_logs, last, why), line in zip(cases, got):
        lib = _parse(line)
        assert isinstance(lib, str) and why in lib and lib == plan(col_logs, last)


def test_the_fused_plan_is_unchanged(tmp_path):
    """fri_plan(col_logs, n, last, steps) still compiles with four arguments and still fuses: tests/fri_plan_main.cpp, unchanged, prints a
    FOLD_COMMIT and a TAIL for a shape that has both"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "fri_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"),
                           os.path.join(here, "fri_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], input="2 14\n", capture_output=True, text=True, check=True).stdout
    assert "FOLD_COMMIT" in out and "TAIL" in out


def test_gpu_shapes_take_both_kinds_of_layer_kernel(tmp_path):
    """at least one tree layer of the GPU FRI test's shapes is hashed by each kernel: the cooperative one (log <= kP252CoopMaxLog) and
    the lane-per-node one (above); with the constant at "never" (negative) every layer takes the latter"""
    k, _ = _library(tmp_path, [])
    logs = [lg for col_logs, bound in S.SHAPES for lg in S.tree_layer_logs(col_logs, bound)]
    assert any(lg > k for lg in logs)
    if k >= 0:
        assert any(lg <= k for lg in logs)
        # ... and inside ONE tree, so that a cooperative layer reads children the other kernel wrote
        assert any(col_logs[0] > k for col_logs, _ in S.SHAPES)
    # every shape is one the plan accepts
    for col_logs, bound in S.SHAPES:
        assert not isinstance(plan(col_logs, S.last_log(bound)), str)

"""The schedule of tstwo_fri_commit_layers (no GPU): csrc/fri_plan.h, compiled on its own, against tests/fri_plan.py, over every
strictly decreasing list of 1 to 3 circle logs out of 3..14 and every last layer from 2^0 rows to the first line layer; then what
every accepted schedule must satisfy whoever states it."""
import itertools
import os
import shutil
import subprocess

import pytest

import fri_plan as F


def _inputs():
    return [(list(c), last) for n in (1, 2, 3) for c in itertools.combinations(range(14, 2, -1), n) for last in range(c[0])]


def _parse(line):
    """A line of fri_plan_main: the steps, or the reason of the rejection."""
    if line.startswith("error: "):
        return line[len("error: "):]
    steps = []
    for word in line.split():
        kind, *nums = word.split(":")
        layer, log, column, alpha_in, alpha_out, n_layers, pre = (int(x) for x in nums)
        steps.append(F.Step(kind, layer, log, column, alpha_in, alpha_out, n_layers, bool(pre)))
    return steps


def _library_plans(tmp_path, inputs):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "fri_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"),
                           os.path.join(here, "fri_plan_main.cpp"), "-o", exe])
    text = "".join(f"{last} {' '.join(map(str, col_logs))}\n" for col_logs, last in inputs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(inputs)
    return got


def _own(col_logs, last):
    try:
        return F.plan(col_logs, last)
    except F.PlanError as e:
        return str(e)


def check_invariants(col_logs, last, steps):
    """What a schedule must satisfy, replayed step by step: who produced and committed which layer, which alpha was drawn when."""
    first_log = col_logs[0] - 1
    L = first_log - last
    joiner = {first_log - (c - 1): j for j, c in enumerate(col_logs) if j}       # layer -> the column due there
    produced, committed, consumed, drawn = [], [], [], []
    incoming = {}                                                               # layer -> the alpha entry that folded into it

    def complete(layer):            # its evaluation is there, and so is the column that joins it
        return layer in produced and (layer not in joiner or joiner[layer] in consumed)

    def produce(layer, alpha):
        assert alpha in drawn, (layer, alpha)
        if layer:
            assert alpha == layer and complete(layer - 1)
        produced.append(layer)
        incoming[layer] = alpha

    def commit(layer, alpha_out):
        assert layer < L and complete(layer) and alpha_out == layer + 1
        committed.append(layer)
        drawn.append(alpha_out)

    for s in steps:
        assert s.log == (col_logs[0] if s.kind == "FIRST_TREE" else first_log - s.layer), s
        if s.kind == "FIRST_TREE":
            assert not drawn and s.alpha_out == 0
            drawn.append(0)
        elif s.kind == "CIRCLE_WRITE":
            assert s.layer == 0 and s.column == 0
            produce(0, s.alpha_in)
            consumed.append(0)
        elif s.kind == "COMMIT":
            commit(s.layer, s.alpha_out)
        elif s.kind == "FOLD_COMMIT":
            assert s.layer not in joiner
            produce(s.layer, s.alpha_in)
            commit(s.layer, s.alpha_out)
        elif s.kind == "FOLD_LINE":
            produce(s.layer, s.alpha_in)
        elif s.kind == "CIRCLE_ACCUM":
            assert joiner.get(s.layer) == s.column and col_logs[s.column] - 1 == s.log
            assert s.layer in produced and s.layer not in committed and s.alpha_in == incoming[s.layer] and s.alpha_in in drawn
            consumed.append(s.column)
        else:
            assert s.kind == "TAIL" and s.log <= F.TAIL_LOG and s.n_layers == L - s.layer >= 1
            assert not any(j >= s.layer + (0 if s.pre else 1) for j in joiner)         # the tail folds no column in
            if s.pre:
                produce(s.layer, s.alpha_in)
            for k in range(s.n_layers):
                commit(s.layer + k, s.alpha_out + k)
                produce(s.layer + k + 1, s.alpha_out + k)
    assert sorted(produced) == list(range(L + 1))                  # every evaluation exactly once
    assert sorted(committed) == list(range(L))                     # every layer above the last exactly once, the last never
    assert sorted(consumed) == list(range(len(col_logs)))          # every column exactly once
    assert sorted(drawn) == list(range(L + 1)) == drawn            # entry i + 1 behind layer i's tree, in order, none past the count


def test_fri_plan_matches_the_library(tmp_path):
    """fri_plan.plan is the tests' own statement of the schedule; csrc/fri_plan.h is the library's.  A stand-alone program that
    includes only that header prints the library's schedule for every input: the two agree step for step, indices included, and
    reject the same inputs for the same reason; every step kind occurs; every accepted schedule satisfies check_invariants."""
    inputs = _inputs()
    got = _library_plans(tmp_path, inputs)
    seen, rejected = set(), 0
    for (col_logs, last), line in zip(inputs, got):
        lib, own = _parse(line), _own(col_logs, last)
        assert lib == own, (col_logs, last, line)
        if isinstance(lib, str):
            rejected += 1
            continue
        assert line == F.render(own)
        seen |= F.kinds(col_logs, last)
        check_invariants(col_logs, last, lib)
    assert seen == set(F.KINDS) | {"TAIL+pre"}
    assert 0 < rejected < len(inputs)


def test_fri_plan_rejections(tmp_path):
    """the inputs without a schedule, each with its reason, from both statements"""
    cases = [([], 0, "no columns"), ([2], 0, "log size 3..31"), ([32], 5, "log size 3..31"), ([8, 8], 2, "column sizes not decreasing"),
             ([8, 9], 2, "column sizes not decreasing"), ([8], 8, "last layer larger than the first line layer"),
             ([8, 5], 5, "not all columns were consumed"), ([31, 30], 3, None), ([8], 7, None)]
    got = _library_plans(tmp_path, [(c, last) for c, last, _ in cases])
    for (col_logs, last, why), line in zip(cases, got):
        lib, own = _parse(line), _own(col_logs, last)
        assert lib == own, (col_logs, last, line)
        if why is None:
            check_invariants(col_logs, last, lib)
        else:
            assert isinstance(lib, str) and why in lib


def test_invariants_reject_broken_schedules():
    """check_invariants is not vacuous: single changes to a good schedule fail it"""
    col_logs, last = [13, 12], 2
    good = F.plan(col_logs, last)
    check_invariants(col_logs, last, good)
    at = {s.kind: i for i, s in enumerate(good)}
    broken = [
        good[:at["CIRCLE_ACCUM"]] + good[at["CIRCLE_ACCUM"] + 1:],                                      # a column never consumed
        [s._replace(alpha_in=s.alpha_in + 1) if s.kind == "FOLD_COMMIT" else s for s in good],          # an alpha read before it is drawn
        [s._replace(n_layers=s.n_layers - 1) if s.kind == "TAIL" else s for s in good],                 # a layer never committed
        [s._replace(pre=False) if s.kind == "TAIL" else s for s in good],                               # a layer never produced
        good[:at["CIRCLE_ACCUM"]] + [good[at["CIRCLE_ACCUM"] + 1], good[at["CIRCLE_ACCUM"]]] + good[at["CIRCLE_ACCUM"] + 2:],  # committed before its column is in
    ]
    for steps in broken:
        with pytest.raises((AssertionError, KeyError)):
            check_invariants(col_logs, last, steps)

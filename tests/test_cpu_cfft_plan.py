"""The launch plan of the Circle FFT entries (no GPU): csrc/cfft_plan.h, compiled on its own, against tests/cfft_plan.py, over
n = 1..31 x 17 column counts x 256 and 64 compute units x every entry (evaluate_extended with ext 0..3) x no knob and every single
value of the experiments build's three; then what every accepted plan must satisfy whoever states it, which shapes are reached, and
the rows the design document quotes."""
import itertools
import os
import shutil
import subprocess

import pytest

import cfft_plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")
COLS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 256, 512, 1024)
KNOBS = [P.NO_KNOBS] + [(kb, 0, 0) for kb in range(11, 16)] + [(0, ka, 0) for ka in range(1, 11)] + [(0, 0, t) for t in range(12, 16)]
ENTRIES = [("evaluate", 0), ("interpolate", 0), ("interpolate_to", 0)] + [("evaluate_extended", e) for e in range(4)]


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _compile(out, *flags):
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-Wall", *flags, "-I", CSRC, os.path.join(HERE, "cfft_plan_main.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("cfft_plan") / "cfft_plan_main"))


def _line(entry, ext, n, n_cols, n_cus, knobs):
    return f"{P.ENTRIES.index(entry)} {ext} {n} {n_cols} {n_cus} {knobs[0]} {knobs[1]} {knobs[2]}\n"


def _library_plans(exe, inputs):
    got = subprocess.run([exe], input="".join(_line(*i) for i in inputs), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(inputs)
    return got


def _own(entry, ext, n, n_cols, n_cus, knobs):
    try:
        return P.render(P.plan(entry, n, n_cols, n_cus, knobs, ext))
    except P.PlanError as e:
        return f"error: {e}"


def _sweep():
    return [(entry, ext, n, n_cols, n_cus, knobs) for (entry, ext), n, n_cols, n_cus, knobs
            in itertools.product(ENTRIES, range(1, 32), COLS, (256, 64), KNOBS)]


def check_invariants(entry, ext, n, n_cols, plan):
    """What a plan must satisfy to transform every layer once, with kernels that exist, inside the limits of a workgroup."""
    inverse, in_place = entry in ("interpolate", "interpolate_to"), entry in ("evaluate", "interpolate")
    if plan.route == "fallback":
        assert not in_place and not plan.passes
        return
    assert plan.passes
    at = 0 if inverse else n                    # the passes cover the layers [0, n) once, contiguously, in execution order
    for i, s in enumerate(plan.passes):
        assert s.k >= 1 and s.lo == (at if inverse else at - s.k), s
        at = at + s.k if inverse else at - s.k
        assert s.scale == (inverse and i == len(plan.passes) - 1), s            # 2^-n on the last inverse pass only
        assert s.lds <= 160 * 1024 and s.threads <= 1024 and s.tiles * n_cols <= 0xffffffff, s
        if s.kind == "whole":
            assert plan.route in ("small", "generic") and len(plan.passes) == 1 and (n <= 2) == (plan.route == "small")
            assert plan.blocks * (plan.cols_per_wg or 64) >= n_cols
            continue
        assert plan.route == "tiled" and (s.kind, s.k, s.logt) in P.TABLE, s
        assert s.tiles << s.logt == 1 << n
        bottom = s.kind.startswith("bottom")
        assert bottom == (s.lo == 0)
        if bottom:
            assert s.logt == s.k
        else:
            assert s.logt - s.k >= 4 and s.logt - s.k <= s.lo, s                 # rows of 16 words and more, inside the layers below
        if s.kind.endswith("_stream"):
            assert not inverse and (n_cols << n) >= 1 << 28 and (s.logt in (13, 14) if bottom else s.logt == 15), s
        if s.kind in ("bottom_oop", "strided_ext"):
            assert i == 0 and entry == ("interpolate_to" if bottom else "evaluate_extended"), s
            assert bottom or (ext in (1, 2) and s.k >= 2), s
    assert at == (n if inverse else 0)
    if not in_place:                            # the entries that read a second table do so in their first pass
        assert plan.passes[0].kind == ("bottom_oop" if inverse else "strided_ext")


def _parse(line):
    head, *words = line.split()
    route, cpw, blocks = head.split(":")
    passes = []
    for w in words:
        kind, *nums = w.split(":")
        lo, k, logt, threads, lds, tiles, scale = (int(x) for x in nums)
        passes.append(P.Pass(kind, lo, k, logt, threads, lds, tiles, bool(scale)))
    return P.Plan(route, int(cpw), int(blocks), passes)


def test_cfft_plan_matches_the_library(exe):
    """cfft_plan.plan is the tests' own statement; csrc/cfft_plan.h is the library's.  A stand-alone program that includes only
    that header prints the library's plan for every input: the two agree field by field and refuse the same inputs for the same
    reason; every accepted plan satisfies check_invariants; every shape of the table is reached, the knob-only ones with a knob
    and never without."""
    inputs = _sweep()
    got = _library_plans(exe, inputs)
    reached, reached_shipped, refusals, routes = set(), set(), set(), set()
    for inp, line in zip(inputs, got):
        assert line == _own(*inp), inp
        entry, ext, n, n_cols, _, knobs = inp
        if line.startswith("error: "):
            refusals.add(line[len("error: "):])
            continue
        plan = _parse(line)
        check_invariants(entry, ext, n, n_cols, plan)
        routes.add(plan.route)
        reached |= P.shapes(plan)
        if knobs == P.NO_KNOBS:
            reached_shipped |= P.shapes(plan)
    assert reached == set(P.TABLE)
    assert reached_shipped == {s for s, knob_only in P.TABLE.items() if not knob_only}
    assert routes == set(P.ROUTES)
    assert refusals == {"cfft: log_size > 30 exceeds MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4)", "cfft: unsupported bottom pass",
                        "cfft: unsupported pass shape", "cfft: more passes than a plan holds"}


def test_table_matches_the_library(exe):
    rows = subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.splitlines()
    table = {(kind, int(k), int(logt)): bool(int(knob)) for kind, k, logt, knob in (r.split() for r in rows)}
    assert len(rows) == len(table) and table == P.TABLE


def test_refusals(exe):
    """the inputs without a plan, each with its reason, from both statements; the largest accepted ones beside them"""
    big = 1 << 40
    cases = [(("evaluate", 0, 0, 1, 256, P.NO_KNOBS), "log_size out of range"), (("interpolate", 0, 32, 1, 256, P.NO_KNOBS), "log_size out of range"),
             (("interpolate_to", 0, 31, 1, 256, P.NO_KNOBS), "exceeds MAX_CIRCLE_DOMAIN_LOG_SIZE"),
             (("evaluate", 0, 30, 1 << 15, 256, P.NO_KNOBS), "too many (tile, column) work items"),
             (("evaluate_extended", 1, 30, 1 << 15, 256, P.NO_KNOBS), "too many (tile, column) work items"),
             (("evaluate", 0, 12, 1 << 32, 256, P.NO_KNOBS), "too many (tile, column) work items"), (("interpolate", 0, 2, big, 256, P.NO_KNOBS), "too many (tile, column) work items"),
             (("evaluate", 0, 15, 4, 256, (15, 0, 0)), "unsupported bottom pass"), (("evaluate", 0, 13, 4, 256, (11, 0, 0)), "unsupported pass shape"),
             (("evaluate", 0, 17, 4, 256, (0, 1, 12)), "unsupported pass shape"),          # two knobs: one layer on the 2^12 tile
             (("interpolate", 0, 30, 4, 256, (0, 1, 0)), "more passes than a plan holds"),
             (("evaluate", 0, 30, (1 << 15) - 1, 256, P.NO_KNOBS), None), (("interpolate_to", 0, 30, 1024, 64, P.NO_KNOBS), None),
             (("evaluate", 0, 20, 4, 256, (0, 1, 0)), None), (("evaluate", 0, 12, (1 << 32) - 1, 256, P.NO_KNOBS), None)]
    got = _library_plans(exe, [c for c, _ in cases])
    for (inp, why), line in zip(cases, got):
        assert line == _own(*inp), inp
        if why is None:
            check_invariants(inp[0], inp[1], inp[2], inp[3], _parse(line))
        else:
            assert line.startswith("error: ") and why in line, (inp, line)


def _short(plan):
    return [("B" if s.lo == 0 else "A", s.k, s.logt) for s in plan.passes]


@pytest.mark.parametrize("n,cols,want", [
    (13, (1,), [("B", 13, 13)]), (14, COLS, [("B", 14, 14)]), (15, (1,), [("B", 12, 12), ("A", 3, 12)]),
    (15, (128,), [("B", 13, 13), ("A", 2, 12)]), (15, (256,), [("B", 13, 13), ("A", 2, 14)]), (20, (1,), [("B", 12, 12), ("A", 8, 12)]),
    (20, (8,), [("B", 13, 13), ("A", 7, 14)]), (21, (4,), [("B", 13, 13), ("A", 8, 14)]), (21, (8,), [("B", 13, 13), ("A", 8, 15)]),
    (22, (1,), [("B", 13, 13), ("A", 9, 13)]), (22, (2,), [("B", 13, 13), ("A", 9, 14)]), (22, (4,), [("B", 13, 13), ("A", 9, 15)]),
    (23, (1,), [("B", 14, 14), ("A", 9, 14)]), (23, (2,), [("B", 13, 13), ("A", 10, 15)]), (24, COLS, [("B", 14, 14), ("A", 10, 15)]),
    (25, COLS, [("B", 13, 13), ("A", 6, 14), ("A", 6, 14)]), (30, COLS, [("B", 13, 13), ("A", 9, 14), ("A", 8, 14)])], ids=str)
def test_pinned_plans(n, cols, want):
    """in-place transforms on 256 compute units, no knobs: the plans DESIGN.md 4.1 quotes, low -> high"""
    for n_cols in cols:
        assert _short(P.plan("interpolate", n, n_cols)) == want, n_cols
        assert _short(P.plan("evaluate", n, n_cols)) == want[::-1], n_cols


def test_invariants_reject_broken_plans():
    """check_invariants is not vacuous: single changes to good plans fail it"""
    n, n_cols = 25, 1024
    good = P.plan("interpolate", n, n_cols)
    check_invariants("interpolate", 0, n, n_cols, good)
    ps = good.passes
    fwd, oop = P.plan("evaluate", n, n_cols), P.plan("interpolate_to", n, n_cols)
    ext = P.plan("evaluate_extended", n, n_cols, ext=1)
    for entry, e, plan in (("evaluate", 0, fwd), ("interpolate_to", 0, oop), ("evaluate_extended", 1, ext)):
        check_invariants(entry, e, n, n_cols, plan)
    assert fwd.passes[-1].kind == "bottom_stream"
    broken = [
        ("interpolate", 0, n_cols, good._replace(passes=ps[:1] + ps[2:])),                                  # layers never transformed
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0], ps[2], ps[1]])),                            # out of order
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0], ps[1]._replace(k=5), ps[2]])),              # a layer left out
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0], ps[1], ps[1], ps[2]])),                     # layers transformed twice
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0]._replace(scale=True), ps[1], ps[2]])),       # scaled twice
        ("interpolate", 0, n_cols, good._replace(passes=ps[:2] + [ps[2]._replace(scale=False)])),           # never scaled
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0]._replace(k=15, logt=15)] + ps[1:])),         # a shape without a kernel
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0], ps[1]._replace(logt=15), ps[2]])),
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0]._replace(threads=2048)] + ps[1:])),
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0]._replace(lds=161 * 1024)] + ps[1:])),
        ("interpolate", 0, 1 << 20, good),                                                                  # work items past 32 bits
        ("interpolate", 0, n_cols, good._replace(passes=[ps[0]._replace(kind="bottom_stream")] + ps[1:])),  # a stream kernel on an inverse pass
        ("evaluate", 0, 1, fwd),                                                                            # ... on a column set inside the cache
        ("interpolate", 0, n_cols, oop), ("interpolate_to", 0, n_cols, good),                               # the second table read by the wrong entry
        ("interpolate_to", 0, n_cols, oop._replace(passes=[ps[0], oop.passes[0]] + ps[2:])),                # ... or not in the first pass
        ("evaluate_extended", 3, n_cols, ext), ("evaluate_extended", 1, n_cols, fwd),                       # an extension no kernel fuses
        ("evaluate", 0, n_cols, good._replace(route="fallback")),
    ]
    for entry, e, cols, plan in broken:
        with pytest.raises(AssertionError):
            check_invariants(entry, e, n, cols, plan)


def test_planner_under_address_and_undefined_sanitizers(tmp_path):
    """the header alone, in a program of its own: the largest accepted inputs, every refusal, and every knob at every size"""
    san = _compile(str(tmp_path / "cfft_plan_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    big = (1 << 64) - 1
    inputs = [(entry, ext, n, n_cols, n_cus, knobs) for (entry, ext), n, n_cols, n_cus, knobs
              in itertools.product(ENTRIES, (0, 1, 2, 3, 12, 13, 14, 20, 23, 24, 25, 30, 31, 32, 1000), (0, 1, 1024, (1 << 15) - 1, 1 << 15, 1 << 32, big),
                                   (1, 64, 256), KNOBS)]
    p = subprocess.run([san], input="".join(_line(*i) for i in inputs).encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(inputs)
    assert {ln for ln in lines if ln.startswith("error: ")} >= {
        "error: cfft: log_size out of range", "error: cfft: too many (tile, column) work items",
        "error: cfft: unsupported bottom pass", "error: cfft: unsupported pass shape", "error: cfft: more passes than a plan holds"}

"""The launch plan of tstwo_lookup_multiplicities_keyed (no GPU): lookup_keyed_plan of csrc/lookup_plan.h, compiled on its own
with the address and undefined-behaviour sanitisers (tests/lookup_keyed_plan_main.cpp, a plain executable), against
tests/lookup_keyed_plan.py over a matrix of inputs; the numpy model of the sums against the host functions it stands in for; what
the shapes of the -m gpu file reach; and the library's build for gfx950."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lookup_keyed_model as KM
import lookup_keyed_plan as KP
import lookup_plan as LP
from tstwo_amd import constraint_framework as F

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = 0x7F0000001000            # a 16-byte aligned device address


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("keyed_plan") / "lookup_keyed_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "..", "tstwo_amd", "csrc"), os.path.join(HERE, "lookup_keyed_plan_main.cpp"), "-o", exe])
    return exe


def _library_plans(exe, inputs):
    """One line of lookup_keyed_plan_main per input (log_range, order, groups)."""
    text = "".join(KP.input_line(*i) + "\n" for i in inputs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(inputs)
    return got


def _own(lg, order, groups):
    try:
        return KP.render(KP.plan(lg, groups, order))
    except KP.PlanError as e:
        return f"error: {e}"


def _group(rows, bits, offsets=None, weight=None):
    """weight: None, or the weight column's byte offset from a 16-byte boundary."""
    offsets = offsets or [0] * len(bits)
    return KP.Group([(BASE + 0x100000 * j + off, b) for j, (off, b) in enumerate(zip(offsets, bits))],
                    0 if weight is None else BASE + 0x900000 + weight, rows)


def test_keyed_plan_matches_the_library(plan_exe):
    """Both statements give the same branch, accumulator width, workgroup, grid, wrap point, vec bits and combining bound: a
    single group of every length around the unit, the workgroup and the wrap point, at every log_range, with and without a weight
    column, with each column in turn misaligned; and calls of 2, 5 and 64 groups, mixed ones included."""
    inputs = []
    for lg in range(1, KP.MAX_LOG + 1):
        for weighted in (False, True):
            w = KP.wrap(lg, "acc64" if weighted else "acc32")
            bits = KP.split_bits(lg, 1 + lg % 4)
            for n in (0, 1, 3, 4, 5, 255, 256, 257, w - 1, w, w + 1):
                for k in range(len(bits) + 2):          # k: which column is misaligned (the last two: the weight column, none)
                    offs = [4 * (1 + j % 3) if j == k else 0 for j in range(len(bits))]
                    wt = None if not weighted else 8 if k == len(bits) else 0
                    inputs.append((lg, lg & 1, [_group(n, bits, offs, wt)]))
        for n_groups in (2, 5, 64):
            for mix in ("none", "all", "some"):
                acc = "acc32" if mix == "none" else "acc64"
                w = KP.wrap(lg, acc, n_groups)
                threads = KP._shape(lg, acc, n_groups)[0]
                groups = []
                for g in range(n_groups):
                    rows = (w + 1, 0, 5, 4 * threads + 1, 3)[g % 5]
                    bits = KP.split_bits(lg, 1 + g % 4)
                    wt = None if mix == "none" or (mix == "some" and g != 1) else 4 * (g % 2)
                    groups.append(_group(rows, bits, [4 * ((g + j) % 4) * (g % 3 == 0) for j in range(len(bits))], wt))
                inputs.append((lg, 1, groups))
    got = _library_plans(plan_exe, inputs)
    seen = set()
    for (lg, order, groups), line in zip(inputs, got):
        assert line == _own(lg, order, groups), (lg, order, groups)
        p = KP.plan(lg, groups, order)
        seen.add((p.branch, p.acc))
        lens = [g.len for g in groups]
        # what any statement of the plan must satisfy: every unit of every group is some lane's, and the cap holds
        assert p.grid_x * p.grid_y <= max(LP.LDS_CAP if p.branch == "LDS" else LP.GLOBAL_CAP, p.grid_y)
        assert p.grid_x * p.threads * KP.UNIT <= p.wrap
        assert (p.grid_x == 0) == (sum(lens) == 0)
        for g, v in zip(groups, p.vec):
            assert not v or (g.len >= 4 and g.weight % 16 == 0 and all(a % 16 == 0 for a, _ in g.limbs))
        if max(lens) <= p.wrap:
            assert p.grid_x * p.threads * KP.UNIT >= max(lens)
        assert (p.acc == "acc64") == any(g.weight for g in groups)
        assert p.combine == KP.COMBINE[p.branch] == (8 if p.branch == "GLOBAL" else 0)
    assert seen == {(b, a) for b in ("LDS", "GLOBAL") for a in ("acc32", "acc64")}
    # the boundaries: a 64-bit histogram has half the bins of a 32-bit one in the same 64 KiB
    for acc, last in (("acc32", 14), ("acc64", 13)):
        wt = None if acc == "acc32" else 0
        assert KP.plan(last, [_group(1, (last,), None, wt)]).branch == "LDS"
        assert KP.plan(last + 1, [_group(1, (last + 1,), None, wt)]).branch == "GLOBAL"
    # one limb and no weight: the old entry's plan, whatever the input
    for lg in (1, 8, 14, 15, 28):
        for n in (0, 5, LP.wrap(lg) + 1):
            old, new = LP.plan(lg, [BASE + 4], [n]), KP.plan(lg, [_group(n, (lg,), [4])])
            assert (old.branch, old.threads, old.grid_x, old.grid_y, old.wrap, old.vec) == (new.branch, new.threads, new.grid_x, new.grid_y, new.wrap, new.vec)


def test_keyed_plan_rejections(plan_exe):
    """the inputs without a plan, each with its reason, from both statements"""
    big = KP.MAX_ROWS
    g8 = _group(8, (8,))
    cases = [(0, 1, [_group(8, (1,))], "log_range must be 1 to 28"), (29, 1, [_group(8, (28, 1))], "log_range must be 1 to 28"),
             (8, 1, [], "1 to 64 groups"), (8, 1, [g8] * 65, "1 to 64 groups"),
             (8, 2, [g8], "order must be 0 (natural) or 1 (coset)"),
             (8, 1, [_group(8, ())], "1 to 4 limbs per group"), (8, 1, [_group(8, (2, 2, 2, 1, 1))], "1 to 4 limbs per group"),
             (8, 1, [_group(8, (8, 0))], "every limb needs at least 1 bit"),
             (8, 1, [_group(8, (4, 3))], "the bits of every group must add up to log_range"),
             (8, 1, [g8, _group(8, (4, 5))], "the bits of every group must add up to log_range"),
             (8, 1, [_group(8, (2 ** 32 - 1, 9))], "the bits of every group must add up to log_range"),
             (8, 1, [KP.Group([(BASE, 4), (0, 4)], 0, 8)], "null device pointer among the limbs"),
             (8, 1, [_group(big + 1, (8,))], "more than 2^31 - 2 rows"), (8, 0, [_group(big, (8,)), _group(1, (4, 4))], "more than 2^31 - 2 rows"),
             (8, 1, [_group(big, (8,))], None), (28, 0, [_group(big - 1, (28,)), _group(1, (7, 7, 7, 7), None, 4)], None),
             (8, 1, [g8] * 64, None)]
    got = _library_plans(plan_exe, [c[:3] for c in cases])
    for (lg, order, groups, why), line in zip(cases, got):
        assert line == _own(lg, order, groups), (lg, order, groups)
        assert line == f"error: {why}" if why else not line.startswith("error")


@pytest.mark.parametrize("log_range", range(1, 11))
def test_model_matches_the_host_functions(log_range):
    """One limb, no weight: the model is np.bincount in natural order and F.range_check_multiplicities in coset order, and the
    old entry's model (tests/lookup_plan.py) with its rejected count; its positions are the framework's."""
    rng = np.random.default_rng(5200 + log_range)
    cols = [rng.integers(0, 1 << log_range, size=n) for n in (0, 1, 257, 4099)]
    groups = [([(c, log_range)], None) for c in cols]
    got, rejected = KM.multiplicities(log_range, groups, "coset")
    assert rejected == 0 and np.array_equal(got, F.range_check_multiplicities(log_range, *cols))
    got, rejected = KM.multiplicities(log_range, groups, "natural")
    assert rejected == 0 and np.array_equal(got, np.bincount(np.concatenate(cols), minlength=1 << log_range))
    assert np.array_equal(LP.coset_positions(log_range), F._coset_positions(log_range))
    outside = np.array([1 << log_range, LP.MAX_VALUES, 0], dtype=np.uint32)
    for order in ("natural", "coset"):
        a, ra = KM.multiplicities(log_range, groups + [([(outside, log_range)], None)], order)
        b, rb = LP.multiplicities(log_range, cols + [outside], order)
        assert ra == rb == 2 and np.array_equal(a, b)
    # weights: np.bincount(weights=) on small integers; a zero weight hides a limb outside the range, a non-zero one does not
    w = rng.integers(0, 3, size=4099).astype(np.uint32)
    got, rejected = KM.multiplicities(log_range, [([(cols[3], log_range)], w)], "natural")
    assert rejected == 0 and np.array_equal(got, np.bincount(cols[3], weights=w, minlength=1 << log_range).astype(np.uint32))
    got, rejected = KM.multiplicities(log_range, [([(outside, log_range)], np.array([0, 1, 5], dtype=np.uint32))], "natural")
    assert rejected == 1 and got[0] == 5 and got.sum() == 5
    # three rows of P - 1 in one bin: -3 mod P, which 32-bit accumulators get wrong
    got, _ = KM.multiplicities(log_range, [([(np.zeros(3, dtype=np.uint32), log_range)], np.full(3, KM.P - 1, dtype=np.uint32))], "natural")
    assert got[0] == KM.P - 3 and (3 * (KM.P - 1)) % 2 ** 32 % KM.P != KM.P - 3


def test_model_joins_limbs_after_checking_each():
    """a = 2^bits_a, b = 0 is rejected and the bin of (0, 1) stays empty; a row with two bad limbs is rejected once."""
    a, b = np.array([4, 0, 3, 9], dtype=np.uint32), np.array([0, 1, 2, 9], dtype=np.uint32)
    got, rejected = KM.multiplicities(5, [([(a, 2), (b, 3)], None)], "natural")
    assert rejected == 2 and got[4] == 1 and got[3 + 4 * 2] == 1 and got.sum() == 2


def test_gpu_shapes_reach_every_path():
    """The shapes tests/test_gpu_lookup_keyed.py runs reach, per branch and accumulator width: 16-byte units, a group read word
    by word, a partial last unit, an empty group, workgroups without work, and lanes that take a second unit; the wrap cases
    sit at the plan's own wrap point + 1029 rows with the number of groups that makes that point smallest."""
    reached = {}
    for name, (lg, shapes) in KP.gpu_shapes().items():
        groups = KP.shape_groups(shapes)
        where, got = KP.reaches(lg, groups)
        reached.setdefault(where, set()).update(got)
        if name.startswith("wrap"):
            p = KP.plan(lg, groups)
            assert "wrap" in got and len(groups) == KP.MAX_GROUPS and max(g.len for g in groups) == p.wrap + KP.WRAP_EXTRA, name
            assert p.wrap == min(KP.wrap(lg, p.acc, n) for n in range(1, KP.MAX_GROUPS + 1))
            assert p.wrap == (1 << 12 if p.branch == "LDS" else 1 << 15)
    assert set(reached) == {(b, a) for b in ("LDS", "GLOBAL") for a in ("acc32", "acc64")}
    for where, got in reached.items():
        assert got == {"vec", "scalar", "tail", "empty", "idle", "wrap"}, (where, sorted(got))
    # a mixed call (a NULL-weight group beside a weighted one) takes the 64-bit kernels
    for lg in (13, 14):
        assert KP.plan(lg, KP.shape_groups(KP.mixed_call(lg))).acc == "acc64"
    # within one group the columns have different alignments somewhere in the matrix
    assert any(len(set(s.offsets) | ({s.weight} if s.weight is not None else set())) > 1
               for _, shapes in KP.gpu_shapes().values() for s in shapes)
    assert set(KP.LENGTHS) >= {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097}


def test_library_builds_for_gfx950_with_the_keyed_entry():
    """python -m tstwo_amd.build cross-compiles without a GPU; the library exports the new symbol."""
    import ctypes as C
    from tstwo_amd import _lib as L
    from tstwo_amd import build
    lib = build.build()
    assert os.path.exists(lib)
    assert hasattr(C.CDLL(lib), "tstwo_lookup_multiplicities_keyed")
    assert "tstwo_lookup_multiplicities_keyed" in L.EXPORTS and C.sizeof(L.LookupGroup) == 72

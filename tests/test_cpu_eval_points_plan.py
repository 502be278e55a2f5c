"""The launch plan of tstwo_eval_at_points (no GPU): csrc/poly_eval_plan.h, compiled on its own with the address and undefined
behaviour sanitizers, against tests/eval_points_plan.py; what the shapes of the -m gpu file reach; and the resource usage of
the new kernels of csrc/poly_eval.hip, compiled for gfx950 without a device."""
import os
import re
import shutil
import subprocess

import pytest

import eval_points_plan as EP
from tstwo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")


def _library_lines(tmp_path, lines):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "eval_points_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "eval_points_plan_main.cpp"), "-o", exe])
    p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _own(lg, cols, points, aligned):
    try:
        return EP.render(EP.plan(lg, cols, points, aligned))
    except EP.PlanError as e:
        return f"error: {e}"


def test_eval_points_plan_matches_the_library(tmp_path):
    """Both statements give the same sweeps, tiles, levels, slabs and scratch for every log <= 31, the column counts around every
    switch, every point count and both alignments; the same reason for a group without a plan; and the same place for the
    results."""
    inputs = [(lg, c, k, a) for lg in range(EP.MAX_LOG + 1) for c in (1, 2, 3, 4, 15, 16, 63, 64, 65, 255, 256, 1100, EP.SLAB_COLS, EP.SLAB_COLS + 8)
              for k in range(1, EP.MAX_POINTS + 1) for a in (False, True)]
    rejected = [(5, 0, 1, True), (5, 1, 0, True), (5, 1, 17, True), (32, 1, 1, True)]
    results = [0, 1, 4095, 4096, 4097, 1 << 20]
    got = _library_lines(tmp_path, [f"{lg} {c} {k} {int(a)}" for lg, c, k, a in inputs + rejected] + [f"results {n}" for n in results])
    for args, line in zip(inputs + rejected, got):
        assert line == _own(*args), args
    assert got[len(inputs):len(inputs) + 4] == ["error: a group without columns", "error: 1 to 16 points per group", "error: 1 to 16 points per group",
                                                "error: log size out of range"]
    assert got[-len(results):] == [str(int(EP.result_pinned(n))) for n in results] == ["1", "1", "1", "1", "0", "0"]
    for lg, c, k, a in inputs:
        p = EP.plan(lg, c, k, a)
        # what any statement of the plan must satisfy
        assert p.chunks << p.chunk_log == max(1 << lg, 1 << p.chunk_log)            # the chunks tile the polynomial; a small one has one
        assert p.fast <= (a and lg >= p.chunk_log)                                 # 16-byte loads never leave the polynomial
        assert (p.sweeps - 1) * EP.MAX_K + p.k_last == k and 1 <= p.k_last <= EP.MAX_K
        assert p.levels == 1 + (p.chunks > 1) + (p.chunks > 4096) and p.groups1 * 4096 == max(p.chunks, 4096)
        assert p.groups1 <= 4096                                                   # a third level always ends the fold
        assert (p.slabs - 1) * EP.SLAB_COLS < c <= p.slabs * EP.SLAB_COLS and p.slab_cols * EP.MAX_K <= 32768     # grid y, y * z
        kmax = EP.MAX_K if p.sweeps > 1 else p.k_last
        need = p.slab_cols * kmax * (p.chunks + p.groups1) if p.levels == 3 else p.slab_cols * kmax * p.chunks if p.levels == 2 else 0
        assert p.scratch_qm31 == need


def test_three_levels_begin_at_log_27():
    """The plan has a three-level case below 2^28 words: 2^27 coefficients (4 groups per chunk there for any column count), which
    tests/test_gpu_eval_points.py runs for one column at 2 points."""
    first = min(lg for lg in range(EP.MAX_LOG + 1) if EP.plan(lg, 1, 2, True).levels == 3)
    assert first == EP.THREE_LEVEL_LOG == 27 and (1 << first) < (1 << 28)
    assert all(EP.plan(lg, c, 1, True).levels < 3 for lg in range(first) for c in (1, 64, 4096))


def test_gpu_shapes_reach_every_branch():
    """The coverage condition: the calls of tests/test_gpu_eval_points.py reach both load paths (and the short polynomial), both
    tile sizes, 1 / 2 / 3 levels, every K of a sweep, a split into several sweeps, the pointer table in device memory, several
    slabs, the constant polynomial, and the results in the page-locked page and in scratch."""
    reached = set()
    for name, groups in EP.gpu_calls().items():
        reached |= EP.branches([(lg, c, k, off == 0) for lg, c, k, off in groups])
    assert EP.reachable_branches() == EP.ALL_BRANCHES
    assert reached == EP.ALL_BRANCHES, sorted(EP.ALL_BRANCHES - reached)
    # the switch points for one column, and the 4-group tile at the size the issue names for a 256-CU device
    one = {lg: EP.plan(lg, 1, 1, True) for lg in range(EP.MAX_LOG + 1)}
    assert min(lg for lg, p in one.items() if p.fast) == 12 and min(lg for lg, p in one.items() if p.levels == 2) == 13
    assert {11, 12, 13, 14} <= set(EP.ONE_GROUP_LOGS)
    assert EP.plan(16, 64, 2, True).g == 4 and EP.plan(16, 63, 2, True).g == 1
    # the second of two calls of the sequence test needs more scratch than the first
    assert EP.call_scratch_qm31([(13, 2, 2, True)]) < EP.call_scratch_qm31([(14, 3, 4, True)])


def test_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """csrc/poly_eval.hip compiles for gfx950 without a device; every instantiation of the K-point kernels (2 load paths x 2 tile
    sizes x K = 1..4, and the fold for K = 1..4) reports no scratch, and at least 4 waves per SIMD."""
    p = subprocess.run([B._hipcc(), *B.FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "poly_eval.hip"), "-o", str(tmp_path / "poly_eval.o")], capture_output=True, text=True)
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
    new = {k: u for k, u in usage.items() if "k_eval_coeffs_pts" in k or "k_eval_partials_pts" in k}
    assert len(new) == 2 * 2 * EP.MAX_K + EP.MAX_K, sorted(new)
    for k, u in sorted(new.items()):
        print(k, "VGPRs", u["VGPRs"], "SGPRs", u["TotalSGPRs"], "occupancy", u["Occupancy [waves/SIMD]"], "scratch", u["ScratchSize [bytes/lane]"])
        assert u["ScratchSize [bytes/lane]"] == "0", (k, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= 4, (k, u)
    # the one-point kernels next to them did not change their footing either
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == "0", (k, u)

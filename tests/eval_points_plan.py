"""The launch plan of tstwo_eval_at_points restated in Python (csrc/poly_eval_plan.h is the statement the library runs;
tests/test_cpu_eval_points_plan.py compiles that header and compares), the branches a call reaches, and the shapes
tests/test_gpu_eval_points.py runs.  Plain Python: nothing here touches a GPU or imports the package under test."""
from __future__ import annotations

from collections import namedtuple

MAX_POINTS, MAX_K, MAX_LOG = 16, 4, 31
MIN_WORKGROUPS = 256            # the CU count of an MI355X, as a constant
SLAB_COLS = 8192
PINNED_BYTES = 64 * 1024

Plan = namedtuple("Plan", "sweeps k_full k_last g chunk_log fast chunks groups1 levels slabs slab_cols scratch_qm31")


class PlanError(ValueError):
    pass


def plan(log: int, cols: int, points: int, aligned: bool) -> Plan:
    """One group: `cols` columns of 2^log coefficients at `points` points."""
    if cols == 0:
        raise PlanError("a group without columns")
    if not 1 <= points <= MAX_POINTS:
        raise PlanError("1 to 16 points per group")
    if log > MAX_LOG:
        raise PlanError("log size out of range")
    sweeps = -(-points // MAX_K)
    k_full = MAX_K if sweeps > 1 else 0
    k_last = points - (sweeps - 1) * MAX_K
    wide = log >= 14 and (cols << (log - 14)) >= MIN_WORKGROUPS
    g, chunk_log = (4, 14) if wide else (1, 12)
    fast = aligned and log >= chunk_log
    chunks = 1 << (log - chunk_log) if log > chunk_log else 1
    groups1 = chunks // 4096 if chunks > 4096 else 1
    levels = 1 if chunks == 1 else 2 if chunks <= 4096 else 3
    slabs = -(-cols // SLAB_COLS)
    slab_cols = min(cols, SLAB_COLS)
    kmax = MAX_K if sweeps > 1 else k_last
    scratch = 0 if levels == 1 else slab_cols * kmax * (chunks + (groups1 if levels == 3 else 0))
    return Plan(sweeps, k_full, k_last, g, chunk_log, fast, chunks, groups1, levels, slabs, slab_cols, scratch)


def render(p: Plan) -> str:
    return " ".join(str(int(v)) for v in p)


def result_pinned(results: int) -> bool:
    """The results of a call (one QM31 per (group, column, point)) fit the page-locked page."""
    return 16 * results <= PINNED_BYTES


def call_scratch_qm31(groups) -> int:
    """QM31 slots one call takes for [(log, cols, points, aligned)]: the largest group's partials, then the results unless pinned."""
    results = sum(c * k for _, c, k, _ in groups)
    return max(plan(*g).scratch_qm31 for g in groups) + (0 if result_pinned(results) else results)


def branches(groups) -> set:
    """What one call over [(log, cols, points, aligned)] reaches."""
    out = set()
    for log, cols, points, aligned in groups:
        p = plan(log, cols, points, aligned)
        out.add("load:fast" if p.fast else "load:small" if log < p.chunk_log else "load:unaligned")
        out.add(f"g{p.g}")
        out.add(f"levels:{p.levels}")
        out.add(f"k{p.k_last}")
        if p.sweeps > 1:
            out |= {f"k{p.k_full}", "sweeps:several"}
        if cols > 64:
            out.add("table")
        if p.slabs > 1:
            out.add("slabs:several")
        if log == 0:
            out.add("log0")
    out.add("result:pinned" if result_pinned(sum(c * k for _, c, k, _ in groups)) else "result:scratch")
    if len(groups) > 1:
        out.add("groups:several")
    return out


ALL_BRANCHES = {"load:fast", "load:small", "load:unaligned", "g1", "g4", "levels:1", "levels:2", "levels:3", "k1", "k2", "k3", "k4",
                "sweeps:several", "table", "slabs:several", "log0", "result:pinned", "result:scratch", "groups:several"}

ONE_GROUP_LOGS = (0, 1, 2, 5, 11, 12, 13, 14, 16)
THREE_LEVEL_LOG = 27            # the smallest size with three levels: 2^27 words, below 2^28 (test_three_levels_begin_at_log_27)
MIXED_CALL = [(6, 3, 1, 0), (13, 2, 3, 0), (0, 2, 2, 0), (12, 70, 2, 0)]


def one_group_shapes():
    """(log, cols, points): the aligned one-group calls of tests/test_gpu_eval_points.py.  12 is the guarded / fast boundary, 13
    the first two-level size, 5 points two sweeps; 3 and 16 points at a one-level and a two-level size."""
    out = [(lg, c, k) for lg in ONE_GROUP_LOGS for c in (1, 3) for k in (1, 2, 4, 5)]
    out += [(lg, c, k) for lg in (5, 13) for c in (1, 3) for k in (3, 16)]
    return out


def gpu_calls():
    """{name: [(log, cols, points, byte offset of the columns from a 16-byte boundary)]}: every call shape of the GPU file."""
    calls = {f"one-{lg}-{c}x{k}": [(lg, c, k, 0)] for lg, c, k in one_group_shapes()}
    calls["g4"] = [(16, 64, 2, 0)]
    calls["three-levels"] = [(THREE_LEVEL_LOG, 1, 2, 0)]
    calls["unaligned-5"] = [(5, 2, 2, 4)]
    calls["unaligned-13"] = [(13, 2, 2, 4)]
    calls["one-unaligned-among-aligned"] = [(13, 3, 2, 4)]
    calls["mixed"] = list(MIXED_CALL)
    calls["result-in-scratch"] = [(5, 1100, 4, 0)]
    calls["slabs"] = [(0, SLAB_COLS + 8, 1, 0)]
    return calls


def reachable_branches() -> set:
    out = set()
    for lg in range(MAX_LOG + 1):
        for cols in (1, 2, 64, 65, 1100, SLAB_COLS + 8):
            for points in (1, 2, 3, 4, 5, 16):
                for aligned in (False, True):
                    out |= branches([(lg, cols, points, aligned)])
    return out | {"groups:several"}

"""The launch plan of tstwo_mle_eval_at_point_base / _secure restated in Python (csrc/mle_eval_plan.h is the statement the
library runs; tests/test_cpu_mle_eval_plan.py compiles that header and compares), the branches a plan reaches, and the shapes
tests/test_gpu_mle_eval.py runs.  Plain Python: nothing here touches a GPU or imports the package under test."""
from __future__ import annotations

from collections import namedtuple

MAX_LOG, MAX_MLES = 28, 32768
GROUP_LOG = 12                  # 256 lanes x 16 values
MIN_WORKGROUPS = 256
FOLD_BLOCK = 256                # partials per block of pass 2
MAX_GPU_VALUES = 1 << 22        # no GPU test evaluates more values than this in one call

Plan = namedtuple("Plan", "groups chunk_log fast chunks grid_y passes blocks scratch_qm31")


class PlanError(ValueError):
    pass


def plan(log_n: int, n_mles: int, is_secure: bool, aligned: bool) -> Plan:
    if n_mles == 0:
        raise PlanError("no MLE given")
    if n_mles > MAX_MLES:
        raise PlanError("more than 32768 MLEs in one call")
    if log_n > MAX_LOG:
        raise PlanError("more than 28 variables")
    wide = (not is_secure) and log_n >= GROUP_LOG + 2 and (n_mles << (log_n - GROUP_LOG - 2)) >= MIN_WORKGROUPS
    groups = 4 if (is_secure or wide) else 1
    chunk_log = GROUP_LOG + (2 if wide else 0)
    fast = aligned and log_n >= chunk_log
    chunks = 1 << (log_n - chunk_log) if log_n > chunk_log else 1
    passes = 2 if chunks > 1 else 1
    blocks = -(-chunks // FOLD_BLOCK) if chunks > 1 else 0
    return Plan(groups, chunk_log, fast, chunks, n_mles, passes, blocks, n_mles * ((chunks if chunks > 1 else 0) + 1))


def render(p: Plan) -> str:
    return f"{p.groups} {p.chunk_log} {int(p.fast)} {p.chunks} {p.grid_y} {p.passes} {p.blocks} {p.scratch_qm31}"


def branches(log_n: int, n_mles: int, is_secure: bool, aligned: bool) -> set:
    """What one call reaches: which pass-1 kernel on which load path ("small": the MLE is shorter than a chunk, so the clamped
    loads; "unaligned": word loads over whole chunks), and how pass 2 runs (not at all, one partly filled block, one full block,
    several blocks); "table": more than 64 column pointers, which travel through the device table."""
    p = plan(log_n, n_mles, is_secure, aligned)
    kind = "secure" if is_secure else f"base{p.groups}"
    path = "fast" if p.fast else ("small" if log_n < p.chunk_log else "unaligned")
    fold = "none" if p.passes == 1 else "part" if p.chunks < FOLD_BLOCK else "full" if p.chunks == FOLD_BLOCK else "multi"
    out = {f"{kind}:{path}", f"fold:{fold}"}
    if n_mles * (4 if is_secure else 1) > 64:
        out.add("table")
    return out


def gpu_shapes():
    """{name: (log_n, n_mles, is_secure, byte offset of the columns from a 16-byte boundary)}: the calls of the parametrised
    tests of tests/test_gpu_mle_eval.py.  log 0..14 cover the empty point, a single lane, the partial chunk and the first
    two-pass size with its neighbours; 19..22 straddle the plan's two switch points for one MLE (pass 2 goes from one block to
    several at 2^20 -> 2^21 values of a base MLE, and pass 1 from 1 group to 4 at 2^21 -> 2^22)."""
    shapes = {}
    for secure in (False, True):
        k = "secure" if secure else "base"
        for lg in list(range(0, 15)) + [19, 20, 21, 22]:
            shapes[f"{k}-{lg}"] = (lg, 1, secure, 0)
        shapes[f"{k}-3x9"] = (9, 3, secure, 0)
        big = 18 if secure else 20
        shapes[f"{k}-3x{big}"] = (big, 3, secure, 0)
        shapes[f"{k}-65x6"] = (6, 65, secure, 0)
        shapes[f"{k}-unaligned-5"] = (5, 2, secure, 4)
        shapes[f"{k}-unaligned-13"] = (13, 2, secure, 12)
    shapes["base-128x15"] = (15, 128, False, 0)             # 4 groups and a partly filled fold block; 128 pointers
    shapes["base-4x20"] = (20, 4, False, 0)                 # the fewest MLEs of 2^20 that take 4 groups
    shapes["base-unaligned-22"] = (22, 1, False, 8)         # 4 groups on the word loads
    return shapes


def reachable_branches() -> set:
    """Every branch some call can reach (all sizes, 1 to 65 MLEs and beyond the pointer table's 64)."""
    out = set()
    for lg in range(MAX_LOG + 1):
        for n in (1, 2, 64, 65, 4096):
            for secure in (False, True):
                for aligned in (False, True):
                    out |= branches(lg, n, secure, aligned)
    return out

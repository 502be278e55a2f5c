"""The tests' own statement of tstwo_lookup_multiplicities (no GPU, no library): the launch plan of csrc/lookup_plan.h, a numpy
model of the counts, and the shapes the -m gpu file (tests/test_gpu_lookup.py) runs, with which parts of the kernels each reaches.

Plan.  One launch, the column on the grid's y axis.  A lane takes UNITS of 4 consecutive words, one per step, grid_x * threads
units apart: a 16-byte load where the column is 16-byte aligned and has a whole unit (its `vec` bit) and the unit is whole, single
words for the last partial unit and for every unit of a column without the bit.  Tables up to 2^14 bins are counted in LDS by
workgroups of 1024 lanes, at most 64 of them; larger ones with one global atomic per value by workgroups of 256, at most 2048.
The columns of a call share the cap.  `wrap` is the number of values of ONE column that one pass of a capped grid covers: a
column longer than that makes lanes take a second unit."""
from collections import namedtuple

import numpy as np

MAX_COLS, MAX_LOG, MAX_VALUES = 64, 28, 2 ** 31 - 2
UNIT = 4
LDS_MAX_LOG, LDS_THREADS, LDS_CAP = 14, 1024, 64
GLOBAL_THREADS, GLOBAL_CAP = 256, 2048
ORDERS = {"natural": 0, "coset": 1}

Plan = namedtuple("Plan", "branch threads grid_x grid_y wrap vec")       # vec: one bool per column


class PlanError(ValueError):
    pass


def branch(log_range):
    return "LDS" if log_range <= LDS_MAX_LOG else "GLOBAL"


def _shape(log_range, n_cols):
    threads, cap = (LDS_THREADS, LDS_CAP) if branch(log_range) == "LDS" else (GLOBAL_THREADS, GLOBAL_CAP)
    return threads, max(1, cap // n_cols)


def wrap(log_range, n_cols=1):
    threads, cap_x = _shape(log_range, n_cols)
    return cap_x * threads * UNIT


def plan(log_range, addrs, lens, order=1):
    """addrs: the columns' byte addresses (only their value mod 16 matters), lens: their lengths in words."""
    n_cols = len(lens)
    if not 1 <= log_range <= MAX_LOG:
        raise PlanError("log_range must be 1 to 28")
    if not 1 <= n_cols <= MAX_COLS:
        raise PlanError("1 to 64 columns")
    if order not in (0, 1):
        raise PlanError("order must be 0 (natural) or 1 (coset)")
    if any(n > MAX_VALUES for n in lens) or sum(lens) > MAX_VALUES:
        raise PlanError("more than 2^31 - 2 values")
    threads, cap_x = _shape(log_range, n_cols)
    units = max(-(-n // UNIT) for n in lens)
    grid_x = min(-(-units // threads), cap_x)
    return Plan(branch(log_range), threads, grid_x, n_cols, cap_x * threads * UNIT, tuple(a % 16 == 0 and n >= UNIT for a, n in zip(addrs, lens)))


def render(p):
    """The line tests/lookup_plan_main.cpp prints for a plan."""
    return f"{p.branch} {p.threads} {p.grid_x} {p.grid_y} {p.wrap} {sum(1 << c for c, v in enumerate(p.vec) if v):x}"


def reaches(log_range, addrs, lens):
    """Which parts of the kernels a call runs: the branch, 16-byte units ("vec"), a column read word by word ("scalar"), the partial
    last unit of a vec column ("tail"), a column without words ("empty"), lanes that take a second unit ("wrap"), and workgroups
    that leave at once because their column is shorter than the longest ("idle")."""
    p = plan(log_range, addrs, lens)
    got = {p.branch}
    for v, n in zip(p.vec, lens):
        units = -(-n // UNIT)
        got |= {"vec"} if v else {"scalar"} if n else set()
        if v and n % UNIT:
            got.add("tail")
        if n == 0:
            got.add("empty")
        if units > p.grid_x * p.threads:
            got.add("wrap")
        if units <= (p.grid_x - 1) * p.threads:
            got.add("idle")
    return got


# ------------------------------------------------------------------ the counts
def coset_positions(log_size):
    """Storage position of coset row k: 2 rev(k >> 1) for even k, 2 (2^(log_size-1) - 1 - rev(k >> 1)) + 1 for odd k (rev over
    log_size - 1 bits)."""
    bits = log_size - 1
    k = np.arange(1 << log_size, dtype=np.int64)
    j, r = k >> 1, np.zeros(1 << log_size, dtype=np.int64)
    for b in range(bits):
        r |= ((j >> b) & 1) << (bits - 1 - b)
    return np.where(k & 1, 2 * ((1 << bits) - 1 - r) + 1, 2 * r)


def place(log_range, order):
    return coset_positions(log_range) if ORDERS.get(order, order) == 1 else np.arange(1 << log_range, dtype=np.int64)


def multiplicities(log_range, cols, order):
    """(the column tstwo_lookup_multiplicities writes, the number of words >= 2^log_range it leaves out)."""
    n = 1 << log_range
    counts, rejected = np.zeros(n, dtype=np.int64), 0
    for c in cols:
        c = np.asarray(c).astype(np.int64)
        ok = (c >= 0) & (c < n)
        rejected += int(c.size - ok.sum())
        counts += np.bincount(c[ok], minlength=n)
    assert counts.sum() <= MAX_VALUES
    out = np.empty(n, dtype=np.uint32)
    out[place(log_range, order)] = counts
    return out, rejected


# ------------------------------------------------------------------ the shapes of tests/test_gpu_lookup.py
LAST_LDS_LOG, FIRST_GLOBAL_LOG = LDS_MAX_LOG, LDS_MAX_LOG + 1
PARITY_LOGS = (1, 2, 8, LAST_LDS_LOG, FIRST_GLOBAL_LOG, 16)
# (length in words, words between a 16-byte boundary and the column's first word)
PARITY_COLUMNS = {
    "1col": [(4099, 0)],
    "2cols": [(255, 0), (257, 1)],
    "5cols": [(0, 0), (1, 0), (255, 0), (257, 1), (4099, 0)],
}
WRAP_EXTRA = 1029                                            # a whole unit row, whole units and a partial one past the wrap
WRAP_CASES = {b: (lg, [(wrap(lg) + WRAP_EXTRA, 0)]) for b, lg in (("LDS", LAST_LDS_LOG), ("GLOBAL", FIRST_GLOBAL_LOG))}


def gpu_shapes():
    """{name: (log_range, [(len, offset words)])}: every call shape of the parity and grid-stride tests."""
    shapes = {f"{name}@{lg}": (lg, cols) for lg in PARITY_LOGS for name, cols in PARITY_COLUMNS.items()}
    shapes.update({f"wrap-{b}": case for b, case in WRAP_CASES.items()})
    return shapes

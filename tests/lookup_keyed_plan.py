"""The tests' own statement of the launch plan of tstwo_lookup_multiplicities_keyed (no GPU, no library): lookup_keyed_plan of
csrc/lookup_plan.h, and the shapes the -m gpu file (tests/test_gpu_lookup_keyed.py) runs, with the parts of the kernels each reaches.

Plan.  One launch, the GROUP on the grid's y axis.  A lane takes units of 4 consecutive rows, grid_x * threads units apart: 16-byte
loads where every column of the group (the limbs in use and the weight column, if any) is 16-byte aligned and the group has a
whole unit (the group's `vec` bit) and the unit is whole, single words otherwise.  A call without any weight column counts in
32-bit words (acc32) and stays in LDS up to 2^14 bins; a call with a weight column accumulates in 64 bits (acc64: a scratch and a
reducing kernel) and stays in LDS up to 2^13 bins.  Workgroups, caps and the wrap point are those of tests/lookup_plan.py, the cap
shared by the groups.  combine: rounds of peeling equal keys off a wave before it adds, 8 on the global branch, 0 in LDS."""
from collections import namedtuple

import lookup_plan as LP

MAX_GROUPS, MAX_LIMBS = 64, 4
MAX_LOG, MAX_ROWS, UNIT = LP.MAX_LOG, LP.MAX_VALUES, LP.UNIT
LDS_MAX_LOG = {"acc32": 14, "acc64": 13}
COMBINE = {"LDS": 0, "GLOBAL": 8}

Group = namedtuple("Group", "limbs weight len")          # limbs: [(byte address, bits)], weight: byte address or 0 (none)
Plan = namedtuple("Plan", "branch acc threads grid_x grid_y wrap vec combine")       # vec: one bool per group


class PlanError(ValueError):
    pass


def branch(log_range, acc):
    return "LDS" if log_range <= LDS_MAX_LOG[acc] else "GLOBAL"


def _shape(log_range, acc, n_groups):
    threads, cap = (LP.LDS_THREADS, LP.LDS_CAP) if branch(log_range, acc) == "LDS" else (LP.GLOBAL_THREADS, LP.GLOBAL_CAP)
    return threads, max(1, cap // n_groups)


def wrap(log_range, acc, n_groups=1):
    threads, cap_x = _shape(log_range, acc, n_groups)
    return cap_x * threads * UNIT


def plan(log_range, groups, order=1):
    if not 1 <= log_range <= MAX_LOG:
        raise PlanError("log_range must be 1 to 28")
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise PlanError("1 to 64 groups")
    if order not in (0, 1):
        raise PlanError("order must be 0 (natural) or 1 (coset)")
    total, vec = 0, []
    for g in groups:
        if not 1 <= len(g.limbs) <= MAX_LIMBS:
            raise PlanError("1 to 4 limbs per group")
        for addr, bits in g.limbs:
            if bits < 1:
                raise PlanError("every limb needs at least 1 bit")
            if not addr:
                raise PlanError("null device pointer among the limbs")
        if sum(b for _, b in g.limbs) != log_range:
            raise PlanError("the bits of every group must add up to log_range")
        if g.len > MAX_ROWS:
            raise PlanError("more than 2^31 - 2 rows")
        total += g.len
        vec.append(g.len >= UNIT and g.weight % 16 == 0 and all(a % 16 == 0 for a, _ in g.limbs))
    if total > MAX_ROWS:
        raise PlanError("more than 2^31 - 2 rows")
    acc = "acc64" if any(g.weight for g in groups) else "acc32"
    threads, cap_x = _shape(log_range, acc, len(groups))
    units = max(-(-g.len // UNIT) for g in groups)
    b = branch(log_range, acc)
    return Plan(b, acc, threads, min(-(-units // threads), cap_x), len(groups), cap_x * threads * UNIT, tuple(vec), COMBINE[b])


def render(p):
    """The line tests/lookup_keyed_plan_main.cpp prints for a plan."""
    return f"{p.branch} {p.acc} {p.threads} {p.grid_x} {p.grid_y} {p.wrap} {sum(1 << g for g, v in enumerate(p.vec) if v):x} {p.combine}"


def input_line(log_range, order, groups):
    """The line tests/lookup_keyed_plan_main.cpp reads for a call."""
    parts = [f"{log_range} {order} {len(groups)}"]
    for g in groups:
        parts.append(f"{len(g.limbs)} {g.weight} {g.len} " + " ".join(f"{a} {b}" for a, b in g.limbs))
    return " ".join(parts)


def reaches(log_range, groups):
    """Which parts of the kernels a call runs, as in tests/lookup_plan.py::reaches: 16-byte units ("vec"), a group read word by
    word ("scalar"), the partial last unit of a vec group ("tail"), a group without rows ("empty"), lanes that take a second unit
    ("wrap"), and workgroups that leave at once because their group is shorter than the longest ("idle")."""
    p = plan(log_range, groups)
    got = set()
    for v, g in zip(p.vec, groups):
        units = -(-g.len // UNIT)
        got |= {"vec"} if v else {"scalar"} if g.len else set()
        if v and g.len % UNIT:
            got.add("tail")
        if g.len == 0:
            got.add("empty")
        if units > p.grid_x * p.threads:
            got.add("wrap")
        if units <= (p.grid_x - 1) * p.threads:
            got.add("idle")
    return (p.branch, p.acc), got


# ------------------------------------------------------------------ the shapes of tests/test_gpu_lookup_keyed.py
# A shape is (log_range, [GroupShape]): GroupShape = (rows, (bits per limb), (offset words of each limb column past a 16-byte
# boundary), weight: None or the offset words of the weight column).  The GPU file places the columns accordingly and draws the
# values; here only lengths, widths and alignments matter.
GroupShape = namedtuple("GroupShape", "rows bits offsets weight")

LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
# (log_range, weighted): 1 and 2, then either side of the LDS / GLOBAL boundary of each accumulator width
TABLES = [(1, False), (2, False), (LDS_MAX_LOG["acc32"], False), (LDS_MAX_LOG["acc32"] + 1, False),
          (1, True), (2, True), (LDS_MAX_LOG["acc64"], True), (LDS_MAX_LOG["acc64"] + 1, True)]
WRAP_EXTRA = 1029


def split_bits(log_range, n_limbs):
    """log_range as up to n_limbs widths, unequal where the table is large enough: (what is left, 2, 3, 4), else (.., 1, 1)."""
    n = min(n_limbs, log_range)
    rest = [j + 1 for j in range(1, n)]
    if sum(rest) >= log_range:
        rest = [1] * (n - 1)
    return (log_range - sum(rest), *rest)


def group_shape(rows, log_range, n_limbs, weighted, g):
    """Group g of a call: limb j starts (g + j) % 4 words past a 16-byte boundary, the weight column (g + 2) % 4 words, so the
    columns of one group have different alignments; every fourth group (g % 4 == 0, limbs at 0, 1, 2, 3) is misaligned as soon as
    it has two limbs.  aligned_shape() below is the group whose columns are all aligned."""
    bits = split_bits(log_range, n_limbs)
    return GroupShape(rows, bits, tuple((g + j) % 4 for j in range(len(bits))), (g + 2) % 4 if weighted else None)


def aligned_shape(rows, log_range, n_limbs, weighted):
    bits = split_bits(log_range, n_limbs)
    return GroupShape(rows, bits, (0,) * len(bits), 0 if weighted else None)


def parity_calls(log_range, weighted):
    """The calls of one (log_range, weighted) parity case: every length as a single aligned group and as a single misaligned
    one, two groups, and 64 groups whose lengths run through LENGTHS (with 1 to 4 limbs in turn)."""
    calls = {}
    for n in LENGTHS:
        calls[f"1group-aligned-{n}"] = [aligned_shape(n, log_range, 1 + n % 4, weighted)]
        calls[f"1group-offset-{n}"] = [group_shape(n, log_range, 1 + n % 4, weighted, 1 + n % 3)]
    calls["2groups"] = [aligned_shape(4097, log_range, 2, weighted), group_shape(255, log_range, 3, weighted, 1)]
    calls["64groups"] = [aligned_shape(LENGTHS[g % len(LENGTHS)], log_range, 1 + g % 4, weighted) if g % 2 else
                         group_shape(LENGTHS[g % len(LENGTHS)], log_range, 1 + g % 4, weighted, g) for g in range(64)]
    return calls


def wrap_call(log_range, weighted):
    """64 groups, which make the wrap point smallest (2^12 rows in LDS, 2^15 on the global branch): one aligned group of
    wrap + 1029 rows, the others short."""
    acc = "acc64" if weighted else "acc32"
    w = wrap(log_range, acc, 64)
    return [aligned_shape(w + WRAP_EXTRA, log_range, 2, weighted)] + [group_shape((0, 5, 64, 257)[g % 4], log_range, 1 + g % 4, weighted, g)
                                                                       for g in range(1, 64)]


def mixed_call(log_range):
    """A NULL-weight group and a weighted group in one call."""
    return [aligned_shape(1025, log_range, 2, False), group_shape(257, log_range, 1, True, 1)]


def shape_groups(shapes):
    """Plan-level groups of a call of GroupShapes, at the addresses the GPU file gives them."""
    base = 0x7F0000001000
    groups = []
    for s in shapes:
        limbs = [(base + 4 * off, b) for off, b in zip(s.offsets, s.bits)]
        groups.append(Group(limbs, 0 if s.weight is None else base + 4 * s.weight, s.rows))
    return groups


def gpu_shapes():
    """{name: (log_range, [GroupShape])}: every call shape of the parity and grid-stride tests."""
    shapes = {}
    for lg, weighted in TABLES:
        for name, call in parity_calls(lg, weighted).items():
            shapes[f"{name}@{lg}{'w' if weighted else ''}"] = (lg, call)
    for lg, weighted in TABLES[2:4] + TABLES[6:8]:
        shapes[f"wrap@{lg}{'w' if weighted else ''}"] = (lg, wrap_call(lg, weighted))
    return shapes

"""The tests' own statement of the schedule of tstwo_fri_commit_layers (no GPU, no library): which steps a commit over circle
columns of log sizes `col_logs`, down to a last layer of 2^last rows, takes, and which layer, column and alpha entries each touches.

Line layer i has log size col_logs[0] - 1 - i; layer L = col_logs[0] - 1 - last is the last one.  Alpha entry 0 is drawn behind the
first-layer tree, entry i + 1 behind layer i's tree; the fold INTO layer i reads entry i.  A column of log c joins the layer of log
c - 1.  The tail launch takes over at layer T, the first layer of at most 2^9 rows by which every column has joined, if T < L.

csrc/fri_plan.h is the library's statement, a loop over the layers; this one says per layer how it is produced and committed.
tests/test_cpu_fri_plan.py compares the two."""
from collections import namedtuple

TAIL_LOG = 9

Step = namedtuple("Step", "kind layer log column alpha_in alpha_out n_layers pre")
KINDS = ("FIRST_TREE", "CIRCLE_WRITE", "COMMIT", "FOLD_COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "TAIL")


def _step(kind, layer, log, column=0, alpha_in=0, alpha_out=0, n_layers=0, pre=False):
    return Step(kind, layer, log, column, alpha_in, alpha_out, n_layers, pre)


class PlanError(Exception):
    pass


def plan(col_logs, last):
    """The ordered steps, or PlanError(reason)."""
    if not col_logs:
        raise PlanError("no columns")
    for i, c in enumerate(col_logs):
        if not 3 <= c <= 31:
            raise PlanError("fri commit: circle evaluations of log size 3..31")
        if i and col_logs[i - 1] <= c:
            raise PlanError("column sizes not decreasing")
    first_log = col_logs[0] - 1
    if last > first_log:
        raise PlanError("fri commit: last layer larger than the first line layer")
    if any(c - 1 < last for c in col_logs):
        raise PlanError("not all columns were consumed")            # a column below the last layer meets no layer
    L = first_log - last
    log = lambda i: first_log - i
    joins = {first_log - (c - 1): j for j, c in enumerate(col_logs) if j}          # layer -> the column that joins it
    last_join = max(joins, default=0)
    T = next((i for i in range(L) if log(i) <= TAIL_LOG and i >= last_join), L)     # no tail: as if it began at the last layer
    # how layer i >= 1 comes to be: inside the tail, fused into its own tree's leaf launch, or by a plain fold (+ its column)
    pre = 1 <= T < L and T not in joins
    fused = {i for i in range(1, T) if i not in joins}
    steps = [_step("FIRST_TREE", 0, col_logs[0], alpha_out=0), _step("CIRCLE_WRITE", 0, first_log, column=0, alpha_in=0)]
    for i in range(T):                                  # layers committed by launches of their own
        if i not in fused:
            steps.append(_step("COMMIT", i, log(i), alpha_out=i + 1))
        nxt = i + 1
        if nxt in fused:
            steps.append(_step("FOLD_COMMIT", nxt, log(nxt), alpha_in=nxt, alpha_out=nxt + 1))
        elif not (nxt == T and pre):
            steps.append(_step("FOLD_LINE", nxt, log(nxt), alpha_in=nxt))
        if nxt in joins:
            steps.append(_step("CIRCLE_ACCUM", nxt, log(nxt), column=joins[nxt], alpha_in=nxt))
    if T < L:
        steps.append(_step("TAIL", T, log(T), alpha_in=T if pre else 0, alpha_out=T + 1, n_layers=L - T, pre=pre))
    return steps


def kinds(col_logs, last):
    """The set of step kinds of a plan; TAIL as "TAIL+pre" or "TAIL"."""
    return {("TAIL+pre" if s.pre else "TAIL") if s.kind == "TAIL" else s.kind for s in plan(col_logs, last)}


def render(steps):
    """One line per plan, as tests/fri_plan_main.cpp prints the library's."""
    return " ".join(f"{s.kind}:{s.layer}:{s.log}:{s.column}:{s.alpha_in}:{s.alpha_out}:{s.n_layers}:{int(s.pre)}" for s in steps)

"""The evals of tests/test_cpu_interaction_trace.py and tests/test_gpu_interaction_trace.py, each written twice: as
`evaluate(eval)` for the package, and as a plain numpy function of the columns and a neighbour function (the twin), so that what
the package derives from `evaluate` is compared with something that is not its own output.

A twin returns the relation entries [(multiplicity, [values])] with numpy uint64 columns or ints; model_fracs turns them into
the fractions of tests/columns_model.py interaction_trace with tests/logup_model.py combine_cols.
"""
from __future__ import annotations

import numpy as np

import air_program_model as X
import columns_model as CM
import logup_model as LM
from tstwo_amd.air import ORIGINAL_TRACE_IDX
from tstwo_amd.fields import QM31
from tstwo_amd.logup import LookupElements, RelationEntry

P = LM.P
Z, ALPHA = (3, 4, 5, 6), (7, 8, 9, 10)


def elements(size=3) -> LookupElements:
    return LookupElements(QM31.from_u32_unchecked(*Z), QM31.from_u32_unchecked(*ALPHA), size)


class GeneralEval:
    """Main columns a, b, c (read at rows -1 and +2), m; preprocessed selector s.  Entries (m s, [a b - c@-1, a^2, 7]) and
    (-m, [c@+2]).  Degree 4 in one batch, 3 in two: log_size + 2."""

    def __init__(self, log_n_rows, lookup_elements, batching=(0, 0)):
        self.log_n_rows, self.lookup_elements, self.batching = log_n_rows, lookup_elements, list(batching)

    def log_size(self):
        return self.log_n_rows

    def max_constraint_log_degree_bound(self):
        return self.log_n_rows + 2

    def evaluate(self, eval):
        s = eval.get_preprocessed_column(0)
        a, b = eval.next_trace_mask(), eval.next_trace_mask()
        c_prev, c_next = eval.next_interaction_mask(ORIGINAL_TRACE_IDX, [-1, 2])
        m = eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, m * s, [a * b - c_prev, a.square(), 7]))
        eval.add_to_relation(RelationEntry(self.lookup_elements, -m, [c_next]))
        eval.finalize_logup_batched(self.batching)
        return eval


def general_columns(log, seed=0):
    """(main [a, b, c, m], preprocessed [s]) as uint64 columns; s is a 0 / 1 selector."""
    rng = np.random.default_rng(100 + 13 * log + seed)
    n = 1 << log
    main = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(4)]
    return main, [rng.integers(0, 2, size=n, dtype=np.uint64)]


def general_twin(main, pre, nb):
    a, b, c, m = main
    s, = pre
    return [(m * s % P, [(a * b + P - c[nb(-1)]) % P, a * a % P, 7]), ((P - m) % P, [c[nb(2)]])]


def state_machine_twin(main, pre, nb):
    x, y = main
    return [(1, [x, y]), (P - 1, [(x + 1) % P, y])]


def permutation_twin(main, pre, nb):
    a, b = main
    return [(1, [a]), (P - 1, [b])]


def table_twin(main, pre, nb):
    return [((P - main[0]) % P, [pre[0]])]


def values_twin(main, pre, nb):
    return [(1, [main[0]]), (1, [main[1]])]


def geometric_neighbours(log):
    """nb(offset) from the geometry (air_program_model.neighbour_map with both logs equal)."""
    return lambda off: X.neighbour_map(log, log, off)


def coset_order_neighbours(log):
    """nb(offset) as a shift in coset order through logup_model.positions."""
    idx = np.arange(1 << log, dtype=np.int64)
    return lambda off: CM.shift_in_coset_order(idx, log, off)


def model_fracs(entries, batching, log, z=Z, alpha=ALPHA):
    """fracs_per_batch of columns_model.interaction_trace from a twin's entries."""
    n = 1 << log
    fracs = [(np.full(n, mult % P, dtype=np.uint64) if isinstance(mult, int) else np.asarray(mult, dtype=np.uint64),
              LM.combine_cols(z, alpha, values, n)) for mult, values in entries]
    return [[f for b, f in zip(batching, fracs) if b == j] for j in range(max(batching) + 1)]


def state_machine_closed_form(log, x0, y0, z=Z, alpha=ALPHA):
    """1 / combine([x0, y0]) - 1 / combine([x0 + 2^log, y0]) as a QM31 4-tuple."""
    from gkr_model import qinv, qsub
    return qsub(qinv(LM.combine(z, alpha, [x0 % P, y0 % P])), qinv(LM.combine(z, alpha, [(x0 + (1 << log)) % P, y0 % P])))


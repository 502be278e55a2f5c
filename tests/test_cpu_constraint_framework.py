"""The constraint framework's host side (tstwo_amd/constraint_framework.py) without a GPU: the row-offset index map against the
geometry, the Info / Program / Point evaluators, and the DEEP-ALI identity of FibonacciRowsEval on the integer model
(tests/air_program_model.py)."""
import numpy as np
import pytest

import air_model as M
import air_program_model as X
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd.fields import QM31

P = M.P


def q(t):
    return QM31.from_u32_unchecked(*t)


@pytest.mark.parametrize("trace_log", range(1, 11))
def test_neighbour_index_matches_the_geometry(trace_log):
    for log_expand in (1, 2, 3):
        eval_log = trace_log + log_expand
        if eval_log > 11:
            continue
        for offset in range(-3, 4):
            want = X.neighbour_map(trace_log, eval_log, offset)
            got = [F.offset_bit_reversed_circle_domain_index(r, trace_log, eval_log, offset) for r in range(1 << eval_log)]
            assert got == list(want), (trace_log, log_expand, offset)


def test_neighbour_index_needs_a_larger_evaluation_domain():
    with pytest.raises(ValueError):
        F.offset_bit_reversed_circle_domain_index(0, 4, 4, 1)


def test_info_of_fibonacci_rows():
    inf = F.info(F.FibonacciRowsEval(5, 1, 2))
    assert inf.mask_offsets() == [[[0]], [[-1, 0], [-1, 0]]]
    assert inf.n_constraints == 4
    assert inf.degrees() == [2, 3, 2, 2] and inf.max_degree() == 3
    comp = F.FrameworkComponent(F.FibonacciRowsEval(5, 1, 2), None, [0])
    assert comp.n_columns == 2 and comp.n_constraints == 4 and comp.max_constraint_log_degree_bound() == 7


def test_degree_bounds():
    assert [F.required_log_degree_bound(10, d) for d in (1, 2, 3, 4, 5, 8, 9)] == [11, 11, 12, 12, 13, 13, 14]

    class TooTight(F.FibonacciRowsEval):
        def max_constraint_log_degree_bound(self):
            return self.log_n_rows + 1
    with pytest.raises(ValueError, match="below"):
        F.FrameworkComponent(TooTight(6), None, [0])


def test_framework_refusals():
    class ReadsPreprocessedMask:
        def log_size(self): return 4
        def max_constraint_log_degree_bound(self): return 5
        def evaluate(self, eval):
            eval.next_interaction_mask(A.PREPROCESSED_TRACE_IDX, [0])
    with pytest.raises(ValueError):
        F.FrameworkComponent(ReadsPreprocessedMask())

    class Unnamed(F.FibonacciRowsEval):
        pass
    with pytest.raises(ValueError, match="preprocessed"):
        F.FrameworkComponent(Unnamed(4))                      # reads is_first, names no preprocessed column


def _point_constraints_against_the_model(ev, kind, n_cols):
    rng = np.random.default_rng(1)
    vals = [tuple(int(v) for v in rng.integers(0, P, size=4)) for _ in range(n_cols)]
    got = F.point_constraints(ev, [[q(v)] for v in vals], [])
    assert [c.tup() for c in got] == M.constraints_point(kind, vals)


def test_point_evaluator_of_wide_fibonacci_equals_the_model():
    """The verifier's side of WideFibonacciComponent (the PointEvaluator over WideFibonacciEval) against the model's integers."""
    _point_constraints_against_the_model(F.WideFibonacciEval(6, 100), M.WIDE_FIB, 100)


def test_point_evaluator_of_mul_add_equals_the_model():
    _point_constraints_against_the_model(F.MulAddEval(6), M.MUL_ADD, 3)


class ProgramWideFibonacciEval(F.WideFibonacciEval):
    """The library eval under another type: exact-type dispatch sends it to the program interpreter."""


def test_hand_written_kernel_is_chosen_by_exact_eval_type():
    wf, ma = F.WideFibonacciComponent(8), F.MulAddComponent(8)
    assert (wf.kind, ma.kind) == (A.AIR_WIDE_FIB, A.AIR_MUL_ADD)
    assert wf.program is None and ma.program is None             # the hand-written path compiles no program

    class UserEval:
        kind = A.AIR_MUL_ADD                                      # an eval cannot opt into a hand-written kernel
        def log_size(self): return 4
        def max_constraint_log_degree_bound(self): return 5
        def evaluate(self, eval):
            x, y = eval.next_trace_mask(), eval.next_trace_mask()
            eval.add_constraint(x * y - 1)
    for comp in (F.FrameworkComponent(F.FibonacciRowsEval(5), None, [0]), F.FrameworkComponent(UserEval()),
                 F.FrameworkComponent(ProgramWideFibonacciEval(8))):
        assert comp.kind is None and comp.program is not None


def test_program_is_deterministic_and_small():
    p1 = F.FrameworkComponent(ProgramWideFibonacciEval(8)).program
    p2 = F.FrameworkComponent(ProgramWideFibonacciEval(8)).program
    assert p1.words == p2.words
    assert p1.n_constraints == 98 and p1.n_loads == 100      # every column loaded once
    assert p1.n_regs <= 6                                      # x_i and x_i^2 die as the window moves
    assert p1.n_regs <= F.MAX_REGS
    fr = F.FrameworkComponent(F.FibonacciRowsEval(6, 3, 4), None, [0]).program
    assert fr.n_loads == 5 and fr.n_regs <= F.MAX_REGS


def test_program_matches_the_model_interpreter():
    """The compiled program of FibonacciRowsEval, run by the model's interpreter, gives the AIR's own constraints."""
    log = 4
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, 3, 5), None, [0])
    a, b, first = X.fib_rows_trace(log, 3, 5)
    el = log + 2
    cols = [M.extend(c, log, el) for c in (a, b, first)]
    got = X.run_program(comp.program.words, cols, log, 2)
    nb = X.neighbour_map(log, el, -1)
    mul = lambda x, y: x * y % P
    sub = lambda x, y: (x + P - y) % P
    want = X.fib_rows_constraints(cols[0], cols[1], cols[0][nb], cols[1][nb], cols[2], np.full_like(cols[0], 3),
                                  np.full_like(cols[0], 5), mul, sub, np.ones_like(cols[0]))
    assert len(got) == 4
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_program_register_bound_is_enforced():
    class Wide:
        """Forty values all live at once: the sum of products in reverse order keeps every load alive."""
        def log_size(self): return 4
        def max_constraint_log_degree_bound(self): return 5
        def evaluate(self, eval):
            xs = [eval.next_trace_mask() for _ in range(40)]
            for i in range(40):
                eval.add_constraint(xs[i] - xs[39 - i] * 1)
            acc = 0
            for x in xs:
                acc = acc + x
            eval.add_constraint(acc)
    comp = F.FrameworkComponent(Wide())
    assert comp.program.n_regs <= F.MAX_REGS
    # loads evicted under pressure are reloaded: the program still computes the constraints
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, P, size=32, dtype=np.uint64) for _ in range(40)]
    got = X.run_program(comp.program.words, cols, 4, 1)
    want = [(cols[i] + P - cols[39 - i]) % P for i in range(40)] + [sum(cols) % P]
    assert len(got) == 41 and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_trace_generators_place_rows_in_coset_order():
    for log in (1, 3, 6):
        assert F.coset_order_positions(log) == X.coset_positions(log)
    a, b = F.fibonacci_rows_trace(5, 7, 9)
    ma, mb, mf = X.fib_rows_trace(5, 7, 9)
    assert np.array_equal(a, ma.astype(np.uint32)) and np.array_equal(b, mb.astype(np.uint32))
    assert np.array_equal(F.is_first_column(5), mf.astype(np.uint32)) and F.is_first_column(5)[0] == 1


@pytest.mark.parametrize("log", [3, 5])
def test_deep_ali_identity_of_fibonacci_rows(log):
    rng = np.random.default_rng(log)
    alpha = tuple(int(v) for v in rng.integers(0, P, size=4))
    t = tuple(int(v) for v in rng.integers(0, P, size=4))
    a0, b0 = 3, 11
    honest = X.fib_rows_trace(log, a0, b0)
    assert X.deep_ali_holds(log, honest, a0, b0, alpha, t)
    assert not X.deep_ali_holds(log, X.fib_rows_trace(log, a0, b0, break_at=(1 << log) // 2 + 1), a0, b0, alpha, t)
    assert not X.deep_ali_holds(log, X.fib_rows_trace(log, a0, b0, bad_a0=a0 + 1), a0, b0, alpha, t)
    # the package's verifier side (PointEvaluator over the sampled mask) gives the model's value at the point
    point = M.random_point(t)
    sampled = X.fib_rows_point_values(log, honest, point)
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, a0, b0), None, [0])
    from tstwo_amd.circle import CirclePoint
    pt = CirclePoint(q(point[0]), q(point[1]))
    mask = [[[q(sampled[2])]], [[q(v) for v in sampled[0]], [q(v) for v in sampled[1]]]]
    acc = A.PointEvaluationAccumulator(q(alpha))
    comp.evaluate_constraint_quotients_at_point(pt, mask, acc)
    assert acc.finalize().tup() == X.fib_rows_composition_at_point(log, sampled, a0, b0, alpha, point)
    # and its mask points are the model's
    mp = comp.mask_points(pt)
    prev = X.shifted_point(point, log, -1)
    assert (mp[1][0][0].x.tup(), mp[1][0][0].y.tup()) == prev


def test_components_share_preprocessed_columns():
    alloc = A.TraceLocationAllocator()
    c1 = F.FrameworkComponent(F.FibonacciRowsEval(5), alloc, [2])
    c2 = F.FrameworkComponent(F.FibonacciRowsEval(5), alloc, [2])
    w = F.WideFibonacciComponent(4, 5, alloc)
    comps = A.Components([c1, w, c2], 3)
    from tstwo_amd.circle import CirclePoint
    pt = CirclePoint(q((1, 2, 3, 4)), q((5, 6, 7, 8)))
    mp = comps.mask_points(pt)
    assert [len(c) for c in mp[0]] == [0, 0, 1]
    assert len(mp[1]) == 2 + 5 + 2 and [len(c) for c in mp[1]] == [2, 2, 1, 1, 1, 1, 1, 2, 2]
    assert comps.column_log_sizes()[0] == [0, 0, 5]
    assert comps.column_log_sizes()[1] == [5, 5, 4, 4, 4, 4, 4, 5, 5]
    # callers without a preprocessed tree see what they saw before
    legacy = A.Components([F.WideFibonacciComponent(4, 5)])
    assert legacy.mask_points(pt)[0] == [] and legacy.column_log_sizes()[0] == []
    with pytest.raises(ValueError):
        A.Components([c1], 2)

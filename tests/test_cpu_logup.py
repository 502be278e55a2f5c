"""LogUp on the host, without a GPU: the coset-order position formula of csrc/logup.hip, the integer model (tests/logup_model.py),
LookupElements on both channels, the Info / Program / Point evaluators of the LogUp examples, the refusals of the framework, the
lowering of secure constraints into the base-field program, honest and dishonest model traces, and no scratch in the new kernels."""
import numpy as np
import pytest

import air_program_model as X
import logup_model as LM
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import M31, QM31
from tstwo_amd.poseidon import Poseidon252Channel

P = LM.P


def q(t):
    return QM31.from_u32_unchecked(*t)


def felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def elements(seed=1, size=2):
    rng = np.random.default_rng(seed)
    return LG.LookupElements(q(felt(rng)), q(felt(rng)), size)


# ------------------------------------------------------------------ positions and the model
@pytest.mark.parametrize("n", range(1, 12))
def test_position_formula_matches_coset_order(n):
    want = F.coset_order_positions(n)
    assert [LM.position(k, n) for k in range(1 << n)] == want
    assert list(LM.positions(n)) == want
    assert X.coset_positions(n) == want
    assert list(F._coset_positions(n)) == want


def test_model_combine_column_and_finalize():
    rng = np.random.default_rng(2)
    log, n = 6, 64
    z, alpha = felt(rng), felt(rng)
    le = LG.LookupElements(q(z), q(alpha), 3)
    vals = [int(v) for v in rng.integers(0, P, size=3)]
    assert le.combine(vals).tup() == LM.combine(z, alpha, vals)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2)]
    den = LM.combine_cols(z, alpha, [cols[0], 9, cols[1]], n)
    for r in (0, 17, 63):
        assert tuple(int(v) for v in den[:, r]) == LM.combine(z, alpha, [int(cols[0][r]), 9, int(cols[1][r])])
    num = rng.integers(0, P, size=n, dtype=np.uint64)
    col = LM.column([(num, den)], None, n)
    assert LM.column_identity_holds(col, np.zeros((4, n), dtype=np.uint64), [(num, den)])
    out, claimed = LM.finalize_last(col, log)
    assert claimed == tuple(int(v) for v in col.sum(axis=1) % P)
    assert all(int(out[j][LM.position(n - 1, log)]) == 0 for j in range(4))


@pytest.mark.parametrize("channel", [Blake2sChannel, Poseidon252Channel])
def test_lookup_elements_draw(channel):
    a, b = channel(), channel()
    le = LG.LookupElements.draw(a, 3)
    z, alpha = b.draw_felts(2)
    assert le.z == z and le.alpha == alpha
    assert le.alpha_powers == [QM31.one(), alpha, alpha.mul(alpha)]
    assert a.draw_felt() == b.draw_felt()
    with pytest.raises(ValueError):
        le.combine([1, 2, 3, 4])
    with pytest.raises(ValueError):
        le.combine_columns([1, 2, 3, 4])


# ------------------------------------------------------------------ the evaluators of the examples
def test_info_of_the_examples():
    le = elements()
    perm = F.info(F.PermutationEval(5, le))
    assert perm.mask_offsets() == [[], [[0], [0]], [[-1, 0]] * 4] and perm.degrees() == [3] and perm.secure_flags() == [True]
    table = F.info(F.RangeCheckTableEval(4, le))
    assert table.mask_offsets() == [[[0]], [[0]], [[-1, 0]] * 4] and table.degrees() == [2]
    values = F.info(F.RangeCheckValuesEval(5, le))
    assert values.degrees() == [3] and values.n_interaction == 4
    c = F.FrameworkComponent(F.PermutationEval(5, le), claimed_sum=QM31.zero())
    assert c.n_constraints == 1 and c.program.n_constraints == 4 and c.max_constraint_log_degree_bound() == 7
    assert c.trace_log_degree_bounds() == [[], [5, 5], [5] * 4]
    assert c.trace_locations == {A.ORIGINAL_TRACE_IDX: (0, 2), A.INTERACTION_TRACE_IDX: (0, 4)}
    assert A.INTERACTION_TRACE_IDX == LG.INTERACTION_TRACE_IDX == 2


class ThreeBatches:
    """Three batches (0, 0, 1, 2), a multiplicity column, a 2-value relation: degree 3 (the pair), columns at [0], [0], [-1, 0]."""

    def __init__(self, le, log=4):
        self.le, self.log = le, log

    def log_size(self): return self.log
    def max_constraint_log_degree_bound(self): return self.log + 2

    def evaluate(self, eval):
        a, b, m = eval.next_trace_mask(), eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_to_relation(F.RelationEntry(self.le, m, [a, b]))
        eval.add_to_relation(F.RelationEntry(self.le, 1, [b, 3]))
        eval.add_to_relation(F.RelationEntry(self.le, -m, [a.square()]))
        eval.add_to_relation(F.RelationEntry(self.le, 2, [a - b]))
        eval.add_constraint(a * b - m)
        eval.finalize_logup_batched([0, 0, 1, 2])


def test_info_of_batches():
    inf = F.info(ThreeBatches(elements()))
    assert inf.mask_offsets()[2] == [[0]] * 8 + [[-1, 0]] * 4
    assert inf.secure_flags() == [False, True, True, True]
    assert inf.degrees() == [2, 3, 3, 2]


def test_framework_refusals():
    le = elements()

    class Base:
        def log_size(self): return 4
        def max_constraint_log_degree_bound(self): return 6

    class NoFinalize(Base):
        def evaluate(self, eval):
            eval.add_to_relation(F.RelationEntry(le, 1, [eval.next_trace_mask()]))

    class Twice(Base):
        def evaluate(self, eval):
            eval.add_to_relation(F.RelationEntry(le, 1, [eval.next_trace_mask()]))
            eval.finalize_logup()
            eval.finalize_logup()

    class AfterFinalize(Base):
        def evaluate(self, eval):
            a = eval.next_trace_mask()
            eval.add_to_relation(F.RelationEntry(le, 1, [a]))
            eval.finalize_logup()
            eval.add_to_relation(F.RelationEntry(le, 1, [a]))

    class Gap(Base):
        def evaluate(self, eval):
            a = eval.next_trace_mask()
            eval.add_to_relation(F.RelationEntry(le, 1, [a]))
            eval.add_to_relation(F.RelationEntry(le, 1, [a]))
            eval.finalize_logup_batched([0, 2])

    for ev, what in ((NoFinalize(), "without finalize"), (Twice(), "twice"), (AfterFinalize(), "after finalize"), (Gap(), "consecutive")):
        with pytest.raises(ValueError, match=what):
            F.FrameworkComponent(ev, claimed_sum=QM31.zero())
    with pytest.raises(ValueError, match="claimed_sum"):
        F.FrameworkComponent(F.PermutationEval(4, le))
    with pytest.raises(ValueError, match="claimed_sum"):
        F.FrameworkComponent(F.MulAddEval(4), claimed_sum=QM31.zero())


def test_existing_evals_are_unchanged():
    """A component without LogUp: two trees, no interaction columns."""
    c = F.FrameworkComponent(F.FibonacciRowsEval(5, 1, 2), None, [0])
    assert c.n_interaction_columns == 0 and len(c.trace_log_degree_bounds()) == 2
    assert F.info(F.FibonacciRowsEval(5)).mask_offsets() == [[[0]], [[-1, 0], [-1, 0]]]


# ------------------------------------------------------------------ lowering: program (expanded coefficients) == point evaluator
def _lowering_holds(eval_, n_main, n_pre, claimed, seed):
    rng = np.random.default_rng(seed)
    comp = F.FrameworkComponent(eval_, None, list(range(n_pre)), claimed_sum=claimed)
    log, le = eval_.log_size(), 2
    n = 1 << (log + le)
    n_int = comp.n_interaction_columns
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_main + n_pre + n_int)]
    cons = X.run_program(comp.program.words, cols, log, le)
    coeffs = [q(felt(rng)) for _ in range(comp.n_constraints)]
    exp = [c.tup() for c in F.expand_coeffs(coeffs, comp.secure_flags)]
    from air_model import row_combination
    got = row_combination(exp, cons)
    nbs = {o: X.neighbour_map(log, log + le, o) for o in (-1, 1)}

    def at(col, o, r):
        return QM31.from_(M31(int(col[r if o == 0 else nbs[o][r]])))
    for r in rng.integers(0, n, size=6):
        main = [[at(cols[k], o, r) for o in offs] for k, offs in enumerate(comp.mask_offsets)]
        pre = [at(cols[n_main + i], 0, r) for i in range(n_pre)]
        inter = [[at(cols[n_main + n_pre + k], o, r) for o in offs] for k, offs in enumerate(comp.interaction_offsets)]
        vals = F.point_constraints(eval_, main, pre, inter, claimed, log)
        want = QM31.zero()
        for c, v in zip(coeffs, vals):
            want = want.add(c.mul(v))
        assert tuple(int(x) for x in got[:, r]) == want.tup()


def test_lowering_of_the_examples():
    le = elements(3, 2)
    claimed = q((11, 12, 13, 14))
    _lowering_holds(F.PermutationEval(3, le), 2, 0, claimed, 1)
    _lowering_holds(F.RangeCheckTableEval(3, le), 1, 1, claimed, 2)
    _lowering_holds(F.RangeCheckValuesEval(3, le), 2, 0, claimed, 3)
    _lowering_holds(ThreeBatches(le, 3), 3, 0, claimed, 4)


class RandomSecure:
    """A random DAG of secure values built from main columns, constants and QM31 constants."""

    def __init__(self, seed):
        self.seed = seed

    def log_size(self): return 3
    def max_constraint_log_degree_bound(self): return 7

    def evaluate(self, eval):
        rng = np.random.default_rng(self.seed)
        base = [eval.next_trace_mask() for _ in range(3)]
        pool = [eval._secure(b) for b in base] + [eval._secure(q(felt(rng)))]
        deg = [1, 1, 1, 0]
        for _ in range(8):
            i, j = (int(t) for t in rng.integers(0, len(pool), size=2))
            pick = int(rng.integers(0, 5))
            d = {0: max(deg[i], deg[j]), 1: max(deg[i], deg[j]), 2: deg[i] + deg[j], 3: deg[i], 4: deg[i] + 1}[pick]
            if d > 4:
                continue
            x, y = pool[i], pool[j]
            pool.append(x + y if pick == 0 else x - y if pick == 1 else x * y if pick == 2 else -x if pick == 3 else x * base[0])
            deg.append(d)
        eval.add_constraint(pool[-1])
        eval.add_constraint(base[0] * base[1])
        eval.add_constraint(pool[-2] * q(felt(rng)) + 5)


@pytest.mark.parametrize("seed", range(4))
def test_lowering_of_random_secure_dags(seed):
    ev = RandomSecure(seed)
    comp = F.FrameworkComponent(ev)
    assert comp.secure_flags == [True, False, True]
    _lowering_holds(ev, 3, 0, None, 10 + seed)


# ------------------------------------------------------------------ honest and dishonest model traces
def _row_constraints(eval_, main_cols, inter_cols, claimed, log):
    """Every constraint on every trace row (offset -1 = the previous coset row), from the model's columns."""
    n = 1 << log
    pos = F.coset_order_positions(log)
    prev = {pos[k]: pos[(k - 1) % n] for k in range(n)}
    comp_offs = F.info(eval_)
    out = []
    for r in range(n):
        def at(col, o):
            return QM31.from_(M31(int(col[r if o == 0 else prev[r]])))
        main = [[at(c, o) for o in offs] for c, offs in zip(main_cols, comp_offs.main_offsets)]
        inter = [[at(c, o) for o in offs] for c, offs in zip(inter_cols, comp_offs.interaction_offsets)]
        out += F.point_constraints(eval_, main, [], inter, claimed, log)
    return out


def _model_permutation(log, a, b, z, alpha):
    n = 1 << log
    fr = [(np.ones(n, dtype=np.uint64), LM.combine_cols(z, alpha, [a], n)),
          (np.full(n, P - 1, dtype=np.uint64), LM.combine_cols(z, alpha, [b], n))]
    col = LM.column(fr, None, n)
    return LM.finalize_last(col, log)


def test_honest_and_dishonest_traces():
    rng = np.random.default_rng(9)
    log = 4
    z, alpha = felt(rng), felt(rng)
    le = LG.LookupElements(q(z), q(alpha), 1)
    a = rng.integers(0, P, size=1 << log, dtype=np.uint64)
    b = rng.permutation(a)
    inter, claimed = _model_permutation(log, a, b, z, alpha)
    assert claimed == (0, 0, 0, 0)
    ev = F.PermutationEval(log, le)
    assert all(c == QM31.zero() for c in _row_constraints(ev, [a, b], list(inter), q(claimed), log))
    assert any(c != QM31.zero() for c in _row_constraints(ev, [a, b], list(inter), q((1, 0, 0, 0)), log))
    c2 = b.copy()
    c2[3] = (c2[3] + 1) % P
    inter2, claimed2 = _model_permutation(log, a, c2, z, alpha)
    assert claimed2 != (0, 0, 0, 0)
    assert all(c == QM31.zero() for c in _row_constraints(ev, [a, c2], list(inter2), q(claimed2), log))
    assert any(c != QM31.zero() for c in _row_constraints(ev, [a, c2], list(inter2), QM31.zero(), log))


# ------------------------------------------------------------------ the new kernels' ISA
def test_logup_kernels_use_no_scratch(tmp_path):
    from test_cpu_isa import _disasm
    kernels = _disasm("logup", tmp_path)
    names = [k for k in kernels if "k_logup" in k]
    assert len(names) == 8, names
    for k in names:
        assert not [i for i in kernels[k] if i.startswith("scratch_")], k
        assert not [i for i in kernels[k] if i.startswith(("flat_load", "flat_store"))], k

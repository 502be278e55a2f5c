"""prove(..., diagnose=True), prover.diagnose and FrameworkComponent.assert_constraints on the MI355X: a wide-Fibonacci proof and
a LogUp range-check proof, each with one cell changed before commitment.  Without the flag `prove` raises the plain
ConstraintsNotSatisfied as before; with it a ConstraintViolation names the component, constraint and row that the integer model
(tests/air_check_model.py over the component's program and the committed columns) predicts; an honest commitment has no failures."""
import numpy as np
import pytest

import air_check_model as CK
import logup_model as LM
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd import prover as PR
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles
from tstwo_amd.prover import ConstraintsNotSatisfied, ConstraintViolation, prove

pytestmark = pytest.mark.gpu

P = LM.P


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, HipColumn(np.asarray(c).astype(np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def model_failures(comp, cols):
    """[(constraint, n_rows, first_row)] of the failing constraints, from the model over the component's program"""
    groups = [c for c, secure in enumerate(comp.secure_flags) for _ in range(4 if secure else 1)]
    rep = CK.report(CK.with_groups(comp._constraint_program().words, groups), cols, comp.log_size, groups)
    return [(c, n, first) for c, (n, first) in enumerate(rep) if n]


# ------------------------------------------------------------------ wide Fibonacci beside a mul-add
WF_LOG, WF_COLS, MA_LOG = 8, 12, 6


def wide_fib_setup(cell=None):
    """Components [mul-add, wide Fibonacci] over one main tree; cell = (column, coset row) of the wide Fibonacci trace to change.
    Returns (components, channel, scheme, the wide Fibonacci columns as committed)."""
    rng = np.random.default_rng(21)
    x0, x1 = (rng.integers(0, P, size=1 << MA_LOG, dtype=np.uint64) for _ in range(2))
    wf = [e.values.to_numpy() for e in A.generate_wide_fib_trace(WF_LOG, rng.integers(1, P, size=1 << WF_LOG),
                                                                  rng.integers(1, P, size=1 << WF_LOG), WF_COLS)]
    if cell is not None:
        j, k = cell
        pos = int(LM.positions(WF_LOG)[k])
        wf[j][pos] = (int(wf[j][pos]) + 1) % P
    alloc = A.TraceLocationAllocator()
    comps = [F.MulAddComponent(MA_LOG, alloc), F.WideFibonacciComponent(WF_LOG, WF_COLS, alloc)]
    config = PcsConfig()
    tw = precompute_twiddles(CanonicCoset(WF_LOG + 1 + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    _commit(scheme, [], ch)
    _commit(scheme, _evals([x0, x1, (x0 * x1 + x0) % P], MA_LOG) + _evals(wf, WF_LOG), ch)
    return comps, ch, scheme, wf


def test_wide_fibonacci_with_a_changed_cell():
    cell = (7, 201)
    comps, ch, scheme, wf = wide_fib_setup(cell)
    with pytest.raises(ConstraintsNotSatisfied) as e:
        prove(comps, ch, scheme)
    assert type(e.value) is ConstraintsNotSatisfied and str(e.value) == "Constraints not satisfied."
    comps, ch, scheme, wf = wide_fib_setup(cell)
    want = model_failures(comps[1], wf)
    assert want == [(5, 1, 201), (6, 1, 201), (7, 1, 201)]              # x_7 is in constraints 5, 6 and 7, on its own row
    with pytest.raises(ConstraintViolation) as e:
        prove(comps, ch, scheme, diagnose=True)
    v = e.value
    assert (v.component, v.constraint, v.row, v.n_rows) == (1, 5, 201, 1)
    assert v.failures == want
    assert str(v) == "component 1: constraint 5 is non-zero on 1 of 256 rows, first at row 201"
    assert PR.diagnose(comps, scheme) == [(1, c, n, first) for c, n, first in want]
    assert comps[1].program is None                                     # the hand-written kind still proves on its own kernel


def test_an_honest_wide_fibonacci_commitment_has_no_failures():
    comps, ch, scheme, wf = wide_fib_setup()
    assert PR.diagnose(comps, scheme) == []
    assert comps[1].assert_constraints(wf) is None
    assert comps[1].constraint_failures(_evals(wf, WF_LOG)) == []
    prove(comps, ch, scheme, diagnose=True)


# ------------------------------------------------------------------ a LogUp range check
LOG_RANGE, LOG_VALUES = 6, 7


def range_check_setup(row=None):
    """Components [table, values]; row: the coset row of v0 changed before commitment (the multiplicities and both interaction
    traces are those of the unchanged values).  Returns (components, channel, scheme, the values component's columns)."""
    rng = np.random.default_rng(22)
    config = PcsConfig(5, FriConfig(0, 1, 3))
    v0 = rng.integers(0, 1 << LOG_RANGE, size=1 << LOG_VALUES).astype(np.uint32)
    v1 = rng.integers(0, 1 << LOG_RANGE, size=1 << LOG_VALUES).astype(np.uint32)
    mult = F.range_check_multiplicities(LOG_RANGE, v0, v1)
    committed_v0 = v0.copy()
    if row is not None:
        pos = int(LM.positions(LOG_VALUES)[row])
        committed_v0[pos] = (int(v0[pos]) + 1) % (1 << LOG_RANGE)
    tw = precompute_twiddles(CanonicCoset(max(LOG_RANGE + 1, LOG_VALUES + 2, 10) + 1).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    _commit(scheme, _evals([F.range_check_table_column(LOG_RANGE)], LOG_RANGE), ch)
    _commit(scheme, _evals([mult], LOG_RANGE) + _evals([committed_v0, v1], LOG_VALUES), ch)
    le = LG.LookupElements.draw(ch, 1)
    t_inter, t_sum = F.range_check_table_interaction_trace(LOG_RANGE, mult, le)
    v_inter, v_sum = F.range_check_values_interaction_trace(LOG_VALUES, v0, v1, le)
    ch.mix_felts([t_sum, v_sum])
    _commit(scheme, t_inter + v_inter, ch)
    alloc = A.TraceLocationAllocator()
    comps = [F.FrameworkComponent(F.RangeCheckTableEval(LOG_RANGE, le), alloc, [0], claimed_sum=t_sum),
             F.FrameworkComponent(F.RangeCheckValuesEval(LOG_VALUES, le), alloc, claimed_sum=v_sum)]
    return comps, ch, scheme, [committed_v0, v1] + [e.values.to_numpy() for e in v_inter]


def test_range_check_with_a_changed_value():
    row = 90
    comps, ch, scheme, cols = range_check_setup(row)
    with pytest.raises(ConstraintsNotSatisfied) as e:
        prove(comps, ch, scheme)
    assert type(e.value) is ConstraintsNotSatisfied
    comps, ch, scheme, cols = range_check_setup(row)
    want = model_failures(comps[1], cols)
    assert want == [(0, 1, row)]                                        # the one (secure) LogUp constraint, on the changed row
    with pytest.raises(ConstraintViolation) as e:
        prove(comps, ch, scheme, diagnose=True)
    v = e.value
    assert (v.component, v.constraint, v.row, v.n_rows) == (1, 0, row, 1)
    assert v.failures == want
    assert str(v) == "component 1: constraint 0 is non-zero on 1 of 128 rows, first at row 90"
    assert PR.diagnose(comps, scheme) == [(1, 0, 1, row)]


def test_an_honest_range_check_commitment_has_no_failures():
    comps, ch, scheme, cols = range_check_setup()
    assert PR.diagnose(comps, scheme) == []
    assert comps[1].assert_constraints(cols[:2], (), cols[2:]) is None
    prove(comps, ch, scheme, diagnose=True)

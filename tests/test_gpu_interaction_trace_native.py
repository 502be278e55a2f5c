"""derive_interaction_trace(..., native=True) on the MI355X: the columns programs run as native kernels
(tstwo_air_eval_columns_compiled), and the interaction trace and its claimed sum are those of the interpreter and of the integer
model (tests/columns_model.py interaction_trace over the numpy twins of tests/interaction_evals.py); one LogUp prove / verify
whose component and derivation are both native gives the interpreted proof byte for byte."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import columns_model as CM  # noqa: E402
import interaction_evals as E  # noqa: E402
import logup_model as LM  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import air as A  # noqa: E402
from tstwo_amd import constraint_framework as F  # noqa: E402
from tstwo_amd import logup as LG  # noqa: E402
from tstwo_amd.backend import HipColumn  # noqa: E402
from tstwo_amd.channel import Blake2sChannel  # noqa: E402
from tstwo_amd.circle import CanonicCoset  # noqa: E402
from tstwo_amd.fields import QM31  # noqa: E402
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig  # noqa: E402
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier  # noqa: E402
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles  # noqa: E402
from tstwo_amd.prover import ConstraintsNotSatisfied, prove, verify  # noqa: E402

P = LM.P
LE = E.elements()
X0, Y0 = P - 5, 77                  # the state machine's x runs through P - 1 and wraps to 0


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def u32(cols):
    return [np.asarray(c).astype(np.uint32) for c in cols]


def same_trace(got, want):
    (g_evals, g_sum), (w_evals, w_sum) = got, want
    assert g_sum == w_sum and len(g_evals) == len(w_evals)
    for g, w in zip(g_evals, w_evals):
        assert g.domain == w.domain and np.array_equal(g.values.to_numpy(), w.values.to_numpy())


def equals_model(got, entries, batching, log):
    """The derived trace against columns_model.interaction_trace over a twin's entries."""
    evals, claimed = got
    cols, want_sum = CM.interaction_trace(E.model_fracs(entries, batching, log), log)
    assert claimed.tup() == want_sum and len(evals) == 4 * len(cols)
    domain = CanonicCoset(log).circleDomain()
    for j, col in enumerate(cols):
        for c in range(4):
            assert evals[4 * j + c].domain == domain
            assert np.array_equal(evals[4 * j + c].values.to_numpy(), col[c].astype(np.uint32)), (j, c)


def _cases(log):
    """(id, eval, main, preprocessed, the twin's entries, batching) for every eval tests/interaction_evals.py has a twin of"""
    rng = np.random.default_rng(30 + log)
    n = 1 << log
    nb = E.geometric_neighbours(log)
    main, pre = E.general_columns(log)
    out = [(f"general-{len(set(b))}-batch", E.GeneralEval(log, LE, b), main, pre, E.general_twin(main, pre, nb), b) for b in ([0, 0], [0, 1])]
    x, y = F.state_machine_trace(log, X0, Y0)
    sm = [x.astype(np.uint64), y.astype(np.uint64)]
    out.append(("state-machine", F.StateMachineEval(log, LE), sm, [], E.state_machine_twin(sm, [], nb), [0, 0]))
    a = rng.integers(0, P, size=n, dtype=np.uint64)
    perm = [a, rng.permutation(a)]
    out.append(("permutation", F.PermutationEval(log, LE), perm, [], E.permutation_twin(perm, [], nb), [0, 0]))
    v = [rng.integers(0, n, size=n).astype(np.uint64) for _ in range(2)]
    out.append(("values", F.RangeCheckValuesEval(log, LE), v, [], E.values_twin(v, [], nb), [0, 0]))
    mult = [np.asarray(F.range_check_multiplicities(log, *u32(v))).astype(np.uint64)]
    table = [np.asarray(F.range_check_table_column(log)).astype(np.uint64)]
    out.append(("table", F.RangeCheckTableEval(log, LE), mult, table, E.table_twin(mult, table, nb), [0]))
    return out


@pytest.mark.parametrize("log", [3, 9])
def test_native_trace_equals_the_interpreted_one_and_the_model(log, monkeypatch):
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    n_native = 0
    for name, eval_, main, pre, entries, batching in _cases(log):
        del calls[:]
        native = LG.derive_interaction_trace(eval_, u32(main), u32(pre), native=True)
        assert "tstwo_air_eval_columns" not in calls, name
        n_native += calls.count("tstwo_air_eval_columns_compiled")
        del calls[:]
        plain = LG.derive_interaction_trace(eval_, u32(main), u32(pre))
        assert "tstwo_air_eval_columns_compiled" not in calls and "tstwo_air_columns_compile" not in calls, name
        same_trace(native, plain)
        equals_model(native, entries, batching, log)
    assert n_native == 4                 # both general evals, the state machine's x + 1 and the table's -m run a columns program


class ManyEval:
    """70 entries with the distinct values x + 1 .. x + 70, one batch each: more expressions than one columns program stores."""

    def log_size(self):
        return 3

    def evaluate(self, eval):
        x = eval.next_trace_mask()
        for i in range(70):
            eval.add_to_relation(LG.RelationEntry(LE, 1, [x + (i + 1)]))
        eval.finalize_logup()


def test_more_than_64_expressions_take_several_native_calls(monkeypatch):
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    x = np.random.default_rng(3).integers(0, P, size=8, dtype=np.uint64)
    got = LG.derive_interaction_trace(ManyEval(), u32([x]), native=True)
    assert calls.count("tstwo_air_eval_columns_compiled") == 2 and calls.count("tstwo_air_eval_columns") == 0
    equals_model(got, [(1, [(x + i + 1) % P]) for i in range(70)], list(range(70)), 3)


# ------------------------------------------------------------------ prove / verify
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, c if isinstance(c, HipColumn) else HipColumn(np.asarray(c, dtype=np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def _state_machine_proof(log, native, tamper=False):
    config = PcsConfig()
    tw = precompute_twiddles(CanonicCoset(log + 2 + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    x, y = F.state_machine_trace(log, X0, Y0)
    committed_x = x.copy()
    if tamper:
        committed_x[5] = (int(committed_x[5]) + 1) % P
    _commit(scheme, [], ch)
    _commit(scheme, _evals([committed_x, y], log), ch)
    le = LG.LookupElements.draw(ch, 2)
    inter, claimed = LG.derive_interaction_trace(F.StateMachineEval(log, le), [x, y], native=native)
    ch.mix_felts([claimed])
    _commit(scheme, inter, ch)
    comp = F.FrameworkComponent(F.StateMachineEval(log, le), claimed_sum=claimed, native=native)
    return comp, prove([comp], ch, scheme), config, (inter, claimed)


def _flat(o):
    """A proof as nested tuples of ints, bytes and strings: every field of every dataclass, every element of every sequence."""
    if o is None or isinstance(o, (bool, int, str, bytes)):
        return o
    if isinstance(o, np.ndarray):
        return ("ndarray", str(o.dtype), o.shape, o.tobytes())
    if isinstance(o, np.generic):
        return int(o)
    if dataclasses.is_dataclass(o):
        return (type(o).__name__,) + tuple((f.name, _flat(getattr(o, f.name))) for f in dataclasses.fields(o))
    if callable(getattr(o, "tup", None)):
        return (type(o).__name__, _flat(o.tup()))
    if isinstance(o, dict):
        return tuple((_flat(k), _flat(v)) for k, v in sorted(o.items()))
    if type(o).__name__ == "M31":
        return ("M31", int(o.value))
    if hasattr(o, "__iter__"):
        return tuple(_flat(x) for x in o)
    if hasattr(o, "__dict__"):
        return (type(o).__name__,) + tuple((k, _flat(v)) for k, v in sorted(vars(o).items()))
    raise TypeError(f"a proof holds a {type(o).__name__}")


def test_logup_proof_is_identical_and_verifies(monkeypatch):
    log = 5
    plain_comp, plain, _, _ = _state_machine_proof(log, False)
    comp, proof, config, trace = _state_machine_proof(log, True)
    assert comp.native is not None and plain_comp.native is None
    assert comp.claimed_sum == plain_comp.claimed_sum
    # the component is the caller's handle on the switch: its derive_interaction_trace is native exactly when it is
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    x, y = F.state_machine_trace(log, X0, Y0)
    same_trace(comp.derive_interaction_trace([x, y]), trace)
    assert calls.count("tstwo_air_eval_columns_compiled") == 1 and "tstwo_air_eval_columns" not in calls
    del calls[:]
    same_trace(plain_comp.derive_interaction_trace([x, y]), trace)
    assert calls.count("tstwo_air_eval_columns") == 1 and "tstwo_air_eval_columns_compiled" not in calls
    monkeypatch.undo()
    assert repr(_flat(proof)).encode() == repr(_flat(plain)).encode()
    assert len(repr(_flat(proof))) > 10_000
    ch = Blake2sChannel()
    v = CommitmentSchemeVerifier(config)
    sizes = A.Components([comp], 0).column_log_sizes()
    v.commit(proof.commitments[0], [], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    le = LG.LookupElements.draw(ch, 2)
    assert le.z == comp.eval.lookup_elements.z
    ch.mix_felts([comp.claimed_sum])
    v.commit(proof.commitments[2], sizes[2], ch)
    expected = QM31.from_u32_unchecked(*E.state_machine_closed_form(log, X0, Y0, le.z.tup(), le.alpha.tup()))
    assert comp.claimed_sum == expected
    verify([comp], ch, v, proof, expected)


def test_a_broken_trace_is_still_refused():
    with pytest.raises(ConstraintsNotSatisfied):
        _state_machine_proof(5, True, tamper=True)

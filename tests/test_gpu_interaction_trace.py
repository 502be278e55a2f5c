"""derive_interaction_trace on the MI355X: bit for bit against the hand-written generators of the three LogUp examples, against
the integer model (tests/columns_model.py interaction_trace over the numpy twins of tests/interaction_evals.py) for the general
eval and the state machine, the state machine's closed-form claimed sum, prove -> verify with interaction traces that come from
derive_interaction_trace only, the rejections, and no read-back before the claimed sum."""
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
from tstwo_amd.fri_prover import FriConfig  # noqa: E402
from tstwo_amd.logup import RelationEntry  # noqa: E402
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig  # noqa: E402
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier  # noqa: E402
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles  # noqa: E402
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel  # noqa: E402
from tstwo_amd.prover import ConstraintsNotSatisfied, InvalidLogupSum, prove, verify  # noqa: E402

P = LM.P
LE = E.elements()
X0, Y0 = P - 5, 77                  # the state machine's x runs through P - 1 and wraps to 0


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


def u32(cols):
    return [np.asarray(c).astype(np.uint32) for c in cols]


def same_trace(got, want):
    (g_evals, g_sum), (w_evals, w_sum) = got, want
    assert g_sum == w_sum and len(g_evals) == len(w_evals)
    for g, w in zip(g_evals, w_evals):
        assert g.domain == w.domain and np.array_equal(g.values.to_numpy(), w.values.to_numpy())


def equals_model(got, entries, batching, log, z=E.Z, alpha=E.ALPHA):
    """The derived trace against columns_model.interaction_trace over a twin's entries."""
    evals, claimed = got
    cols, want_sum = CM.interaction_trace(E.model_fracs(entries, batching, log, z, alpha), log)
    assert claimed.tup() == want_sum and len(evals) == 4 * len(cols)
    domain = CanonicCoset(log).circleDomain()
    for j, col in enumerate(cols):
        for c in range(4):
            assert evals[4 * j + c].domain == domain
            assert np.array_equal(evals[4 * j + c].values.to_numpy(), col[c].astype(np.uint32)), (j, c)


# ------------------------------------------------------------------ against the hand-written generators
@pytest.mark.parametrize("log", [4, 10])
def test_derived_trace_equals_the_hand_written_generators(log):
    rng = np.random.default_rng(20 + log)
    a = rng.integers(0, P, size=1 << log, dtype=np.uint32)
    b = rng.permutation(a)
    same_trace(LG.derive_interaction_trace(F.PermutationEval(log, LE), [a, b]), F.permutation_interaction_trace(log, a, b, LE))
    v0, v1 = (rng.integers(0, 1 << log, size=1 << log).astype(np.uint32) for _ in range(2))
    same_trace(LG.derive_interaction_trace(F.RangeCheckValuesEval(log, LE), [v0, v1]), F.range_check_values_interaction_trace(log, v0, v1, LE))
    mult = F.range_check_multiplicities(log, v0, v1)
    got = LG.derive_interaction_trace(F.RangeCheckTableEval(log, LE), [HipColumn(mult)], [F.range_check_table_column(log)])
    same_trace(got, F.range_check_table_interaction_trace(log, mult, LE))
    assert got[1].add(F.range_check_values_interaction_trace(log, v0, v1, LE)[1]) == QM31.zero()


# ------------------------------------------------------------------ against the model
@pytest.mark.parametrize("log", [1, 3, 5, 10])
def test_general_eval_equals_the_model(log):
    main, pre = E.general_columns(log)
    entries = E.general_twin(main, pre, E.geometric_neighbours(log))
    for batching in ([0, 0], [0, 1]):
        got = LG.derive_interaction_trace(E.GeneralEval(log, LE, batching), u32(main), u32(pre))
        equals_model(got, entries, batching, log)


@pytest.mark.parametrize("log", [1, 3, 5, 10])
def test_state_machine_equals_the_model_and_the_closed_form(log):
    x, y = F.state_machine_trace(log, X0, Y0)
    main = [x.astype(np.uint64), y.astype(np.uint64)]
    assert np.array_equal(main[0][LM.positions(log)], (X0 + np.arange(1 << log)) % P)
    got = LG.deriveInteractionTrace(F.StateMachineEval(log, LE), [x, y])
    equals_model(got, E.state_machine_twin(main, [], None), [0, 0], log)
    assert got[1].tup() == E.state_machine_closed_form(log, X0, Y0)


class ManyEval:
    """70 entries with the distinct values x + 1 .. x + 70, one batch each: more expressions than one columns program stores."""

    def log_size(self):
        return 3

    def evaluate(self, eval):
        x = eval.next_trace_mask()
        for i in range(70):
            eval.add_to_relation(RelationEntry(LE, 1, [x + (i + 1)]))
        eval.finalize_logup()


def test_more_than_64_expressions_take_several_calls(monkeypatch):
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    x = np.random.default_rng(3).integers(0, P, size=8, dtype=np.uint64)
    got = LG.derive_interaction_trace(ManyEval(), u32([x]))
    assert calls.count("tstwo_air_eval_columns") == 2 and calls.count("tstwo_logup_column") == 70
    equals_model(got, [(1, [(x + i + 1) % P]) for i in range(70)], list(range(70)), 3)


def test_a_vanishing_denominator_raises():
    """z = x0 + 3 (no i, u, iu part) and y = 0: the second entry's x + 1 meets z at coset row 2."""
    log = 6
    le = LG.LookupElements(q(((X0 + 3) % P, 0, 0, 0)), q(E.ALPHA), 2)
    x, y = F.state_machine_trace(log, X0, 0)
    with pytest.raises(L.TstwoError, match="0 has no inverse"):
        LG.derive_interaction_trace(F.StateMachineEval(log, le), [x, y])
    LG.derive_interaction_trace(F.StateMachineEval(log, LE), [x, y])                  # the flag was cleared


# ------------------------------------------------------------------ prove / verify
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, c if isinstance(c, HipColumn) else HipColumn(np.asarray(c, dtype=np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def _state_machine_proof(log, channel_cls=Blake2sChannel, merkle=None, tamper=False):
    config = PcsConfig()
    tw = precompute_twiddles(CanonicCoset(log + 2 + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    ch = channel_cls()
    scheme = CommitmentSchemeProver(config, tw, merkle)
    x, y = F.state_machine_trace(log, X0, Y0)
    committed_x = x.copy()
    if tamper:
        committed_x[5] = (int(committed_x[5]) + 1) % P
    _commit(scheme, [], ch)
    _commit(scheme, _evals([committed_x, y], log), ch)
    le = LG.LookupElements.draw(ch, 2)
    inter, claimed = LG.derive_interaction_trace(F.StateMachineEval(log, le), [x, y])
    ch.mix_felts([claimed])
    _commit(scheme, inter, ch)
    comp = F.FrameworkComponent(F.StateMachineEval(log, le), claimed_sum=claimed)
    return comp, prove([comp], ch, scheme), config, le


def _verify_state_machine(comp, proof, config, logup_sum, channel_cls=Blake2sChannel, merkle=None):
    ch = channel_cls()
    v = CommitmentSchemeVerifier(config, merkle)
    sizes = A.Components([comp], 0).column_log_sizes()
    v.commit(proof.commitments[0], [], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    le = LG.LookupElements.draw(ch, 2)
    assert le.z == comp.eval.lookup_elements.z
    ch.mix_felts([comp.claimed_sum])
    v.commit(proof.commitments[2], sizes[2], ch)
    verify([comp], ch, v, proof, logup_sum)


def _closed_form(log, le):
    return q(E.state_machine_closed_form(log, X0, Y0, le.z.tup(), le.alpha.tup()))


@pytest.mark.parametrize("log", [4, 8])
def test_prove_verify_state_machine_blake2s(log):
    comp, proof, config, le = _state_machine_proof(log)
    assert comp.max_constraint_log_degree_bound() == log + 2 and comp.program is not None
    assert comp.claimed_sum == _closed_form(log, le)
    _verify_state_machine(comp, proof, config, _closed_form(log, le))
    with pytest.raises(InvalidLogupSum):
        _verify_state_machine(comp, proof, config, QM31.zero())


def test_prove_verify_state_machine_poseidon252():
    comp, proof, config, le = _state_machine_proof(6, Poseidon252Channel, Poseidon252MerkleChannel)
    _verify_state_machine(comp, proof, config, _closed_form(6, le), Poseidon252Channel, Poseidon252MerkleChannel)


def test_a_tampered_trace_value_is_not_provable():
    with pytest.raises(ConstraintsNotSatisfied):
        _state_machine_proof(6, tamper=True)


@pytest.mark.parametrize("batching", [[0, 0], [0, 1]], ids=["one-batch", "two-batches"])
def test_prove_verify_general_eval_beside_wide_fibonacci(batching):
    log, wf_log, blowup = 6, 8, 1
    config = PcsConfig(5, FriConfig(0, blowup, 3))
    rng = np.random.default_rng(11)
    main, pre = E.general_columns(log)
    wf_main = A.generate_wide_fib_trace(wf_log, rng.integers(0, P, size=1 << wf_log), rng.integers(0, P, size=1 << wf_log), 20)
    tw = precompute_twiddles(CanonicCoset(10 + blowup).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    pre_evals, main_evals = _evals(u32(pre), log), _evals(u32(main), log)
    _commit(scheme, pre_evals, ch)
    _commit(scheme, main_evals + wf_main, ch)
    le = LG.LookupElements.draw(ch, 3)
    eval_ = E.GeneralEval(log, le, batching)
    inter, claimed = LG.derive_interaction_trace(eval_, [e.values for e in main_evals], [e.values for e in pre_evals])
    assert len(inter) == 4 * (max(batching) + 1)
    ch.mix_felts([claimed])
    _commit(scheme, inter, ch)
    alloc = A.TraceLocationAllocator()
    comps = [F.FrameworkComponent(eval_, alloc, [0], claimed_sum=claimed), F.WideFibonacciComponent(wf_log, 20, alloc)]
    proof = prove(comps, ch, scheme)
    ch = Blake2sChannel()
    v = CommitmentSchemeVerifier(config)
    sizes = A.Components(comps, 1).column_log_sizes()
    v.commit(proof.commitments[0], [log], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    LG.LookupElements.draw(ch, 3)
    ch.mix_felts([claimed])
    v.commit(proof.commitments[2], sizes[2], ch)
    verify(comps, ch, v, proof, claimed)
    equals_model((inter, claimed), E.general_twin(main, pre, E.geometric_neighbours(log)), batching, log, le.z.tup(), le.alpha.tup())


# ------------------------------------------------------------------ no read-back before the claimed sum
SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_gkr_sum_poly", "tstwo_gather_words", "tstwo_eval_at_point",
              "tstwo_eval_at_point_batch", "tstwo_check_zero_flag", "tstwo_logup_finalize_last", "tstwo_upload_wait"}


def test_nothing_is_read_back_before_the_claimed_sum(monkeypatch):
    """The calls test_logup_composition_phase_makes_no_readback counts, here up to finalize_last: its zero-flag check and its
    claimed sum are the first and only read-backs, behind every columns program and every tstwo_logup_column."""
    log = 10
    main, pre = E.general_columns(log)
    main, pre = [HipColumn(c) for c in u32(main)], [HipColumn(c) for c in u32(pre)]
    L.sync()
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    LG.derive_interaction_trace(E.GeneralEval(log, LE, [0, 1]), main, pre)
    monkeypatch.undo()
    assert calls.count("tstwo_air_eval_columns") == 1 and calls.count("tstwo_logup_column") == 2
    first = calls.index("tstwo_check_zero_flag")
    assert sum(c in SYNC_CALLS for c in calls[:first]) == 0
    assert calls[first:] == ["tstwo_check_zero_flag", "tstwo_logup_finalize_last"]
    assert max(i for i, c in enumerate(calls) if c in ("tstwo_air_eval_columns", "tstwo_logup_column")) < first

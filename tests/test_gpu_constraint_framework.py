"""User-defined constraints on the MI355X: tstwo_air_eval_program bit-exact against the integer model (tests/air_program_model.py)
on random programs, the framework's composition polynomial against the hand-written kernels', prove -> verify of
FibonacciRowsEval (row offsets, a preprocessed selector, degree 3) alone and beside the hand-written components, rejections, and
no read-back in the composition phase."""
import copy
import ctypes as C

import numpy as np
import pytest

import air_model as M
import air_program_model as X
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd.backend import HipColumn, SecureColumnByCoords
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier
from tstwo_amd.poly import HipCircleEvaluation, evaluate_polynomials, interpolate_columns, precompute_twiddles
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel
from tstwo_amd.prover import ConstraintsNotSatisfied, OodsNotMatching, StarkProof, prove, verify

pytestmark = pytest.mark.gpu

P = M.P
vp = C.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


def rand_felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def col(a):
    return HipColumn(np.asarray(a, dtype=np.uint32))


# ------------------------------------------------------------------ the kernel against the model
def _call_raw(cols_ptrs, trace_log, log_expand, words, n_constraints, coeffs, dinv, acc_ptrs):
    cw = L.u32x([w for c in coeffs for w in c])
    L.call("tstwo_air_eval_program", L.ptr_array(cols_ptrs), len(cols_ptrs), trace_log, log_expand, L.u32x(words), len(words) // 2,
           cw, n_constraints, L.u32x(dinv), L.p4(acc_ptrs))


def _run_case(seed, trace_log, log_expand, n_cols, n_constraints, n_ops, aligned=True):
    rng = np.random.default_rng(seed)
    n = 1 << (trace_log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    words = X.random_program(rng, n_cols, n_constraints, n_ops, max_offset=3)
    coeffs = [rand_felt(rng) for _ in range(n_constraints)]
    dinv = M.denom_inv(trace_log, trace_log + log_expand)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want = X.eval_program_on_domain(words, cols, trace_log, log_expand, coeffs, dinv, pre)
    k = 0 if aligned else 1             # unaligned: the data starts one word into a buffer of n + 1 words
    dcols = [col(np.concatenate([np.zeros(k, dtype=np.uint64), c])) for c in cols]
    dacc = [col(np.concatenate([np.zeros(k, dtype=np.uint64), pre[j]])) for j in range(4)]
    _call_raw([c.ptr + 4 * k for c in dcols], trace_log, log_expand, words, n_constraints, coeffs, dinv, [a.ptr + 4 * k for a in dacc])
    for j in range(4):
        assert np.array_equal(dacc[j].to_numpy()[k:], want[j].astype(np.uint32)), j


PROGRAM_CASES = [(tl, le) for tl in (2, 3, 5, 8, 11, 14, 17, 20) for le in (1, 2, 3) if tl + le <= 21]


@pytest.mark.parametrize("trace_log,log_expand", PROGRAM_CASES)
def test_program_kernel_matches_model(trace_log, log_expand):
    _run_case(7 * trace_log + log_expand, trace_log, log_expand, n_cols=6, n_constraints=5, n_ops=40)


@pytest.mark.parametrize("trace_log,log_expand", [(2, 1), (6, 2), (10, 3), (13, 1)])
def test_program_kernel_unaligned_fallback(trace_log, log_expand):
    _run_case(100 + trace_log, trace_log, log_expand, n_cols=5, n_constraints=3, n_ops=30, aligned=False)


def test_program_kernel_more_than_64_columns():
    _run_case(555, 9, 2, n_cols=90, n_constraints=20, n_ops=300)


def test_program_kernel_many_registers_and_constraints():
    _run_case(556, 7, 1, n_cols=12, n_constraints=200, n_ops=600)


def test_program_kernel_odd_small_domain():
    # 2 rows in all (trace_log 0, log_expand 1): the scalar path
    _run_case(557, 0, 1, n_cols=3, n_constraints=2, n_ops=12)


# ------------------------------------------------------------------ rejections of the entry point
def _small_call(words, n_constraints=1, log_expand=1, n_cols=2, trace_log=3):
    n = 1 << (trace_log + log_expand)
    cols = [col(np.zeros(n)) for _ in range(n_cols)]
    acc = [col(np.zeros(n)) for _ in range(4)]
    _call_raw([c.ptr for c in cols], trace_log, log_expand, words, n_constraints, [(1, 0, 0, 0)] * n_constraints,
              [1] * (1 << log_expand), [a.ptr for a in acc])


def test_program_entry_rejects_bad_programs():
    ok = X.encode(X.LOAD, 0, 1, -2) + X.encode(X.ACC, 0, 0)
    _small_call(ok)
    bad = {
        "bad opcode": X.encode(X.LOAD, 0, 0, 0) + X.encode(9, 1, 0, 0) + X.encode(X.ACC, 0, 0),
        "register": X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ADD, 1, 0, 5) + X.encode(X.ACC, 0, 1),
        "register ": X.encode(X.LOAD, 40, 0, 0) + X.encode(X.ACC, 0, 40),
        "column out of range": X.encode(X.LOAD, 0, 2, 0) + X.encode(X.ACC, 0, 0),
        "offset beyond": X.encode(X.LOAD, 0, 0, F.MAX_OFFSET + 1) + X.encode(X.ACC, 0, 0),
        "constant out of range": X.encode(X.CONST, 0, 0, P) + X.encode(X.ACC, 0, 0),
    }
    for what, words in bad.items():
        with pytest.raises(L.TstwoError, match=what.strip()):
            _small_call(words)
    with pytest.raises(L.TstwoError, match="ACC"):
        _small_call(ok, n_constraints=2)
    with pytest.raises(L.TstwoError, match="log_expand"):
        _small_call(ok, log_expand=0)
    _small_call(ok)                     # still works


def test_program_entry_is_refused_during_graph_capture():
    n = 1 << 6
    rng = np.random.default_rng(9)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2)]
    words = X.encode(X.LOAD, 0, 0, -1) + X.encode(X.LOAD, 1, 1, 1) + X.encode(X.MUL, 0, 0, 1) + X.encode(X.ACC, 0, 0)
    coeffs = [rand_felt(rng)]
    dinv = M.denom_inv(4, 6)
    dcols = [col(c) for c in cols]
    acc = [col(np.zeros(n)) for _ in range(4)]
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="graph capture"):
            _call_raw([c.ptr for c in dcols], 4, 2, words, 1, coeffs, dinv, [a.ptr for a in acc])
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)
    _call_raw([c.ptr for c in dcols], 4, 2, words, 1, coeffs, dinv, [a.ptr for a in acc])
    want = X.eval_program_on_domain(words, cols, 4, 2, coeffs, dinv)
    for j in range(4):
        assert np.array_equal(acc[j].to_numpy(), want[j].astype(np.uint32))


# ------------------------------------------------------------------ the same composition polynomial as the hand-written kernels
def _device_trace(cols, log, eval_log, twiddles, pre=()):
    def tree(cs):
        ev = [HipCircleEvaluation(CanonicCoset(log).circleDomain(), col(c)) for c in cs]
        ps = interpolate_columns(ev, twiddles) if ev else []
        return ps, (evaluate_polynomials(ps, CanonicCoset(eval_log).circleDomain(), twiddles) if ps else [])
    p0, e0 = tree(list(pre))
    p1, e1 = tree(cols)
    return A.Trace([p0, p1], [e0, e1])


class ProgramWideFibonacciEval(F.WideFibonacciEval):
    """The library evals under other types: exact-type dispatch sends them to the program interpreter."""


class ProgramMulAddEval(F.MulAddEval):
    pass


@pytest.mark.parametrize("which", ["wide_fib", "mul_add"])
def test_framework_composition_equals_hand_written(which):
    rng = np.random.default_rng(31)
    log = 10
    if which == "wide_fib":
        cols = M.wide_fib_trace(rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log), 100)
        hand, fw = F.WideFibonacciComponent(log, 100), F.FrameworkComponent(ProgramWideFibonacciEval(log, 100))
    else:
        cols = M.mul_add_trace(rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log))
        hand, fw = F.MulAddComponent(log), F.FrameworkComponent(ProgramMulAddEval(log))
    assert hand.kind is not None and fw.kind is None            # one component per kernel
    tw = precompute_twiddles(CanonicCoset(log + 2).circleDomain().halfCoset)
    trace = _device_trace(cols, log, log + 1, tw)
    alpha = q(rand_felt(rng))
    want = A.ComponentProvers([hand]).compute_composition_polynomial(alpha, trace, tw)
    got = A.ComponentProvers([fw]).compute_composition_polynomial(alpha, trace, tw)
    for j in range(4):
        assert np.array_equal(got[j].coeffs.to_numpy(), want[j].coeffs.to_numpy()), j


# ------------------------------------------------------------------ prove / verify
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, col(c)) for c in cols]


def _commit_and_prove(components, pre_evals, main_evals, config, channel, merkle_channel=None):
    max_log = max(c.max_constraint_log_degree_bound() for c in components)
    tw = precompute_twiddles(CanonicCoset(max_log + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    scheme = CommitmentSchemeProver(config, tw, merkle_channel)
    for evs in (pre_evals, main_evals):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(channel)
    return prove(components, channel, scheme)


def _verify(components, proof, config, channel, pre_sizes, merkle_channel=None):
    v = CommitmentSchemeVerifier(config, merkle_channel)
    sizes = A.Components(components, len(pre_sizes)).column_log_sizes()
    v.commit(proof.commitments[0], pre_sizes, channel)
    v.commit(proof.commitments[1], sizes[1], channel)
    verify(components, channel, v, proof)


def _fib_rows(log, a0=3, b0=5, alloc=None, pre_index=0):
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, a0, b0), alloc, [pre_index])
    a, b = F.fibonacci_rows_trace(log, a0, b0)
    return comp, _evals([a, b], log), _evals([F.is_first_column(log)], log)


@pytest.mark.parametrize("log", [4, 5, 8, 11, 14, 16])
def test_prove_verify_fibonacci_rows_blake2s(log):
    comp, main, pre = _fib_rows(log, 3 + log, 5)
    config = PcsConfig()
    proof = _commit_and_prove([comp], pre, main, config, Blake2sChannel())
    assert [len(c) for c in proof.sampled_values[1]] == [2, 2] and [len(c) for c in proof.sampled_values[0]] == [1]
    _verify([comp], proof, config, Blake2sChannel(), [log])


@pytest.mark.parametrize("log", [4, 9, 16])
def test_prove_verify_fibonacci_rows_poseidon252(log):
    comp, main, pre = _fib_rows(log, 1, 1)
    config = PcsConfig()
    proof = _commit_and_prove([comp], pre, main, config, Poseidon252Channel(), Poseidon252MerkleChannel)
    _verify([comp], proof, config, Poseidon252Channel(), [log], Poseidon252MerkleChannel)


def _mixed():
    """FibonacciRowsEval + WideFibonacciComponent + a mul-add on the program path; preprocessed tree: [unread, is_first] of the same size."""
    alloc = A.TraceLocationAllocator()
    rng = np.random.default_rng(77)
    fr, fr_main, fr_pre = _fib_rows(9, 2, 7, alloc, pre_index=1)
    wf = F.WideFibonacciComponent(8, 20, alloc)
    wf_main = A.generate_wide_fib_trace(8, rng.integers(0, P, size=1 << 8), rng.integers(0, P, size=1 << 8), 20)
    ma = F.FrameworkComponent(ProgramMulAddEval(6), alloc)
    ma_main = _evals(M.mul_add_trace(rng.integers(0, P, size=64), rng.integers(0, P, size=64)), 6)
    unread = _evals([rng.integers(0, P, size=1 << 9)], 9)
    return [fr, wf, ma], unread + fr_pre, fr_main + wf_main + ma_main, [9, 9]


@pytest.mark.parametrize("blowup", [1, 2])
def test_prove_verify_mixed_components(blowup):
    comps, pre, main, pre_sizes = _mixed()
    config = PcsConfig(5, FriConfig(0, blowup, 3))
    proof = _commit_and_prove(comps, pre, main, config, Blake2sChannel())
    assert [len(c) for c in proof.sampled_values[0]] == [0, 1]
    _verify(comps, proof, config, Blake2sChannel(), pre_sizes)


def test_prove_rejects_a_broken_transition():
    log = 7
    comp, main, pre = _fib_rows(log, 3, 5)
    b = main[1].values.to_numpy()
    pos = F.coset_order_positions(log)[40]
    b[pos] = (int(b[pos]) + 1) % P
    main[1] = HipCircleEvaluation(main[1].domain, col(b))
    with pytest.raises(ConstraintsNotSatisfied):
        _commit_and_prove([comp], pre, main, PcsConfig(), Blake2sChannel())


def test_prove_rejects_a_wrong_start():
    log = 7
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, 3, 5), None, [0])
    a, b = F.fibonacci_rows_trace(log, 4, 5)                # an honest sequence from the wrong a0
    with pytest.raises(ConstraintsNotSatisfied):
        _commit_and_prove([comp], _evals([F.is_first_column(log)], log), _evals([a, b], log), PcsConfig(), Blake2sChannel())


@pytest.fixture(scope="module")
def honest():
    comp, main, pre = _fib_rows(6, 3, 5)
    config = PcsConfig()
    return comp, config, _commit_and_prove([comp], pre, main, config, Blake2sChannel())


def _bump(v):
    t = list(v.tup())
    t[0] = (t[0] + 1) % P
    return q(t)


def test_verify_rejects_a_tampered_offset_sample(honest):
    comp, config, proof = honest
    _verify([comp], proof, config, Blake2sChannel(), [6])
    bad = StarkProof(copy.deepcopy(proof.commitment_scheme_proof))
    bad.sampled_values[1][1][0] = _bump(bad.sampled_values[1][1][0])           # prev_b
    with pytest.raises(OodsNotMatching):
        _verify([comp], bad, config, Blake2sChannel(), [6])


def test_verify_rejects_a_tampered_preprocessed_sample(honest):
    comp, config, proof = honest
    bad = StarkProof(copy.deepcopy(proof.commitment_scheme_proof))
    bad.sampled_values[0][0][0] = _bump(bad.sampled_values[0][0][0])           # is_first
    with pytest.raises(OodsNotMatching):
        _verify([comp], bad, config, Blake2sChannel(), [6])


class ReadbackCounter:
    SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_gkr_sum_poly", "tstwo_gather_words",
                  "tstwo_eval_at_point", "tstwo_eval_at_point_batch", "tstwo_check_zero_flag"}

    def __init__(self, monkeypatch):
        self.n = 0
        orig_call = L.call

        def call(name, *a):
            if name in self.SYNC_CALLS:
                self.n += 1
            return orig_call(name, *a)
        monkeypatch.setattr(L, "call", call)


def test_framework_composition_phase_makes_no_readback(monkeypatch):
    comps, pre, main, _ = _mixed()
    tw = precompute_twiddles(CanonicCoset(12).circleDomain().halfCoset)
    scheme = CommitmentSchemeProver(PcsConfig(), tw)
    ch = Blake2sChannel()
    for evs in (pre, main):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(ch)
    L.sync()
    counter = ReadbackCounter(monkeypatch)
    alpha = ch.draw_felt()
    poly = A.ComponentProvers(comps, 2).compute_composition_polynomial(alpha, A.Trace.of(scheme), tw)
    tb = scheme.tree_builder()
    tb.extend_polys(poly.into_coordinate_polys())
    tb.commit(ch)
    assert counter.n == 0

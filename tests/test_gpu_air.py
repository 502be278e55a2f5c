"""AIR proving on the MI355X: the trace-generation and constraint-quotient kernels bit-exact against the integer model
(tests/air_model.py), the composition polynomial against the model's, and prove -> verify for wide Fibonacci, the Rust tutorial's
example 05 and a multi-component set, with tampered proofs rejected and no read-back in the composition phase."""
import copy
import ctypes as C
import re

import numpy as np
import pytest

import air_model as M
import air_plan as AP
import air_program_model as X
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd.backend import HipColumn, SecureColumnByCoords
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.fri_verifier import FriVerificationError
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier, VerificationError
from tstwo_amd.poly import HipCircleEvaluation, interpolate_columns, evaluate_polynomials, precompute_twiddles
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel
from tstwo_amd.prover import ConstraintsNotSatisfied, OodsNotMatching, StarkProof, prove, verify

pytestmark = pytest.mark.gpu

P = M.P
KIND = {M.WIDE_FIB: A.AIR_WIDE_FIB, M.MUL_ADD: A.AIR_MUL_ADD}


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


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("log,n_cols", [(2, 3), (3, 100), (5, 4), (8, 17), (12, 100), (16, 7), (20, 100)])
def test_wide_fib_trace_kernel_matches_model(log, n_cols):
    rng = np.random.default_rng(log)
    a, b = rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log)
    got = A.generate_wide_fib_trace(log, a, b, n_cols)
    want = M.wide_fib_trace(a, b, n_cols)
    assert len(got) == n_cols
    for g, w in zip(got, want):
        assert g.domain == CanonicCoset(log).circleDomain()
        assert np.array_equal(g.values.to_numpy(), w.astype(np.uint32))


CASES = [(M.WIDE_FIB, 3, 2, 1), (M.WIDE_FIB, 4, 1, 1), (M.WIDE_FIB, 4, 6, 1), (M.WIDE_FIB, 17, 11, 1), (M.WIDE_FIB, 17, 20, 1),
         (M.WIDE_FIB, 100, 3, 1), (M.WIDE_FIB, 100, 14, 1), (M.WIDE_FIB, 100, 18, 1), (M.WIDE_FIB, 17, 9, 2),
         (M.MUL_ADD, 3, 2, 1), (M.MUL_ADD, 3, 8, 2), (M.MUL_ADD, 3, 20, 1)]


@pytest.mark.parametrize("kind,n_cols,log,log_expand", CASES)
def test_constraint_quotients_kernel_matches_model_and_adds(kind, n_cols, log, log_expand):
    rng = np.random.default_rng(1000 + 37 * log + n_cols + log_expand)
    n = 1 << (log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    n_c = M.n_constraints(kind, n_cols)
    coeffs = [rand_felt(rng) for _ in range(n_c)]
    dinv = M.denom_inv(log, log + log_expand)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want = M.quotients_on_domain(kind, cols, log, log_expand, coeffs, dinv, pre)
    acc = SecureColumnByCoords.from_numpy([pre[j].astype(np.uint32) for j in range(4)])
    A.evaluate_constraint_quotients(KIND[kind], [col(c) for c in cols], log, log_expand, [q(c) for c in coeffs], dinv, acc)
    got = acc.to_numpy()
    for j in range(4):
        assert np.array_equal(got[j], want[j].astype(np.uint32)), j


def test_constraint_quotients_rejects_bad_arguments():
    acc = SecureColumnByCoords.zeros(8)
    cols = [col(np.zeros(8)) for _ in range(4)]
    with pytest.raises(L.TstwoError):     # wrong number of coefficients for 4 wide-Fibonacci columns
        A.evaluate_constraint_quotients(A.AIR_WIDE_FIB, cols, 2, 1, [q((1, 0, 0, 0))], [1, 1], acc)
    with pytest.raises(L.TstwoError):     # mul-add takes exactly 3 columns
        A.evaluate_constraint_quotients(A.AIR_MUL_ADD, cols, 2, 1, [q((1, 0, 0, 0))], [1, 1], acc)


# ------------------------------------------------------------------ one row per lane, and the grid-stride loops
# Sizes from the plan's model (tests/air_plan.py) for the part the tests run on: the smallest logs at which the lanes of
# k_wide_fib_trace, k_constraint_quotients and k_air_program take a second turn round the grid, in fours and (every pointer one
# word off a 16-byte boundary) row by row; and a small size row by row, which nothing above runs.
STRIDE_CASES = [("w1-small", 1, 6), ("w4-stride", 4, None), ("w1-stride", 1, None)]
STRIDE_IDS = [c[0] for c in STRIDE_CASES]


def _n_cus():
    return int(re.search(r"(\d+) CUs", L.device_name()).group(1))


def _stride_shape(entry, w, small_log, log_expand, n_cols, n_terminal, program_len=0, n_regs=0):
    """(log of the rows, word offset of every pointer); asserts from the model that the call runs at W = w and strides, or does not."""
    log = small_log if small_log is not None else AP.first_striding_log(entry, w, _n_cus())
    i = AP.Input(entry, AP.MUL_ADD, log, log_expand, n_cols, n_terminal, program_len, n_regs, w == 4, _n_cus())
    assert AP.plan(i).w == w and AP.strides(i) == (small_log is None), i
    assert small_log is not None or not AP.strides(i._replace(log=log - 1))
    return log, 0 if w == 4 else 1


def _shifted(arrays, k):
    """Device copies that begin k words into their buffers, and the pointers to them."""
    bufs = [col(np.concatenate([np.zeros(k, dtype=np.uint64), np.asarray(a, dtype=np.uint64)])) for a in arrays]
    return bufs, [b.ptr + 4 * k for b in bufs]


@pytest.mark.parametrize("name,w,small_log", STRIDE_CASES, ids=STRIDE_IDS)
def test_wide_fib_trace_kernel_at_both_widths_and_beyond_the_grid(name, w, small_log):
    log, k = _stride_shape("wide_fib_trace", w, small_log, 0, 2, 0)
    rng = np.random.default_rng(300 + log)
    a, b = rng.integers(0, P, size=1 << log, dtype=np.uint64), rng.integers(0, P, size=1 << log, dtype=np.uint64)
    (da, db), (pa, pb) = _shifted([a, b], k)
    outs = [HipColumn.zeros((1 << log) + k) for _ in range(2)]
    L.call("tstwo_air_wide_fib_trace", C.c_void_p(pa), C.c_void_p(pb), log, L.ptr_array([o.ptr + 4 * k for o in outs]), 2)
    for o, want in zip(outs, (a, b)):
        got = o.to_numpy()
        assert np.array_equal(got[k:], want.astype(np.uint32)) and not got[:k].any()
    if name == "w1-small":          # more than the two columns that are copies: the recurrence, row by row
        outs = [HipColumn.zeros((1 << log) + k) for _ in range(5)]
        L.call("tstwo_air_wide_fib_trace", C.c_void_p(pa), C.c_void_p(pb), log, L.ptr_array([o.ptr + 4 * k for o in outs]), 5)
        for o, want in zip(outs, M.wide_fib_trace(a, b, 5)):
            assert np.array_equal(o.to_numpy()[k:], want.astype(np.uint32))


@pytest.mark.parametrize("name,w,small_log", STRIDE_CASES, ids=STRIDE_IDS)
def test_constraint_quotients_kernel_at_both_widths_and_beyond_the_grid(name, w, small_log):
    """MUL_ADD over 3 columns, bit for bit against the model on every row."""
    log_expand = 1
    eval_log, k = _stride_shape("quotients", w, small_log, log_expand, 3, 1)
    trace_log, n = eval_log - log_expand, 1 << eval_log
    rng = np.random.default_rng(400 + eval_log)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(3)]
    coeffs, dinv = [rand_felt(rng)], M.denom_inv(trace_log, eval_log)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want = M.quotients_on_domain(M.MUL_ADD, cols, trace_log, log_expand, coeffs, dinv, pre)
    dcols, pcols = _shifted(cols, k)
    dacc, pacc = _shifted(pre, k)
    L.call("tstwo_air_constraint_quotients", A.AIR_MUL_ADD, L.ptr_array(pcols), 3, trace_log, log_expand, L.u32x(list(coeffs[0])), 1,
           L.u32x([int(d) for d in dinv]), L.p4(pacc))
    for j in range(4):
        got = dacc[j].to_numpy()
        assert np.array_equal(got[k:], want[j].astype(np.uint32)) and not got[:k].any(), j


# r0 = x0, r1 = x1 one row back, r2 = r0 r1 - x2: 3 columns, 6 instructions, one constraint
STRIDE_PROGRAM = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, -1) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.LOAD, 1, 2, 0)
                  + X.encode(X.SUB, 2, 2, 1) + X.encode(X.ACC, 0, 2))


@pytest.mark.parametrize("name,w,small_log", STRIDE_CASES[1:], ids=STRIDE_IDS[1:])
def test_program_interpreter_beyond_the_grid_matches_the_model(name, w, small_log):
    """k_air_program where its one-wave workgroups wrap, against the integer model (tests/air_program_model.py) on every row."""
    log_expand = 1
    eval_log, k = _stride_shape("eval_program", w, small_log, log_expand, 3, 1, len(STRIDE_PROGRAM) // 2, 3)
    trace_log, n = eval_log - log_expand, 1 << eval_log
    rng = np.random.default_rng(500 + eval_log)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(3)]
    coeffs, dinv = [rand_felt(rng)], M.denom_inv(trace_log, eval_log)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want = X.eval_program_on_domain(STRIDE_PROGRAM, cols, trace_log, log_expand, coeffs, dinv, pre)
    dcols, pcols = _shifted(cols, k)
    dacc, pacc = _shifted(pre, k)
    L.call("tstwo_air_eval_program", L.ptr_array(pcols), 3, trace_log, log_expand, L.u32x(STRIDE_PROGRAM), len(STRIDE_PROGRAM) // 2,
           L.u32x(list(coeffs[0])), 1, L.u32x([int(d) for d in dinv]), L.p4(pacc))
    for j in range(4):
        got = dacc[j].to_numpy()
        assert np.array_equal(got[k:], want[j].astype(np.uint32)) and not got[:k].any(), j


# ------------------------------------------------------------------ composition polynomial
def _device_trace(model_components, twiddles):
    """Trace object of the model's components: trace polys and their evaluations on each eval domain (log + 1)."""
    polys, evals = [], []
    for _, log, cols in model_components:
        ev = [HipCircleEvaluation(CanonicCoset(log).circleDomain(), col(c)) for c in cols]
        ps = interpolate_columns(ev, twiddles)
        polys += ps
        evals += evaluate_polynomials(ps, CanonicCoset(log + 1).circleDomain(), twiddles)
    return A.Trace([[], polys], [[], evals])


def _host_components(specs):
    alloc = A.TraceLocationAllocator()
    return [F.WideFibonacciComponent(log, n, alloc) if kind == M.WIDE_FIB else F.MulAddComponent(log, alloc) for kind, log, n in specs]


def _model_components(specs, rng):
    out = []
    for kind, log, n in specs:
        a, b = rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log)
        out.append((kind, log, M.wide_fib_trace(a, b, n) if kind == M.WIDE_FIB else M.mul_add_trace(a, b)))
    return out


@pytest.mark.parametrize("specs", [[(M.WIDE_FIB, 9, 100)], [(M.MUL_ADD, 6, 3)],
                                   [(M.WIDE_FIB, 10, 20), (M.WIDE_FIB, 8, 16), (M.MUL_ADD, 5, 3), (M.WIDE_FIB, 8, 5)]])
def test_composition_polynomial_matches_model(specs):
    rng = np.random.default_rng(len(specs))
    model = _model_components(specs, rng)
    alpha = rand_felt(rng)
    max_log = max(l for _, l, _ in specs) + 1
    tw = precompute_twiddles(CanonicCoset(max_log + 1).circleDomain().halfCoset)
    trace = _device_trace(model, tw)
    poly = A.ComponentProvers(_host_components(specs)).compute_composition_polynomial(q(alpha), trace, tw)
    log, want = M.composition_polynomial(model, alpha)
    assert poly.log_size() == log
    for j in range(4):
        assert np.array_equal(poly[j].coeffs.to_numpy(), want[j].astype(np.uint32)), j


# ------------------------------------------------------------------ prove / verify
def _commit_and_prove(components, trace_evals, config, channel, merkle_channel=None, mix_log=None):
    max_log = max(c.max_constraint_log_degree_bound() for c in components)
    tw = precompute_twiddles(CanonicCoset(max_log + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    scheme = CommitmentSchemeProver(config, tw, merkle_channel)
    tb = scheme.tree_builder()
    tb.extend_evals([])
    tb.commit(channel)
    if mix_log is not None:
        channel.mix_u64(mix_log)
    tb = scheme.tree_builder()
    tb.extend_evals(trace_evals)
    tb.commit(channel)
    return prove(components, channel, scheme)


def _verify(components, proof, config, channel, merkle_channel=None, mix_log=None):
    v = CommitmentSchemeVerifier(config, merkle_channel)
    sizes = A.Components(components).column_log_sizes()
    v.commit(proof.commitments[0], sizes[0], channel)
    if mix_log is not None:
        channel.mix_u64(mix_log)
    v.commit(proof.commitments[1], sizes[1], channel)
    verify(components, channel, v, proof)


def _wide_fib(log, n_cols, seed=0, alloc=None):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log)
    return F.WideFibonacciComponent(log, n_cols, alloc), A.generate_wide_fib_trace(log, a, b, n_cols)


@pytest.mark.parametrize("log", [4, 5, 6, 8, 10, 12, 14, 16])
def test_prove_verify_wide_fibonacci_100(log):
    comp, trace = _wide_fib(log, 100, seed=log)
    config = PcsConfig()
    proof = _commit_and_prove([comp], trace, config, Blake2sChannel())
    assert len(proof.commitments) == 3 and len(proof.sampled_values[2]) == 4
    _verify([comp], proof, config, Blake2sChannel())


def test_prove_verify_example05_table():
    comp = F.MulAddComponent(4)
    domain = CanonicCoset(4).circleDomain()
    trace = [HipCircleEvaluation(domain, col(c)) for c in M.example05_trace(4)]
    config = PcsConfig()
    proof = _commit_and_prove([comp], trace, config, Blake2sChannel(), mix_log=4)
    _verify([comp], proof, config, Blake2sChannel(), mix_log=4)


def _multi():
    alloc = A.TraceLocationAllocator()
    c1, t1 = _wide_fib(10, 100, 1, alloc)
    c2, t2 = _wide_fib(8, 16, 2, alloc)
    c3 = F.MulAddComponent(5, alloc)
    rng = np.random.default_rng(3)
    t3 = [HipCircleEvaluation(CanonicCoset(5).circleDomain(), col(c))
          for c in M.mul_add_trace(rng.integers(0, P, size=32), rng.integers(0, P, size=32))]
    return [c1, c2, c3], t1 + t2 + t3


@pytest.mark.parametrize("blowup", [1, 2])
def test_prove_verify_multi_component(blowup):
    comps, trace = _multi()
    config = PcsConfig(5, FriConfig(0, blowup, 3))
    proof = _commit_and_prove(comps, trace, config, Blake2sChannel())
    _verify(comps, proof, config, Blake2sChannel())


def test_prove_verify_blowup2_wide_fibonacci():
    comp, trace = _wide_fib(9, 100, 5)
    config = PcsConfig(5, FriConfig(0, 2, 3))
    proof = _commit_and_prove([comp], trace, config, Blake2sChannel())
    _verify([comp], proof, config, Blake2sChannel())


def test_prove_verify_poseidon252():
    comps, trace = _multi()
    config = PcsConfig()
    proof = _commit_and_prove(comps, trace, config, Poseidon252Channel(), Poseidon252MerkleChannel)
    _verify(comps, proof, config, Poseidon252Channel(), Poseidon252MerkleChannel)


@pytest.fixture(scope="module")
def honest():
    comp, trace = _wide_fib(7, 100, 11)
    config = PcsConfig()
    return comp, config, _commit_and_prove([comp], trace, config, Blake2sChannel())


def _tampered(proof):
    return StarkProof(copy.deepcopy(proof.commitment_scheme_proof))


def _bump(v):
    t = list(v.tup())
    t[0] = (t[0] + 1) % P
    return q(t)


REJECT = (VerificationError, FriVerificationError)


def test_verify_rejects_tampered_trace_sample(honest):
    comp, config, proof = honest
    bad = _tampered(proof)
    bad.sampled_values[1][5][0] = _bump(bad.sampled_values[1][5][0])
    with pytest.raises(OodsNotMatching):
        _verify([comp], bad, config, Blake2sChannel())


def test_verify_rejects_tampered_composition_sample(honest):
    comp, config, proof = honest
    bad = _tampered(proof)
    bad.sampled_values[2][3][0] = _bump(bad.sampled_values[2][3][0])
    with pytest.raises(OodsNotMatching):
        _verify([comp], bad, config, Blake2sChannel())


def test_verify_rejects_tampered_queried_value(honest):
    comp, config, proof = honest
    bad = _tampered(proof)
    vals = bad.queried_values[1]
    vals[0] = type(vals[0])((vals[0].value + 1) % P)
    with pytest.raises(REJECT):
        _verify([comp], bad, config, Blake2sChannel())


def test_verify_rejects_tampered_root(honest):
    comp, config, proof = honest
    bad = _tampered(proof)
    r = bytearray(bad.commitments[1])
    r[0] ^= 1
    bad.commitments[1] = bytes(r)
    with pytest.raises(REJECT):
        _verify([comp], bad, config, Blake2sChannel())


def test_verify_rejects_other_log_size(honest):
    comp, config, proof = honest
    other = F.WideFibonacciComponent(comp.log_size + 1, comp.n_columns)
    with pytest.raises(REJECT):
        _verify([other], proof, config, Blake2sChannel())
    _verify([comp], proof, config, Blake2sChannel())        # the honest proof still verifies


def test_prove_rejects_broken_trace():
    comp, trace = _wide_fib(6, 20, 4)
    v = trace[13].values.to_numpy()
    v[17] = (int(v[17]) + 1) % P
    trace[13] = HipCircleEvaluation(trace[13].domain, col(v))
    with pytest.raises(ConstraintsNotSatisfied):
        _commit_and_prove([comp], trace, PcsConfig(), Blake2sChannel())


class ReadbackCounter:
    """Counts the library's synchronous read-backs at the C ABI (every entry that hands device results to the host)."""

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


def test_composition_phase_makes_no_readback(monkeypatch):
    comps, trace = _multi()
    config = PcsConfig()
    tw = precompute_twiddles(CanonicCoset(12).circleDomain().halfCoset)
    scheme = CommitmentSchemeProver(config, tw)
    ch = Blake2sChannel()
    for evs in ([], trace):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(ch)
    L.sync()
    counter = ReadbackCounter(monkeypatch)
    alpha = ch.draw_felt()
    poly = A.ComponentProvers(comps).compute_composition_polynomial(alpha, A.Trace.of(scheme), tw)
    tb = scheme.tree_builder()
    tb.extend_polys(poly.into_coordinate_polys())
    tb.commit(ch)                       # ends with the composition root (read by the commit entry itself)
    assert counter.n == 0

"""LogUp on the MI355X: tstwo_logup_column and tstwo_logup_finalize_last against the integer model (tests/logup_model.py), the
trace generator end to end, prove -> verify of the permutation and range-check examples (alone and beside wide Fibonacci), the
rejections, and no read-back in the composition phase of a LogUp proof."""
import copy
import ctypes as C

import numpy as np
import pytest

import logup_model as LM
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd.backend import HipColumn, SecureColumnByCoords
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel
from tstwo_amd.prover import ConstraintsNotSatisfied, InvalidLogupSum, OodsNotMatching, StarkProof, prove, verify

pytestmark = pytest.mark.gpu

P = LM.P


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


def felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def offset_col(a, k):
    """A device column holding `a` that starts k words into its buffer (k = 1: not 16-byte aligned); (buffer, pointer)."""
    buf = HipColumn(np.concatenate([np.zeros(k, dtype=np.uint32), np.asarray(a, dtype=np.uint32)]))
    return buf, buf.ptr + 4 * k


# ------------------------------------------------------------------ tstwo_logup_column against the model
def _column_case(seed, log, n_fracs, n_terms, col_num, with_prev, aligned):
    rng = np.random.default_rng(seed)
    n, k = 1 << log, 0 if aligned else 1
    keep, descs, model = [], (L.LogupFrac * n_fracs)(), []
    for d in descs:
        cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_terms)]
        coeffs = [felt(rng) for _ in range(n_terms)]
        const = felt(rng)
        den = np.zeros((4, n), dtype=np.uint64)
        for j in range(4):
            den[j] = const[j]
            for c, co in zip(cols, coeffs):
                den[j] = (den[j] + co[j] * c) % P
        dcols = [offset_col(c, k) for c in cols]
        tab = L.ptr_array([p for _, p in dcols])
        cw = L.u32x([w for co in coeffs for w in co])
        keep += [dcols, tab, cw]
        d.cols, d.coeffs, d.n_terms = C.cast(tab, C.POINTER(L.vp)), C.cast(cw, L.u32p), n_terms
        d.constant[:] = list(const)
        if col_num:
            num = rng.integers(0, P, size=n, dtype=np.uint64)
            buf, ptr = offset_col(num, k)
            keep.append(buf)
            d.num, d.num_const = ptr, 0
        else:
            c = int(rng.integers(0, P))
            num = np.full(n, c, dtype=np.uint64)
            d.num, d.num_const = None, c
        model.append((num, den))
    prev = rng.integers(0, P, size=(4, n), dtype=np.uint64) if with_prev else np.zeros((4, n), dtype=np.uint64)
    dprev = [offset_col(prev[j], k) for j in range(4)] if with_prev else None
    dout = [offset_col(np.zeros(n), k) for _ in range(4)]
    L.call("tstwo_logup_column", descs, n_fracs, L.p4([p for _, p in dprev]) if with_prev else None, log,
           L.p4([p for _, p in dout]))
    L.call("tstwo_check_zero_flag")
    out = np.stack([b.to_numpy()[k:].astype(np.uint64) for b, _ in dout])
    assert LM.column_identity_holds(out, prev, model)
    if log <= 6:
        assert np.array_equal(out, LM.column(model, prev if with_prev else None, n))


COLUMN_CASES = [
    # (log, n_fracs, n_terms, column numerator, prev, aligned)
    (1, 1, 1, False, False, True), (2, 1, 2, True, True, True), (3, 2, 1, True, False, False), (5, 8, 16, True, True, True),
    (6, 3, 4, False, True, False), (10, 2, 2, True, True, True), (12, 1, 4, False, False, True), (14, 4, 3, True, True, False),
    (16, 2, 4, True, True, True), (18, 1, 1, True, False, True), (20, 2, 2, False, True, True), (22, 1, 2, True, True, True),
    (9, 7, 9, True, True, True), (11, 5, 16, False, False, True),
]


@pytest.mark.parametrize("log,n_fracs,n_terms,col_num,with_prev,aligned", COLUMN_CASES)
def test_logup_column_matches_the_model(log, n_fracs, n_terms, col_num, with_prev, aligned):
    _column_case(1000 + 7 * log + n_fracs, log, n_fracs, n_terms, col_num, with_prev, aligned)


def _gen_one(log, a, num=1):
    le = LG.LookupElements(q((3, 4, 5, 6)), q((7, 8, 9, 10)), 2)
    gen = LG.LogupTraceGenerator(log)
    col = gen.new_col()
    col.write_frac(num, le.combine_columns([HipColumn(a)]))
    col.finalize_col()
    return gen


def test_zero_denominator_raises():
    # alpha^0 a - z = 0 where a = z (z has zero i, u, iu coordinates)
    n = 64
    a = np.full(n, 5, dtype=np.uint32)
    le = LG.LookupElements(q((5, 0, 0, 0)), q((1, 2, 3, 4)), 1)
    gen = LG.LogupTraceGenerator(6)
    col = gen.new_col()
    col.write_frac(1, le.combine_columns([HipColumn(a)]))
    col.finalize_col()
    with pytest.raises(L.TstwoError, match="0 has no inverse"):
        gen.finalize_last()
    _gen_one(6, np.arange(n, dtype=np.uint32) + 100).finalize_last()          # the flag was cleared


def test_logup_column_argument_errors():
    n = 16
    a = HipColumn(np.arange(n, dtype=np.uint32))
    out = SecureColumnByCoords.zeros(n)
    form = LG.LinearForm([(QM31.one(), a)], QM31.one())
    with pytest.raises(ValueError):
        LG.logup_column([(1, form)] * 9, None, 4, out)
    with pytest.raises(ValueError):
        LG.logup_column([(1, LG.LinearForm([(QM31.one(), a)] * 17, QM31.one()))], None, 4, out)
    descs = (L.LogupFrac * 9)()
    with pytest.raises(L.TstwoError, match="fractions"):
        L.call("tstwo_logup_column", descs, 9, None, 4, out.ptrs())
    descs = (L.LogupFrac * 1)()
    tab = L.ptr_array([a.ptr] * 17)
    cw = L.u32x([1] * 68)
    descs[0].cols, descs[0].coeffs, descs[0].n_terms = C.cast(tab, C.POINTER(L.vp)), C.cast(cw, L.u32p), 17
    with pytest.raises(L.TstwoError, match="terms"):
        L.call("tstwo_logup_column", descs, 1, None, 4, out.ptrs())
    descs[0].n_terms = 1
    descs[0].constant[:] = [P, 0, 0, 0]
    with pytest.raises(L.TstwoError, match="out of range"):
        L.call("tstwo_logup_column", descs, 1, None, 4, out.ptrs())
    with pytest.raises(L.TstwoError, match="log_size"):
        L.call("tstwo_logup_finalize_last", out.ptrs(), 0, (C.c_uint32 * 4)())


def _capture(fn):
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="graph capture"):
            fn()
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)


def test_entries_are_refused_during_graph_capture():
    n = 64
    a = HipColumn(np.arange(n, dtype=np.uint32) + 9)
    out = SecureColumnByCoords.zeros(n)
    form = LG.LinearForm([(q((1, 2, 3, 4)), a)], q((5, 6, 7, 8)))
    _capture(lambda: LG.logup_column([(1, form)], None, 6, out))
    _capture(lambda: LG.logup_finalize_last(out, 6))
    LG.logup_column([(1, form)], None, 6, out)
    LG.logup_finalize_last(out, 6)


# ------------------------------------------------------------------ finalize_last against the model
@pytest.mark.parametrize("log", [1, 2, 3, 4, 7, 11, 12, 13, 14, 15, 17, 20, 22, 24])
def test_finalize_last_matches_the_model(log):
    rng = np.random.default_rng(50 + log)
    n = 1 << log
    col = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want, claimed = LM.finalize_last(col, log)
    dev = SecureColumnByCoords([HipColumn(col[j].astype(np.uint32)) for j in range(4)])
    got = LG.logup_finalize_last(dev, log)
    assert got.tup() == claimed
    for j in range(4):
        assert np.array_equal(dev.columns[j].to_numpy(), want[j].astype(np.uint32)), j
    assert all(int(want[j][LM.position(n - 1, log)]) == 0 for j in range(4))


def test_finalize_last_unaligned():
    rng = np.random.default_rng(77)
    log = 15
    n = 1 << log
    col = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    want, claimed = LM.finalize_last(col, log)
    bufs = [offset_col(col[j], 1) for j in range(4)]
    out = (C.c_uint32 * 4)()
    L.call("tstwo_logup_finalize_last", L.p4([p for _, p in bufs]), log, out)
    assert tuple(out) == claimed
    for j in range(4):
        assert np.array_equal(bufs[j][0].to_numpy()[1:], want[j].astype(np.uint32))


# ------------------------------------------------------------------ the generator end to end
@pytest.mark.parametrize("log", [10, 20])
def test_generator_end_to_end(log):
    rng = np.random.default_rng(log)
    n = 1 << log
    z, alpha = felt(rng), felt(rng)
    le = LG.LookupElements(q(z), q(alpha), 3)
    a, b, c, m = (rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(4))
    gen = LG.LogupTraceGenerator(log)
    c0 = gen.new_col()
    c0.write_frac(HipColumn(m.astype(np.uint32)), le.combine_columns([HipColumn(a.astype(np.uint32)), 7, HipColumn(b.astype(np.uint32))]))
    c0.write_frac(3, le.combine_columns([HipColumn(c.astype(np.uint32))]))
    c0.finalize_col()
    c1 = gen.new_col()
    c1.write_frac(P - 1, le.combine_columns([HipColumn(b.astype(np.uint32)), HipColumn(c.astype(np.uint32))]))
    c1.finalize_col()
    evals, claimed = gen.finalize_last()
    assert len(evals) == 8 and all(e.domain == CanonicCoset(log).circleDomain() for e in evals)
    f0 = [(m, LM.combine_cols(z, alpha, [a, 7, b], n)), (np.full(n, 3, dtype=np.uint64), LM.combine_cols(z, alpha, [c], n))]
    col0 = np.stack([evals[j].values.to_numpy().astype(np.uint64) for j in range(4)])
    assert LM.column_identity_holds(col0, np.zeros((4, n), dtype=np.uint64), f0)
    last = np.stack([evals[4 + j].values.to_numpy().astype(np.uint64) for j in range(4)])
    # undo the scan: the row values of the last column before finalize_last
    pos = LM.positions(log)
    inv_n = pow(n, P - 2, P)
    s = [v * inv_n % P for v in claimed.tup()]
    raw = np.empty_like(last)
    for j in range(4):
        seq = last[j][pos]
        d = (seq + P - np.concatenate([[0], seq[:-1]]).astype(np.uint64)) % P
        raw[j][pos] = (d + s[j]) % P
    assert tuple(int(v) for v in raw.sum(axis=1, dtype=np.uint64) % P) == claimed.tup()
    f1 = [(np.full(n, P - 1, dtype=np.uint64), LM.combine_cols(z, alpha, [b, c], n))]
    assert LM.column_identity_holds(raw, col0, f1)


# ------------------------------------------------------------------ prove / verify
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, HipColumn(np.asarray(c, dtype=np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def _permutation(log, rng, channel, scheme, alloc=None, permute=True, claimed_override=None):
    a = rng.integers(0, P, size=1 << log, dtype=np.uint32)
    b = rng.permutation(a) if permute else rng.integers(0, P, size=1 << log, dtype=np.uint32)
    return a, b


def _prove_permutation(log, channel_cls=Blake2sChannel, merkle=None, permute=True, claimed_override=None, config=None):
    rng = np.random.default_rng(log)
    config = config or PcsConfig()
    a, b = _permutation(log, rng, None, None, permute=permute)
    tw = precompute_twiddles(CanonicCoset(log + 2 + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    ch = channel_cls()
    scheme = CommitmentSchemeProver(config, tw, merkle)
    _commit(scheme, [], ch)
    _commit(scheme, _evals([a, b], log), ch)
    le = LG.LookupElements.draw(ch, 1)
    inter, claimed = F.permutation_interaction_trace(log, a, b, le)
    ch.mix_felts([claimed])
    _commit(scheme, inter, ch)
    comp = F.FrameworkComponent(F.PermutationEval(log, le), claimed_sum=claimed if claimed_override is None else claimed_override)
    return comp, prove([comp], ch, scheme), config, claimed


def _verify_permutation(log, comp, proof, config, channel_cls=Blake2sChannel, merkle=None, logup_sum=QM31.zero()):
    ch = channel_cls()
    v = CommitmentSchemeVerifier(config, merkle)
    sizes = A.Components([comp], 0).column_log_sizes()
    v.commit(proof.commitments[0], [], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    le = LG.LookupElements.draw(ch, 1)
    assert le.z == comp.eval.lookup_elements.z
    ch.mix_felts([comp.claimed_sum])
    v.commit(proof.commitments[2], sizes[2], ch)
    verify([comp], ch, v, proof, logup_sum)


@pytest.mark.parametrize("log", [4, 8, 12])
def test_prove_verify_permutation_blake2s(log):
    comp, proof, config, claimed = _prove_permutation(log)
    assert claimed == QM31.zero()
    assert [len(c) for c in proof.sampled_values[2]] == [2, 2, 2, 2]
    _verify_permutation(log, comp, proof, config)


def test_prove_verify_permutation_poseidon252():
    comp, proof, config, _ = _prove_permutation(6, Poseidon252Channel, Poseidon252MerkleChannel)
    _verify_permutation(6, comp, proof, config, Poseidon252Channel, Poseidon252MerkleChannel)


def test_non_permutation_gives_invalid_logup_sum():
    comp, proof, config, claimed = _prove_permutation(6, permute=False)
    assert claimed != QM31.zero()
    with pytest.raises(InvalidLogupSum):
        _verify_permutation(6, comp, proof, config)


def test_wrong_claimed_sum_is_not_provable():
    with pytest.raises(ConstraintsNotSatisfied):
        _prove_permutation(6, claimed_override=QM31.from_u32_unchecked(1, 0, 0, 0))


def test_tampered_interaction_sample_is_rejected():
    comp, proof, config, _ = _prove_permutation(6)
    bad = StarkProof(copy.deepcopy(proof.commitment_scheme_proof))
    t = list(bad.sampled_values[2][0][0].tup())
    t[0] = (t[0] + 1) % P
    bad.sampled_values[2][0][0] = q(t)                    # column 0 of the interaction tree at offset -1
    with pytest.raises(OodsNotMatching):
        _verify_permutation(6, comp, bad, config)


def _range_check(log_range, log_values, rng, extra=None, blowup=1):
    """Table + values components (and `extra` main columns after them), committed by the caller protocol."""
    config = PcsConfig(5, FriConfig(0, blowup, 3))
    v0 = rng.integers(0, 1 << log_range, size=1 << log_values)
    v1 = rng.integers(0, 1 << log_range, size=1 << log_values)
    mult = F.range_check_multiplicities(log_range, v0, v1)
    max_log = max(log_range + 1, log_values + 2, 10)
    tw = precompute_twiddles(CanonicCoset(max_log + blowup).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    _commit(scheme, _evals([F.range_check_table_column(log_range)], log_range), ch)
    main = _evals([mult], log_range) + _evals([v0, v1], log_values)
    if extra is not None:
        main += extra[1]
    _commit(scheme, main, ch)
    le = LG.LookupElements.draw(ch, 1)
    t_inter, t_sum = F.range_check_table_interaction_trace(log_range, mult, le)
    v_inter, v_sum = F.range_check_values_interaction_trace(log_values, v0.astype(np.uint32), v1.astype(np.uint32), le)
    ch.mix_felts([t_sum, v_sum])
    _commit(scheme, t_inter + v_inter, ch)
    alloc = A.TraceLocationAllocator()
    table = F.FrameworkComponent(F.RangeCheckTableEval(log_range, le), alloc, [0], claimed_sum=t_sum)
    values = F.FrameworkComponent(F.RangeCheckValuesEval(log_values, le), alloc, claimed_sum=v_sum)
    comps = [table, values] + ([extra[0](alloc)] if extra is not None else [])
    proof = prove(comps, ch, scheme)
    assert t_sum.add(v_sum) == QM31.zero()
    # verify
    ch = Blake2sChannel()
    v = CommitmentSchemeVerifier(config)
    sizes = A.Components(comps, 1).column_log_sizes()
    v.commit(proof.commitments[0], [log_range], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    LG.LookupElements.draw(ch, 1)
    ch.mix_felts([t_sum, v_sum])
    v.commit(proof.commitments[2], sizes[2], ch)
    verify(comps, ch, v, proof)


def test_prove_verify_range_check_pair():
    _range_check(8, 9, np.random.default_rng(3))


@pytest.mark.parametrize("blowup", [1, 2])
def test_prove_verify_logup_beside_wide_fibonacci(blowup):
    rng = np.random.default_rng(11)
    wf_main = A.generate_wide_fib_trace(8, rng.integers(0, P, size=1 << 8), rng.integers(0, P, size=1 << 8), 20)
    _range_check(6, 7, rng, extra=(lambda alloc: F.WideFibonacciComponent(8, 20, alloc), wf_main), blowup=blowup)


class ReadbackCounter:
    SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_gkr_sum_poly", "tstwo_gather_words",
                  "tstwo_eval_at_point", "tstwo_eval_at_point_batch", "tstwo_check_zero_flag", "tstwo_logup_finalize_last"}

    def __init__(self, monkeypatch):
        self.n = 0
        orig_call = L.call

        def call(name, *a):
            if name in self.SYNC_CALLS:
                self.n += 1
            return orig_call(name, *a)
        monkeypatch.setattr(L, "call", call)


def test_logup_composition_phase_makes_no_readback(monkeypatch):
    log = 10
    rng = np.random.default_rng(5)
    a = rng.integers(0, P, size=1 << log, dtype=np.uint32)
    b = rng.permutation(a)
    tw = precompute_twiddles(CanonicCoset(log + 3).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(PcsConfig(), tw)
    _commit(scheme, [], ch)
    _commit(scheme, _evals([a, b], log), ch)
    le = LG.LookupElements.draw(ch, 1)
    inter, claimed = F.permutation_interaction_trace(log, a, b, le)
    ch.mix_felts([claimed])
    _commit(scheme, inter, ch)
    comp = F.FrameworkComponent(F.PermutationEval(log, le), claimed_sum=claimed)
    L.sync()
    counter = ReadbackCounter(monkeypatch)
    alpha = ch.draw_felt()
    poly = A.ComponentProvers([comp], 0).compute_composition_polynomial(alpha, A.Trace.of(scheme), tw)
    tb = scheme.tree_builder()
    tb.extend_polys(poly.into_coordinate_polys())
    tb.commit(ch)
    assert counter.n == 0

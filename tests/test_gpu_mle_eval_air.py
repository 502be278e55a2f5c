"""-m gpu: the device side of the mle_eval component.  tstwo_mle_eval_selectors and tstwo_mle_eval_terms bit for bit against the
integer model (tests/mle_eval_air_model.py) inside guard bands (tests/arena.py), at the sizes where the launch code changes its
path: one lane, several lanes, more than one workgroup, unaligned columns (one row per lane) and the smallest sizes at which the
grid-stride loop takes a second trip (csrc/mle_eval_air.hip: kMaxBlocks = 8192 workgroups of 256 lanes, so 2^24 rows at four rows
per lane and 2^22 at one); every refusal with its text and untouched outputs; the calls back to back behind a plug
(tests/sequence.py); and the component itself: assert_constraints on an honest trace and on a trace with one changed cell,
interpreted and native."""

import numpy as np
import pytest

import gkr_model as G
import mle_eval_air_model as M
import sequence as SQ
from arena import Arena, rin, rinout, rout
from saturation import SAT, SAT4
from tstwo_amd import _lib as L
from tstwo_amd import constraint_framework as F
from tstwo_amd import mle_eval as ME
from tstwo_amd.backend import HipColumn
from tstwo_amd.fields import QM31
from tstwo_amd.gkr import GkrInputClaimMismatch
from tstwo_amd.prover import ConstraintViolation

pytestmark = pytest.mark.gpu

P = M.P
BAD_ARG = 7                     # TSTWO_ERR_BAD_ARG
LANES_PER_TRIP = 8192 * 256     # csrc/mle_eval_air.hip: kMaxBlocks * kThreads


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*[int(v) for v in t])


# ------------------------------------------------------------------ tstwo_mle_eval_selectors
@pytest.mark.parametrize("log,offset", [(2, 0), (3, 0), (4, 0), (5, 0), (9, 0), (2, 4), (5, 8), (9, 12)])
def test_selectors_match_the_model(log, offset):
    n_cols = 2 * log + 2
    names = [f"s{c}" for c in range(n_cols)]
    with Arena([rout(nm, 1 << log, offset) for nm in names]) as ar:
        L.call("tstwo_mle_eval_selectors", log, ar.ptrs(names))
        got = ar.check()
    want = M.selectors_vec(log)
    for c, nm in enumerate(names):
        assert np.array_equal(got[nm], want[c]), (log, c)
    if log <= 5:
        assert np.array_equal(want, np.stack(M.selectors(log)).astype(np.uint32))


def test_selectors_refusals():
    cols = [HipColumn(np.full(16, 7, dtype=np.uint32)) for _ in range(10)]
    tab = L.ptr_array([c.ptr for c in cols])
    for log in (0, 1, 29):
        with pytest.raises(L.TstwoError, match="^mle eval selectors: log_size must be 2 to 28") as e:
            L.call("tstwo_mle_eval_selectors", log, tab)
        assert e.value.code == BAD_ARG
    with pytest.raises(L.TstwoError, match="^mle eval selectors: null host argument"):
        L.call("tstwo_mle_eval_selectors", 4, None)
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        L.call("tstwo_mle_eval_selectors", 4, L.ptr_array([c.ptr for c in cols[:9]] + [0]))
    with pytest.raises(L.TstwoError, match="^mle eval selectors: two output columns overlap"):
        L.call("tstwo_mle_eval_selectors", 4, L.ptr_array([c.ptr for c in cols[:9]] + [cols[3].ptr + 32]))
    assert all((c.to_numpy() == 7).all() for c in cols)
    L.call("tstwo_mle_eval_selectors", 4, tab)
    assert np.array_equal(np.stack([c.to_numpy() for c in cols]), M.selectors_vec(4))


# ------------------------------------------------------------------ tstwo_mle_eval_terms
def _terms_case(log, n_terms, offset=0, zero_const=False, sat=False, alias=False, sample=None, seed=0):
    rng = np.random.default_rng(100 * log + n_terms + seed)
    n = 1 << log
    if sat:                                   # 2^31 - 2 in every position: columns, coefficients, constant and eq
        cols = [np.full(n, SAT, dtype=np.uint32) for _ in range(n_terms)]
        coeffs, constant = [SAT4] * n_terms, SAT4
        eq = np.full((4, n), SAT, dtype=np.uint32)
    else:
        cols = [rng.integers(0, P, size=n, dtype=np.uint32) for _ in range(n_terms)]
        coeffs = [G.random_felt(rng) for _ in range(n_terms)]
        constant = (0, 0, 0, 0) if zero_const else G.random_felt(rng)
        eq = rng.integers(0, P, size=(4, n), dtype=np.uint32)
    cn, en, on = [f"c{k}" for k in range(n_terms)], [f"e{j}" for j in range(4)], [f"o{j}" for j in range(4)]
    regions = [rin(nm, c, offset) for nm, c in zip(cn, cols)]
    regions += [(rinout if alias else rin)(nm, eq[j], offset) for j, nm in enumerate(en)]
    if not alias:
        regions += [rout(nm, n, offset) for nm in on]
    with Arena(regions) as ar:
        L.call("tstwo_mle_eval_terms", ar.p4(en), ar.ptrs(cn), L.u32x([w for c in coeffs for w in c]), n_terms, L.u32x(constant), log,
               ar.p4(en if alias else on))
        got = ar.check()
    out = np.stack([got[nm] for nm in (en if alias else on)])
    assert (out < P).all()                                         # every word written, with a canonical value
    idx = np.arange(n) if sample is None else sample
    want = M.terms(eq[:, idx], [c[idx] for c in cols], coeffs, constant)
    assert np.array_equal(out[:, idx], want.astype(np.uint32))


TERMS_CASES = [
    # (log, n_terms, byte offset from a 16-byte boundary, zero constant, saturated, out is eq)
    (0, 1, 0, False, False, False), (2, 1, 0, False, False, False), (2, 16, 0, True, False, True), (3, 2, 0, False, False, False),
    (3, 1, 4, False, False, True), (5, 16, 0, False, False, False), (5, 2, 8, True, False, False), (5, 1, 0, False, True, False),
    (5, 16, 0, False, True, True), (10, 1, 0, False, False, True), (10, 2, 0, True, False, False), (10, 16, 0, False, False, False),
    (10, 16, 12, False, True, False), (10, 4, 4, False, False, True), (10, 5, 0, False, True, True),
]


@pytest.mark.parametrize("log,n_terms,offset,zero_const,sat,alias", TERMS_CASES)
def test_terms_match_the_model(log, n_terms, offset, zero_const, sat, alias):
    _terms_case(log, n_terms, offset, zero_const, sat, alias)


def _trip_sample(n, rows_per_trip):
    rng = np.random.default_rng(n)
    edge = np.arange(-2048, 2048) + rows_per_trip
    return np.unique(np.concatenate([np.arange(2048), edge, np.arange(n - 2048, n), rng.integers(0, n, size=1 << 15)]))


@pytest.mark.parametrize("log,offset,alias", [(22, 4, False), (24, 0, True)])
def test_terms_second_trip_of_the_grid_stride_loop(log, offset, alias):
    """One row per lane (unaligned) wraps at 2^21 rows, four rows per lane at 2^23: the sizes here are the first powers of two
    above them.  The model is compared on the rows around the wrap, both ends and a random sample; every word must be canonical."""
    rows_per_trip = LANES_PER_TRIP * (1 if offset else 4)
    assert rows_per_trip < 1 << log <= 2 * rows_per_trip and (1 << (log - 1)) <= rows_per_trip
    _terms_case(log, 1, offset, alias=alias, sample=_trip_sample(1 << log, rows_per_trip))


def test_terms_refusals_leave_the_outputs_untouched():
    n, log = 64, 6
    rng = np.random.default_rng(3)
    cols = [HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(17)]
    eq = [HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(4)]
    out = [HipColumn(np.full(n, 12345, dtype=np.uint32)) for _ in range(4)]
    eq_before = [c.to_numpy().copy() for c in eq]
    e4, o4 = L.p4([c.ptr for c in eq]), L.p4([c.ptr for c in out])
    tab = L.ptr_array([c.ptr for c in cols])
    ok_c, ok_k = L.u32x([1, 2, 3, 4] * 17), L.u32x([5, 6, 7, 8])
    big_c, big_k = L.u32x([1, 2, 3, 4] * 16 + [0, 0, P, 0]), L.u32x([0, 0, 0, P])
    cases = [
        ("1 to 16 terms", (e4, tab, ok_c, 0, ok_k, log, o4)),
        ("1 to 16 terms", (e4, tab, ok_c, 17, ok_k, log, o4)),
        ("log_size above 28", (e4, tab, ok_c, 1, ok_k, 29, o4)),
        ("null host argument", (e4, None, ok_c, 1, ok_k, log, o4)),
        ("null host argument", (e4, tab, None, 1, ok_k, log, o4)),
        ("null host argument", (e4, tab, ok_c, 1, None, log, o4)),
        ("coefficient word out of range", (e4, L.ptr_array([c.ptr for c in cols[1:]]), L.u32x(list(big_c)[4:]), 16, ok_k, log, o4)),
        ("constant out of range", (e4, tab, ok_c, 2, big_k, log, o4)),
        ("an output column is also an input", (e4, L.ptr_array([cols[0].ptr, out[2].ptr + 4 * (n - 1)]), ok_c, 2, ok_k, log, o4)),
        ("out may alias eq only column for column", (e4, tab, ok_c, 1, ok_k, log, L.p4([eq[1].ptr, eq[0].ptr, out[2].ptr, out[3].ptr]))),
        ("out may alias eq only column for column", (e4, tab, ok_c, 1, ok_k, log, L.p4([eq[0].ptr + 16, out[1].ptr, out[2].ptr, out[3].ptr]))),
        ("two output columns overlap", (e4, tab, ok_c, 1, ok_k, log, L.p4([out[0].ptr, out[0].ptr, out[2].ptr, out[3].ptr]))),
    ]
    for text, args in cases:
        with pytest.raises(L.TstwoError, match="^mle eval terms: " + text) as e:
            L.call("tstwo_mle_eval_terms", *args)
        assert e.value.code == BAD_ARG, text
    for bad in (L.p4([eq[0].ptr, 0, eq[2].ptr, eq[3].ptr]),):
        with pytest.raises(L.TstwoError, match="null device pointer in table"):
            L.call("tstwo_mle_eval_terms", bad, tab, ok_c, 1, ok_k, log, o4)
        with pytest.raises(L.TstwoError, match="null device pointer in table"):
            L.call("tstwo_mle_eval_terms", e4, tab, ok_c, 1, ok_k, log, L.p4([out[0].ptr, out[1].ptr, 0, out[3].ptr]))
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        L.call("tstwo_mle_eval_terms", e4, L.ptr_array([cols[0].ptr, 0]), ok_c, 2, ok_k, log, o4)
    assert all((c.to_numpy() == 12345).all() for c in out)
    assert all(np.array_equal(c.to_numpy(), b) for c, b in zip(eq, eq_before))
    # the zero flag is not touched: a form that vanishes everywhere is a legal input
    L.call("tstwo_mle_eval_terms", e4, tab, L.u32x([0] * 64), 16, L.u32x([0] * 4), log, o4)
    L.call("tstwo_check_zero_flag")
    assert all((c.to_numpy() == 0).all() for c in out)


# ------------------------------------------------------------------ back to back behind a plug
def _op_selectors(s, log):
    outs = [s.buf(1 << log, kind="m31") for _ in range(2 * log + 2)]
    s.add(SQ.Op("tstwo_mle_eval_selectors", [], outs, lambda A: L.call("tstwo_mle_eval_selectors", log, L.ptr_array([A(x) for x in outs])),
                lambda S: dict(zip(outs, M.selectors_vec(log)))))
    return outs


def _op_terms(s, eq4, cols, log, rng, in_place):
    coeffs, constant = [G.random_felt(rng) for _ in cols], G.random_felt(rng)
    o4 = eq4 if in_place else [s.buf(1 << log, kind="m31") for _ in range(4)]
    s.add(SQ.Op("tstwo_mle_eval_terms", eq4 + cols, o4,
                lambda A: L.call("tstwo_mle_eval_terms", L.p4([A(x) for x in eq4]), L.ptr_array([A(x) for x in cols]),
                                 L.u32x([w for c in coeffs for w in c]), len(cols), L.u32x(constant), log, L.p4([A(x) for x in o4])),
                lambda S: dict(zip(o4, SQ.coords(M.terms(np.stack([S[x] for x in eq4]), [S[c] for c in cols], coeffs, constant))))))
    return o4


def test_two_calls_back_to_back_behind_a_plug():
    """eq table -> terms into new columns -> terms in place over those, with the selectors between them: nothing synchronises
    between the calls, and the second terms call reads what the first one wrote."""
    rng = np.random.default_rng(11)
    log = 10
    s = SQ.Seq()
    sel = _op_selectors(s, log)
    eq4 = SQ.gkr_gen_eq_evals(s, M.random_point(rng, log), G.ONE)
    cols = SQ.rand_cols(s, rng, 3, 1 << log)
    t4 = _op_terms(s, eq4, cols, log, rng, in_place=False)
    _op_selectors(s, 3)
    _op_terms(s, t4, cols[:1] + sel[:2], log, rng, in_place=True)
    plug = SQ.Plug()
    try:
        SQ.run(s, plug)
    finally:
        plug.free()


# ------------------------------------------------------------------ the component on the device
def _statement(log, seed=0, n_terms=2):
    """An honest statement: the model's columns and claim, and the device columns of the component."""
    rng = np.random.default_rng(7 * log + seed)
    point = M.random_point(rng, log)
    cols = [G.random_base(rng, 1 << log) for _ in range(n_terms)]
    coeffs, constant = [G.random_felt(rng) for _ in range(n_terms)], G.random_felt(rng)
    e, s, claim = M.interaction_trace(point, cols, coeffs, constant)
    form = ME.MleEvalForm([(q(w), ("main", i)) for i, w in enumerate(coeffs)], q(constant))
    ev = ME.MleEvalEval(log, [q(r) for r in point], q(claim), form)
    main = [HipColumn(c.astype(np.uint32)) for c in cols]
    return point, cols, coeffs, constant, e, s, claim, ev, main


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("log", [2, 3, 5, 8])
def test_assert_constraints_on_an_honest_and_on_a_changed_trace(log, native):
    point, cols, coeffs, constant, e, s, claim, ev, main = _statement(log)
    comp = F.FrameworkComponent(ev, None, list(range(2 * log + 2)), native=native)
    assert (comp.native is not None) == native
    sel = ME.mle_eval_selector_columns(log)
    inter = ME.mle_eval_interaction_trace(ev.point, ev.claim, ev.form.on_columns(main))
    got = np.stack([c.values.to_numpy() for c in inter])
    assert np.array_equal(got[:4], e.astype(np.uint32)) and np.array_equal(got[4:], s.astype(np.uint32))
    comp.assert_constraints(main, sel, inter)
    rows = np.empty(1 << log, dtype=np.int64)
    rows[M.LM.positions(log)] = np.arange(1 << log)
    msel = M.selectors(log)
    for which, coord, p in ((0, 1, (1 << log) - 2), (1, 2, 1)):                # one cell of E, one cell of S
        e2, s2 = e.copy(), s.copy()
        (e2 if which == 0 else s2)[coord, p] = ((e2 if which == 0 else s2)[coord, p] + 1) % P
        changed = [HipColumn(c.astype(np.uint32)) for c in list(e2) + list(s2)]
        want = []
        for k, c in enumerate(M.constraints(log, point, claim, cols, coeffs, constant, e2, s2, msel)):
            fr = M.failing_rows(c)
            if len(fr):
                want.append((k, len(fr), int(rows[fr].min())))
        assert [tuple(f) for f in comp.constraint_failures(main, sel, changed)] == want
        first = 0 if which == 0 else 2                                           # constraint 1 (step) or 3 (sum) of DESIGN §4.5
        assert want[0][0] == first
        with pytest.raises(ConstraintViolation) as err:
            comp.assert_constraints(main, sel, changed)
        assert (err.value.constraint, err.value.row, err.value.n_rows) == (first, want[0][2], want[0][1])


def test_interaction_trace_refuses_a_wrong_claim_and_a_degenerate_point():
    point, cols, coeffs, constant, e, s, claim, ev, main = _statement(4, seed=1)
    wrong = q(tuple((v + 1) % P for v in claim))
    with pytest.raises(GkrInputClaimMismatch):
        ME.mle_eval_interaction_trace(ev.point, wrong, ev.form.on_columns(main))
    bad = list(ev.point)
    bad[2] = QM31.one()
    with pytest.raises(ValueError, match="coordinate 2"):
        ME.mle_eval_interaction_trace(bad, ev.claim, ev.form.on_columns(main))
    # the claim is the MLE of the form at the point, as the GKR side evaluates it
    from tstwo_amd.gkr import Mle
    form_mle = Mle.secure(M.form_values(cols, coeffs, constant, 16).astype(np.uint32))
    assert form_mle.eval_at_point(ev.point).tup() == claim

"""The round model (tests/gkr_round_model.py) without a GPU: chained over a layer it is gkr_model.sumcheck_prove_batch — which the
reference's vectors pin (test_cpu_gkr.py) — in round polynomials, assignment, final claims and channel digest; its batched
inv_eq0 table is the direct inverses; its degenerate eq points are exactly where it raises.  The product's host helpers
(gkr.inv_eq0_table, gkr.DEGENERATE_EQ_POINTS) agree with the model's."""
import numpy as np
import pytest

import gkr_model as M
import gkr_round_model as R
from tstwo_amd import gkr as G


def make_layer(rng, kind, n_vars):
    n = 1 << n_vars
    num = {M.GENERIC: M.random_secure(rng, n), M.MULT: M.random_base(rng, n)}.get(kind)
    return {"kind": kind, "num": num, "den": M.random_secure(rng, n)}


def oracles_for(rng, shapes, n):
    """Oracles of one GKR layer with n rounds: shapes = [(kind, oracle variables)]; 0 variables = a constant oracle."""
    y = [M.random_felt(rng) for _ in range(n)]
    eqe = M.eq_evals_generate(y)
    lam = M.random_felt(rng)
    return [M.Oracle(eqe, list(y), make_layer(rng, kind, n_v + 1), M.ONE, lam) for kind, n_v in shapes]


BATCHES = [
    ([(M.GENERIC, 5)], 5),
    ([(M.GP, 4), (M.SINGLES, 4)], 4),
    ([(M.GENERIC, 6), (M.GP, 2), (M.SINGLES, 4), (M.MULT, 1)], 6),           # instances joining in later rounds
    ([(M.GP, 0), (M.GENERIC, 3), (M.SINGLES, 0)], 3),                         # constant instances first and last
    ([(M.MULT, 5), (M.GENERIC, 0), (M.GP, 5), (M.SINGLES, 1)], 5),
    ([(M.SINGLES, 1)], 1),
]


@pytest.mark.parametrize("case", range(len(BATCHES)))
def test_chained_round_model_is_the_sumcheck_model(case):
    shapes, n = BATCHES[case]
    rng = np.random.default_rng(900 + case)
    oracles = oracles_for(rng, shapes, n)
    claims = [M.random_felt(rng) for _ in oracles]
    alpha = M.random_felt(rng)
    start = M.Channel()
    start.mix_felts([M.random_felt(rng)])
    a, b = M.Channel(), M.Channel()
    a.digest = b.digest = start.digest
    # any claim passes the model's own round check: r(1) is defined as claim - r(0), and a waiting instance sends claim / 2 twice
    want_polys, want_assign, _, want_claims = M.sumcheck_prove_batch(claims, oracles, alpha, a)
    got_polys, got_assign, got_claims = R.layer_by_rounds(claims, oracles, alpha, b)
    assert got_polys == want_polys
    assert got_assign == want_assign
    assert got_claims == want_claims
    assert (b.digest, b.n_sent) == (a.digest, a.n_sent)


def test_round_model_corrections_follow_the_oracle():
    rng = np.random.default_rng(77)
    (o,) = oracles_for(rng, [(M.GENERIC, 4)], 4)
    ch = M.Channel()
    claims, corrs = [M.random_felt(rng)], [M.ONE]
    lay = o.layer
    for rnd in range(4):
        rem = 4 - rnd
        sums = [M.sum_f0_f2(lay, o.eq_evals, rem, o.lam)]
        _, c, claims, corrs = R.round_finish(ch, sums, claims, corrs, [True], o.y, rem, M.random_felt(rng))
        o = o.fix_first_variable(c)
        lay = o.layer
        assert corrs == [o.correction]


@pytest.mark.parametrize("n", [0, 1, 2, 5, 13])
def test_inv_eq0_table_is_the_direct_inverses(n):
    rng = np.random.default_rng(40 + n)
    y = [M.random_felt(rng) for _ in range(n)]
    assert R.inv_eq0_table(y) == R.inv_eq0_direct(y)
    assert G.inv_eq0_table(y) == R.inv_eq0_direct(y)


def test_inv_eq0_table_zero_eq_raises():
    rng = np.random.default_rng(41)
    y = [M.random_felt(rng), M.ONE, M.random_felt(rng)]
    with pytest.raises(ZeroDivisionError):
        R.inv_eq0_table(y)
    with pytest.raises(ZeroDivisionError, match="0 has no inverse"):
        G.inv_eq0_table(y)


def test_degenerate_eq_points_are_exactly_where_the_model_raises():
    P = M.P
    assert set(R.DEGENERATE_Y) == {(0, 0, 0, 0), (1, 0, 0, 0), (1 << 30, 0, 0, 0), (0x55555555, 0, 0, 0)}
    assert set(G.DEGENERATE_EQ_POINTS) == set(R.DEGENERATE_Y)
    rng = np.random.default_rng(5)
    f0, f2, claim, a = (M.random_felt(rng) for _ in range(4))
    for y in R.DEGENERATE_Y:
        with pytest.raises(ZeroDivisionError):
            R.corrected_poly(f0, f2, claim, y, a)
    # neighbours of the four, values that differ from them in one coordinate only, and the rest of the small rationals
    others = [M.qm(2), M.qm(3), M.qm(P - 1), M.qm(P - 2), M.qinv(M.qm(4)), M.qneg(R.HALF), M.qdouble(M.qinv(M.qm(3))),
              (0, 1, 0, 0), (1, 0, 0, 1), (1 << 30, 0, 1, 0), (0x55555555, P - 1, 0, 0), (0, 0, 0, 1),
              (P - 1, P - 1, P - 1, P - 1)] + [M.random_felt(rng) for _ in range(50)]
    for y in others:
        p = R.corrected_poly(f0, f2, claim, y, a)
        assert M.qadd(M.horner(p, M.ZERO), M.horner(p, M.ONE)) == claim
    # every value the model inverts is a product of y, 1 - y, 1 - 2y, 1 - 3y up to constants: b = (1-y)/(1-2y), 1 - b = -y/(1-2y),
    # 2 - b = (1-3y)/(1-2y), so no other y can raise
    for y in others[:20]:
        d = M.qsub(M.ONE, M.qdouble(y))
        b = M.qdiv(M.qsub(M.ONE, y), d)
        assert M.qmul(M.qsub(M.ONE, b), d) == M.qneg(y)
        assert M.qmul(M.qsub(M.qm(2), b), d) == M.qsub(M.ONE, M.qmul(M.qm(3), y))


def test_round_model_trims_the_combined_polynomial():
    """n_coeffs is part of the transcript: an all-zero round hashes the digest alone, and a vanishing cubic term drops a felt."""
    rng = np.random.default_rng(6)
    y, a, alpha = M.random_felt(rng), M.random_felt(rng), M.random_felt(rng)
    ch = M.Channel()
    coeffs, _, claims, _ = R.round_finish_at(ch, [(M.ZERO, M.ZERO)], [M.ZERO], [M.ONE], [True], y, a, alpha)
    assert coeffs == [] and claims == [M.ZERO]
    ref = M.Channel()
    ref.mix_felts([])
    assert ch.digest == ref.digest
    f0, claim, corr = M.random_felt(rng), M.random_felt(rng), M.random_felt(rng)
    f2 = f2_for_quadratic(f0, claim, corr, y, a)
    coeffs, _, _, _ = R.round_finish_at(M.Channel(), [(f0, f2)], [claim], [corr], [True], y, a, alpha)
    assert len(coeffs) == 3


def f2_for_quadratic(f0, claim, corr, y, a):
    """The f2 for which the corrected polynomial has no cubic term.  Its leading coefficient is w0 + w1 + w2 with
    w0 = r0 / (-2b), w1 = -r1 / (1 - b), w2 = r2 / (2 (2 - b)) and r2 = f2 corr (3y - 1) a: solve w2 = -(w0 + w1) for f2."""
    b = M.qdiv(M.qsub(M.ONE, y), M.qsub(M.ONE, M.qdouble(y)))
    r0 = M.qmul(M.qmul(M.qmul(f0, corr), M.qsub(M.ONE, y)), a)
    r1 = M.qsub(claim, r0)
    w0 = M.qdiv(r0, M.qneg(M.qdouble(b)))
    w1 = M.qdiv(M.qneg(r1), M.qsub(M.ONE, b))
    r2 = M.qmul(M.qneg(M.qadd(w0, w1)), M.qdouble(M.qsub(M.qm(2), b)))
    eq2 = M.qsub(M.qmul(M.qm(3), y), M.ONE)
    return M.qdiv(r2, M.qmul(M.qmul(corr, eq2), a))

"""One round of prove_batch's batched sum-check, stated on gkr_model's tuples: what the prover does between the sums of a round
and the launches of the next (the corrected round polynomials, their combination, the channel's mix and draw, the new claims and
eq corrections).  tstwo_gkr_round_finish is checked against it word by word; chained over a layer it is gkr_model's
sumcheck_prove_batch (test_cpu_gkr_rounds.py), which is pinned by the reference's vectors.

It imports nothing from the package under test.  Scalars are QM31 4-tuples; `channel` is a gkr_model.Channel (updated)."""
from __future__ import annotations

import gkr_model as M

HALF = M.qinv(M.qm(2))
# the eq points at which correct_sum_as_poly_in_first_variable divides by zero: b = (1 - y) / (1 - 2y) is undefined (y = 1/2) or
# collides with the interpolation points 0, 1, 2 (y = 1, 0, 1/3)
DEGENERATE_Y = (M.ZERO, M.ONE, HALF, M.qinv(M.qm(3)))


def corrected_poly(f0, f2, claim, y_k, a):
    """correct_sum_as_poly_in_first_variable (gkr_prover.ts:609-660) from y_k = y[n - k] and a = 1 / eq({0}^(n-k+1), y[:n-k+1])."""
    b = M.qdiv(M.qsub(M.ONE, y_k), M.qsub(M.ONE, M.qdouble(y_k)))
    r0 = M.qmul(M.qmul(f0, M.eq([M.ZERO], [y_k])), a)
    r1 = M.qsub(claim, r0)
    r2 = M.qmul(M.qmul(f2, M.eq([M.qm(2)], [y_k])), a)
    return M.interpolate_lagrange([M.ZERO, M.ONE, M.qm(2), b], [r0, r1, r2, M.ZERO])


def combine(polys, alpha):
    """sumcheck.ts: reduceRight((acc, p) => acc * alpha + p), trimmed."""
    comb = []
    for p in reversed(polys):
        comb = [M.qmul(c, alpha) for c in comb]
        comb = [M.qadd(comb[i] if i < len(comb) else M.ZERO, p[i] if i < len(p) else M.ZERO) for i in range(max(len(comb), len(p)))]
    return M.trim(comb)


def round_finish_at(channel, sums, claims, corrections, active, y_k, a, alpha):
    """The round with its eq point given directly.  sums[i] = (f0, f2) (read for active instances only).  Returns
    (coeffs of the combined polynomial, trimmed; challenge; new claims; new corrections)."""
    polys = []
    for s, c, corr, act in zip(sums, claims, corrections, active):
        if act:
            polys.append(corrected_poly(M.qmul(s[0], corr), M.qmul(s[1], corr), c, y_k, a))
        else:
            polys.append(M.trim([M.qmul(c, HALF)]))
    coeffs = combine(polys, alpha)
    channel.mix_felts(coeffs)
    ch = channel.draw_felt()
    new_claims = [M.horner(p, ch) for p in polys]
    new_corr = [M.qmul(corr, M.eq([ch], [y_k])) if act else corr for corr, act in zip(corrections, active)]
    return coeffs, ch, new_claims, new_corr


def round_finish(channel, sums, claims, corrections, active, y, k, alpha):
    """The round of an oracle with k variables left, eq point y (all of the layer's)."""
    n = len(y)
    assert 0 < k <= n
    a = M.qinv(M.eq([M.ZERO] * (n - k + 1), list(y[:n - k + 1])))
    return round_finish_at(channel, sums, claims, corrections, active, y[n - k], a, alpha)


def inv_eq0_direct(y):
    """Entry r (the round with k = n - r variables left): 1 / eq({0}^(r+1), y[:r+1]), each by its own inversion."""
    return [M.qinv(M.eq([M.ZERO] * (r + 1), list(y[:r + 1]))) for r in range(len(y))]


def inv_eq0_table(y):
    """The same table from prefix products and one inversion (Montgomery's trick over the layer's rounds)."""
    pre, acc = [], M.ONE
    for yj in y:
        acc = M.qmul(acc, M.qsub(M.ONE, yj))
        pre.append(acc)
    prods, acc = [], M.ONE
    for e in pre:
        acc = M.qmul(acc, e)
        prods.append(acc)
    if not pre:
        return []
    inv = M.qinv(acc)
    out = [None] * len(pre)
    for r in range(len(pre) - 1, -1, -1):
        out[r] = M.qmul(inv, prods[r - 1]) if r else inv
        inv = M.qmul(inv, pre[r])
    return out


def layer_by_rounds(claims, oracles, alpha, channel):
    """gkr_model.sumcheck_prove_batch restated as a chain of round_finish calls: the sums come from the oracles' layers
    (gkr_model.sum_f0_f2), everything else from the round model.  Returns (round polys, assignment, final claims)."""
    n = max(o.n_vars() for o in oracles)
    claims = [M.qmul(c, M.qm(1 << (n - o.n_vars()))) for c, o in zip(claims, oracles)]
    corrections = [M.ONE] * len(oracles)
    layers = [o.layer for o in oracles]
    n_v = [o.n_vars() for o in oracles]
    y = oracles[0].y
    round_polys, assignment = [], []
    for rnd in range(n):
        rem = n - rnd
        active = [v >= rem and v > 0 for v in n_v]
        sums = [M.sum_f0_f2(lay, o.eq_evals, rem, o.lam) if act else None for lay, o, act in zip(layers, oracles, active)]
        coeffs, ch, claims, corrections = round_finish(channel, sums, claims, corrections, active, y, rem, alpha)
        for j, act in enumerate(active):
            if act:
                lay = layers[j]
                num = None if lay["num"] is None or lay["kind"] == M.SINGLES else M.fix_first_variable(lay["num"], ch)
                layers[j] = {"kind": M.GENERIC if lay["kind"] == M.MULT else lay["kind"], "num": num,
                             "den": M.fix_first_variable(lay["den"], ch)}
        round_polys.append(coeffs)
        assignment.append(ch)
    return round_polys, assignment, claims

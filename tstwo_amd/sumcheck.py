"""Batched sum-check (lookups/sumcheck.ts:99-227) and the univariate polynomials it exchanges (lookups/utils.ts).

Host-side protocol: O(rounds) QM31 scalars.  The per-round sums over 2^n values come from the oracle (gkr.py:
GkrMultivariatePolyOracle, whose sums run on the GPU)."""
from __future__ import annotations

from .fields import M31, P, QM31

MAX_DEGREE = 3


def _zero() -> QM31:
    return QM31.zero()


class UnivariatePoly:
    """Coefficients in the monomial basis, leading zeros trimmed (lookups/utils.ts UnivariatePoly)."""

    def __init__(self, coeffs):
        c = list(coeffs)
        while c and c[-1].tup() == (0, 0, 0, 0):
            c.pop()
        self.coeffs = c

    @staticmethod
    def from_(v: QM31) -> "UnivariatePoly":
        return UnivariatePoly([v])

    def eval_at_point(self, x: QM31) -> QM31:
        xt, acc = x.tup(), _Z
        for c in reversed(self.coeffs):
            acc = _qadd(_qmul(acc, xt), c.tup())
        return QM31.from_u32_unchecked(*acc)

    def degree(self) -> int:
        return max(0, len(self.coeffs) - 1)

    def mul_scalar(self, s: QM31) -> "UnivariatePoly":
        return UnivariatePoly([c.mul(s) for c in self.coeffs])

    def add(self, o: "UnivariatePoly") -> "UnivariatePoly":
        n = max(len(self.coeffs), len(o.coeffs))
        a = self.coeffs + [_zero()] * (n - len(self.coeffs))
        b = o.coeffs + [_zero()] * (n - len(o.coeffs))
        return UnivariatePoly([x.add(y) for x, y in zip(a, b)])

    @staticmethod
    def interpolate_lagrange(xs, ys) -> "UnivariatePoly":
        """The polynomial of degree < len(xs) through (xs[i], ys[i]) (lookups/utils.ts interpolateLagrange).  Runs on 4-tuples of
        ints: the result is exact, so it is the reference's whatever the order of operations."""
        if len(xs) != len(ys) or not xs:
            raise ValueError("xs and ys must have the same, nonzero length")
        xs, ys = [x.tup() for x in xs], [y.tup() for y in ys]
        coeffs = [_Z] * len(xs)
        for i, (xi, yi) in enumerate(zip(xs, ys)):
            den = _O
            for j, xj in enumerate(xs):
                if i != j:
                    den = _qmul(den, _qsub(xi, xj))
            term = [_qmul(yi, _qinv(den))]
            for j, xj in enumerate(xs):
                if i != j:                      # term *= (x - xj)
                    nxt = [_Z] * (len(term) + 1)
                    for k, a in enumerate(term):
                        nxt[k + 1] = _qadd(nxt[k + 1], a)
                        nxt[k] = _qsub(nxt[k], _qmul(a, xj))
                    term = nxt
            coeffs = [_qadd(a, b) for a, b in zip(coeffs, term)]
        return UnivariatePoly([QM31.from_u32_unchecked(*c) for c in coeffs])

    def __eq__(self, o):
        return isinstance(o, UnivariatePoly) and [c.tup() for c in self.coeffs] == [c.tup() for c in o.coeffs]

    def __repr__(self):
        return f"UnivariatePoly({[c.tup() for c in self.coeffs]})"


# QM31 on 4-tuples of ints (a + bi) + (c + di)u, u^2 = 2 + i: the same field as fields.QM31 without an object per M31
_Z, _O = (0, 0, 0, 0), (1, 0, 0, 0)


def _qadd(x, y): return ((x[0] + y[0]) % P, (x[1] + y[1]) % P, (x[2] + y[2]) % P, (x[3] + y[3]) % P)
def _qsub(x, y): return ((x[0] - y[0]) % P, (x[1] - y[1]) % P, (x[2] - y[2]) % P, (x[3] - y[3]) % P)


def _qmul(x, y):
    a, b, c, d = x
    e, f, g, h = y
    tr, ti = c * g - d * h, c * h + d * g               # x1 y1
    return ((a * e - b * f + 2 * tr - ti) % P, (a * f + b * e + tr + 2 * ti) % P,
            (a * g - b * h + c * e - d * f) % P, (a * h + b * g + c * f + d * e) % P)


def _qinv(x):
    if x == _Z:
        raise ZeroDivisionError("0 has no inverse")
    a, b, c, d = x
    b2r, b2i = (c * c - d * d) % P, (2 * c * d) % P
    dr, di = (a * a - b * b - 2 * b2r + b2i) % P, (2 * a * b - b2r - 2 * b2i) % P        # x0^2 - (2 + i) x1^2
    n = pow((dr * dr + di * di) % P, P - 2, P)
    ir, ii = dr * n % P, -di * n % P
    return ((a * ir - b * ii) % P, (a * ii + b * ir) % P, (-(c * ir - d * ii)) % P, (-(c * ii + d * ir)) % P)


def horner_eval(coeffs, x: QM31) -> QM31:
    acc = _zero()
    for c in reversed(coeffs):
        acc = acc.mul(x).add(c)
    return acc


def random_linear_combination(v, alpha: QM31) -> QM31:
    """v_0 + alpha v_1 + ... (lookups/utils.ts)."""
    return horner_eval(list(v), alpha)


def eq(x, y) -> QM31:
    """Lagrange kernel of the boolean hypercube (lookups/utils.ts eq); 1 for two empty vectors, as in Rust."""
    if len(x) != len(y):
        raise ValueError("x and y must have the same length")
    one = QM31.one()
    acc = one
    for a, b in zip(x, y):
        acc = acc.mul(a.mul(b).add(one.sub(a).mul(one.sub(b))))
    return acc


def fold_mle_evals(r: QM31, v0: QM31, v1: QM31) -> QM31:
    """foldMleEvals (lookups/utils.ts:256): v0 + r (v1 - v0)."""
    return r.mul(v1.sub(v0)).add(v0)


class SumcheckProof:
    def __init__(self, round_polys):
        self.round_polys = list(round_polys)


class SumcheckError(Exception):
    def __init__(self, message: str, round: int | None = None):
        super().__init__(message)
        self.round = round

    @staticmethod
    def degree_invalid(round: int) -> "SumcheckError":
        return SumcheckError(f"degree of the polynomial in round {round} is too high", round)

    @staticmethod
    def sum_invalid(claim, s, round: int) -> "SumcheckError":
        return SumcheckError(f"sum does not match the claim in round {round} (sum {s}, claim {claim})", round)


def prove_batch(claims, polys, lam: QM31, channel):
    """sumcheck.ts proveBatch: returns (proof, assignment, constant oracles, final claims).  Oracles with fewer variables join
    the last rounds: their claims are scaled by 2^unused and they contribute the constant claim / 2 until then."""
    if not polys:
        raise ValueError("No multivariate polynomials provided")
    if len(claims) != len(polys):
        raise ValueError("Mismatch between number of claims and polynomials")
    n = max(p.n_variables() for p in polys)
    claims = [c.mulM31(M31(1 << (n - p.n_variables()))) for c, p in zip(claims, polys)]
    polys = list(polys)
    half = M31(2).inverse()
    round_polys, assignment = [], []
    for rnd in range(n):
        rem = n - rnd
        this = polys_for_round(polys, claims, rem, half)
        for i, (rp, c) in enumerate(zip(this, claims)):
            if not rp.eval_at_point(QM31.zero()).add(rp.eval_at_point(QM31.one())).equals(c):
                raise AssertionError(f"Round polynomial check failed: i={i}, round={rnd}")
            if rp.degree() > MAX_DEGREE:
                raise AssertionError(f"Polynomial degree too high: i={i}, round={rnd}")
        rp = combine(this, lam)
        channel.mix_felts(rp.coeffs)
        ch = channel.draw_felt()
        claims = [p.eval_at_point(ch) for p in this]
        polys = [p.fix_first_variable(ch) if rem == p.n_variables() else p for p in polys]
        round_polys.append(rp)
        assignment.append(ch)
    return SumcheckProof(round_polys), assignment, polys, claims


def polys_for_round(polys, claims, rem, half):
    """Round polynomial of every oracle for a round with `rem` rounds left (a device-backed batch overrides the active ones)."""
    out = []
    for p, c in zip(polys, claims):
        out.append(p.sum_as_poly_in_first_variable(c) if rem == p.n_variables() else UnivariatePoly.from_(c.mulM31(half)))
    return out


def combine(polys, alpha: QM31) -> UnivariatePoly:
    """reduceRight((acc, p) => acc * alpha + p, 0)."""
    acc = UnivariatePoly([])
    for p in reversed(polys):
        acc = acc.mul_scalar(alpha).add(p)
    return acc


def partially_verify(claim: QM31, proof: SumcheckProof, channel):
    """sumcheck.ts partiallyVerify: returns (assignment, claimed evaluation at it)."""
    assignment = []
    for rnd, rp in enumerate(proof.round_polys):
        if rp.degree() > MAX_DEGREE:
            raise SumcheckError.degree_invalid(rnd)
        s = rp.eval_at_point(QM31.zero()).add(rp.eval_at_point(QM31.one()))
        if not claim.equals(s):
            raise SumcheckError.sum_invalid(claim, s, rnd)
        channel.mix_felts(rp.coeffs)
        ch = channel.draw_felt()
        claim = rp.eval_at_point(ch)
        assignment.append(ch)
    return assignment, claim

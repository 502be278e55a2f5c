"""Pure-Python integer model of the reference's LogUp-GKR ops and protocol (packages/core/src of the reference:
backend/cpu/lookups/{gkr,mle}.ts, lookups/{gkr_prover,sumcheck,gkr_verifier,utils}.ts), with the Rust stwo behaviour where the
TypeScript text is a placeholder (EqEvals.generate; eq() of two empty vectors = 1).

It imports nothing from the package under test or the oracle: QM31 arithmetic and the Blake2s channel are written out here, and
the QM31 arithmetic is pinned by tests/golden/qm31-test-vectors.json (test_cpu_gkr.py).

Scalars are QM31 4-tuples of ints.  MLE columns are numpy uint64 arrays: a secure column has shape (4, n) (the 4 SoA
coordinates), a base column shape (n,); the first variable is the most significant bit of the index.  Layers are dicts
{"kind": GP | GENERIC | MULT | SINGLES, "num": column or None, "den": column} (grand product: "den" holds the product column).
"""
from __future__ import annotations

import hashlib

import numpy as np

P = 2147483647
GP, GENERIC, MULT, SINGLES = 0, 1, 2, 3
ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)


# ---------------------------------------------------------------- scalar QM31 (fields/qm31.ts)
def qadd(x, y): return tuple((a + b) % P for a, b in zip(x, y))
def qsub(x, y): return tuple((a - b) % P for a, b in zip(x, y))
def qneg(x): return tuple((-a) % P for a in x)
def qdouble(x): return qadd(x, x)
def qm(v): return (int(v) % P, 0, 0, 0)


def _cmul(ar, ai, br, bi):
    return (ar * br - ai * bi) % P, (ar * bi + ai * br) % P


def qmul(x, y):
    a0r, a0i, a1r, a1i = x
    b0r, b0i, b1r, b1i = y
    c0r, c0i = _cmul(a0r, a0i, b0r, b0i)
    tr, ti = _cmul(a1r, a1i, b1r, b1i)
    rr, ri = (2 * tr - ti) % P, (tr + 2 * ti) % P          # (2 + i) * t
    d0r, d0i = _cmul(a0r, a0i, b1r, b1i)
    d1r, d1i = _cmul(a1r, a1i, b0r, b0i)
    return ((c0r + rr) % P, (c0i + ri) % P, (d0r + d1r) % P, (d0i + d1i) % P)


def qinv(x):
    if x == ZERO:
        raise ZeroDivisionError("0 has no inverse")
    # x^(P^4 - 2) is slow in Python; use the norm tower instead (qm31.ts:282-305)
    a0r, a0i, a1r, a1i = x
    b2r, b2i = _cmul(a1r, a1i, a1r, a1i)
    a2r, a2i = _cmul(a0r, a0i, a0r, a0i)
    # denom = a0^2 - (2 + i) b^2
    rr, ri = (2 * b2r - b2i) % P, (b2r + 2 * b2i) % P
    dr, di = (a2r - rr) % P, (a2i - ri) % P
    n = pow((dr * dr + di * di) % P, P - 2, P)
    ir, ii = dr * n % P, (-di) * n % P
    c0 = _cmul(a0r, a0i, ir, ii)
    c1 = _cmul(a1r, a1i, ir, ii)
    return (c0[0], c0[1], (-c1[0]) % P, (-c1[1]) % P)


def qdiv(x, y): return qmul(x, qinv(y))


def eq(x, y):
    """lookups/utils.ts eq(); the product over zero coordinates is 1 (Rust)."""
    assert len(x) == len(y)
    acc = ONE
    for a, b in zip(x, y):
        acc = qmul(acc, qadd(qmul(a, b), qmul(qsub(ONE, a), qsub(ONE, b))))
    return acc


def horner(coeffs, x):
    acc = ZERO
    for c in reversed(coeffs):
        acc = qadd(qmul(acc, x), c)
    return acc


random_linear_combination = horner


def fold_mle_evals(r, v0, v1): return qadd(qmul(r, qsub(v1, v0)), v0)


# ---------------------------------------------------------------- numpy QM31 columns, shape (4, n)
def vadd(x, y): return (x + y) % P
def vsub(x, y): return (x + (P - y)) % P


def _vcmul(ar, ai, br, bi):
    return (ar * br + (P - ai) * bi) % P, (ar * bi + ai * br) % P


def vmul(x, y):
    """Element-wise QM31 product of (4, n) arrays; y may be a scalar 4-tuple."""
    y = [np.uint64(v) for v in y] if isinstance(y, tuple) else y
    c0r, c0i = _vcmul(x[0], x[1], y[0], y[1])
    tr, ti = _vcmul(x[2], x[3], y[2], y[3])
    rr, ri = (2 * tr + (P - ti)) % P, (tr + 2 * ti) % P
    d0r, d0i = _vcmul(x[0], x[1], y[2], y[3])
    d1r, d1i = _vcmul(x[2], x[3], y[0], y[1])
    return np.stack([(c0r + rr) % P, (c0i + ri) % P, (d0r + d1r) % P, (d0i + d1i) % P])


def vmul_base(x, m):
    """(4, n) QM31 times (n,) M31."""
    return (x * m[None, :]) % P


def lift(m):
    """(n,) M31 -> (4, n) QM31."""
    out = np.zeros((4, m.shape[0]), dtype=np.uint64)
    out[0] = m
    return out


def vsum(x): return tuple(int(v) for v in (x.sum(axis=1, dtype=np.uint64) % P))
def at(x, i): return tuple(int(v) for v in x[:, i]) if x.ndim == 2 else qm(x[i])


def random_secure(rng, n): return rng.integers(0, P, size=(4, n), dtype=np.uint64)
def random_base(rng, n): return rng.integers(0, P, size=n, dtype=np.uint64)
def random_felt(rng): return tuple(int(v) for v in rng.integers(0, P, size=4))


# ---------------------------------------------------------------- GkrOps / MleOps (backend/cpu/lookups)
def gen_eq_evals_loop(y, v):
    """gkr.ts:90-104, element by element (the reference's doubling loop)."""
    evals = [v]
    for yi in reversed(y):
        n = len(evals)
        for j in range(n):
            tmp = qmul(evals[j], yi)
            evals.append(tmp)
            evals[j] = qsub(evals[j], tmp)
    return np.array(evals, dtype=np.uint64).T.reshape(4, -1)


def gen_eq_evals(y, v):
    """The same table, one numpy doubling per variable: the new most significant bit comes from y[0] last."""
    evals = np.array(v, dtype=np.uint64).reshape(4, 1)
    for yi in reversed(y):
        tmp = vmul(evals, yi)
        evals = np.concatenate([vsub(evals, tmp), tmp], axis=1)
    return evals


def eq_evals_generate(y):
    """EqEvals.generate (Rust): [1] for empty y, else gen_eq_evals(y[1:], eq([0], [y[0]]))."""
    if not y:
        return np.array(ONE, dtype=np.uint64).reshape(4, 1)
    return gen_eq_evals(list(y[1:]), qsub(ONE, y[0]))


def n_vars_of(layer): return int(layer["den"].shape[-1]).bit_length() - 1


def next_layer(layer):
    """gkr.ts:109-137, 317-358; None for an output layer."""
    if n_vars_of(layer) == 0:
        return None
    d = layer["den"]
    d0, d1 = d[:, 0::2], d[:, 1::2]
    if layer["kind"] == GP:
        return {"kind": GP, "num": None, "den": vmul(d0, d1)}
    if layer["kind"] == GENERIC:
        n0, n1 = layer["num"][:, 0::2], layer["num"][:, 1::2]
        num = vadd(vmul(n0, d1), vmul(n1, d0))
    elif layer["kind"] == MULT:
        num = vadd(vmul_base(d1, layer["num"][0::2]), vmul_base(d0, layer["num"][1::2]))
    else:
        num = vadd(d0, d1)
    return {"kind": GENERIC, "num": num, "den": vmul(d0, d1)}


def fix_first_variable(col, r):
    """mle.ts:68-130: base (n,) or secure (4, n) -> secure (4, n/2)."""
    if col.ndim == 1:
        col = lift(col)
    h = col.shape[1] // 2
    lhs, rhs = col[:, :h], col[:, h:]
    return vadd(vmul(vsub(rhs, lhs), r), lhs)


def _gate_vec(kind, n0, d0, n1, d1, lam):
    if kind == GP:
        return vmul(d0, d1)
    dd = vmul(d0, d1)
    nn = vadd(d0, d1) if kind == SINGLES else vadd(vmul(n0, d1), vmul(n1, d0))
    return vadd(nn, vmul(dd, lam))


def sum_f0_f2(layer, eq_evals, n_vars, lam):
    """evalGrandProductSum / evalLogupSum / evalLogupSinglesSum (gkr.ts:185-311) over n_terms = 2^(n_vars-1) terms."""
    if n_vars == 0:
        raise ValueError("Number of variables must not be zero")
    nt = 1 << (n_vars - 1)
    d = layer["den"]
    num = layer["num"]
    if layer["kind"] == MULT:
        num = lift(num)
    idx0 = 2 * np.arange(nt)
    idx1 = 2 * (nt + np.arange(nt))

    def pick(c, idx):
        return None if c is None else c[:, idx]
    d00, d01, d10, d11 = pick(d, idx0), pick(d, idx0 + 1), pick(d, idx1), pick(d, idx1 + 1)
    n00, n01, n10, n11 = pick(num, idx0), pick(num, idx0 + 1), pick(num, idx1), pick(num, idx1 + 1)

    def at2(x0, x1): return None if x0 is None else vsub(vadd(x1, x1), x0)
    e = eq_evals[:, :nt]
    f0 = vsum(vmul(_gate_vec(layer["kind"], n00, d00, n01, d01, lam), e))
    f2 = vsum(vmul(_gate_vec(layer["kind"], at2(n00, n10), at2(d00, d10), at2(n01, n11), at2(d01, d11), lam), e))
    return f0, f2


# ---------------------------------------------------------------- univariate polynomials (lookups/utils.ts)
def trim(coeffs):
    coeffs = list(coeffs)
    while coeffs and coeffs[-1] == ZERO:
        coeffs.pop()
    return coeffs


def poly_mul_linear(p, c):
    """p(x) * (x - c)."""
    out = [ZERO] * (len(p) + 1)
    for i, a in enumerate(p):
        out[i + 1] = qadd(out[i + 1], a)
        out[i] = qsub(out[i], qmul(a, c))
    return out


def interpolate_lagrange(xs, ys):
    coeffs = [ZERO] * len(xs)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        prod = yi
        for j, xj in enumerate(xs):
            if i != j:
                prod = qmul(prod, qinv(qsub(xi, xj)))
        term = [prod]
        for j, xj in enumerate(xs):
            if i != j:
                term = poly_mul_linear(term, xj)
        coeffs = [qadd(a, b) for a, b in zip(coeffs, term)]
    return trim(coeffs)


def correct_sum_as_poly_in_first_variable(f0, f2, claim, y, k):
    """gkr_prover.ts:609-660."""
    n = len(y)
    assert 0 < k <= n
    a = qinv(eq([ZERO] * (n - k + 1), list(y[:n - k + 1])))
    yk = y[n - k]
    b = qdiv(qsub(ONE, yk), qsub(ONE, qdouble(yk)))
    r0 = qmul(qmul(f0, eq([ZERO], [yk])), a)
    r1 = qsub(claim, r0)
    r2 = qmul(qmul(f2, eq([qm(2)], [yk])), a)
    return interpolate_lagrange([ZERO, ONE, qm(2), b], [r0, r1, r2, ZERO])


# ---------------------------------------------------------------- Blake2s channel (Rust draw semantics)
class Channel:
    def __init__(self):
        self.digest, self.n_sent = bytes(32), 0

    def mix_felts(self, felts):
        h = hashlib.blake2s(self.digest)
        for f in felts:
            for v in f:
                h.update(int(v).to_bytes(4, "little"))
        self.digest, self.n_sent = h.digest(), 0

    def draw_felt(self):
        while True:
            b = hashlib.blake2s(self.digest + self.n_sent.to_bytes(4, "little") + bytes(28)).digest()
            self.n_sent += 1
            u = [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(8)]
            if all(x < 2 * P for x in u):
                return tuple(x % P for x in u[:4])


# ---------------------------------------------------------------- GKR prover (gkr_prover.ts:440-580, sumcheck.ts:99-227)
def output_values(layer):
    d0 = at(layer["den"], 0)
    if layer["kind"] == GP:
        return [d0]
    if layer["kind"] == SINGLES:
        return [ONE, d0]
    return [at(layer["num"], 0), d0]


class Oracle:
    """GkrMultivariatePolyOracle (gkr_prover.ts:290-420) over a model layer."""

    def __init__(self, eq_evals, y, layer, correction, lam):
        self.eq_evals, self.y, self.layer, self.correction, self.lam = eq_evals, y, layer, correction, lam

    def n_vars(self): return n_vars_of(self.layer) - 1

    def sum_as_poly(self, claim):
        k = self.n_vars()
        f0, f2 = sum_f0_f2(self.layer, self.eq_evals, k, self.lam)
        return correct_sum_as_poly_in_first_variable(qmul(f0, self.correction), qmul(f2, self.correction), claim, self.y, k)

    def fix_first_variable(self, c):
        k = self.n_vars()
        if k == 0:
            return self
        z0 = self.y[len(self.y) - k]
        lay = self.layer
        kind = GENERIC if lay["kind"] == MULT else lay["kind"]
        num = None if lay["num"] is None or lay["kind"] == SINGLES else fix_first_variable(lay["num"], c)
        new = {"kind": kind, "num": num, "den": fix_first_variable(lay["den"], c)}
        return Oracle(self.eq_evals, self.y, new, qmul(self.correction, eq([c], [z0])), self.lam)

    def mask(self):
        lay = self.layer
        assert n_vars_of(lay) == 1
        d = (at(lay["den"], 0), at(lay["den"], 1))
        if lay["kind"] == GP:
            return [d]
        if lay["kind"] == SINGLES:
            return [(ONE, ONE), d]
        if lay["kind"] == MULT:
            raise NotImplementedError("LogUpMultiplicities should never reach tryIntoMask")
        return [(at(lay["num"], 0), at(lay["num"], 1)), d]


def sumcheck_prove_batch(claims, oracles, alpha, channel):
    n = max(o.n_vars() for o in oracles)
    claims = [qmul(c, qm(1 << (n - o.n_vars()))) for c, o in zip(claims, oracles)]
    round_polys, assignment = [], []
    half = qinv(qm(2))
    for rnd in range(n):
        rem = n - rnd
        polys = []
        for c, o in zip(claims, oracles):
            p = o.sum_as_poly(c) if rem == o.n_vars() else trim([qmul(c, half)])
            assert qadd(horner(p, ZERO), horner(p, ONE)) == c, "round polynomial does not sum to the claim"
            assert len(p) <= 4
            polys.append(p)
        comb = []
        for p in reversed(polys):                      # reduceRight(acc * alpha + poly)
            comb = [qmul(a, alpha) for a in comb]
            comb = [qadd(comb[i] if i < len(comb) else ZERO, p[i] if i < len(p) else ZERO) for i in range(max(len(comb), len(p)))]
            comb = trim(comb)
        channel.mix_felts(comb)
        ch = channel.draw_felt()
        claims = [horner(p, ch) for p in polys]
        oracles = [o.fix_first_variable(ch) if rem == o.n_vars() else o for o in oracles]
        round_polys.append(comb)
        assignment.append(ch)
    return round_polys, assignment, oracles, claims


def gen_layers(layer):
    out = [layer]
    while (nxt := next_layer(out[-1])) is not None:
        out.append(nxt)
    return out


def prove_batch(channel, input_layers):
    """Returns (proof, artifact): proof = {"sumcheck_proofs": [[poly coeffs] per round] per layer, "masks": [[mask] per layer]
    per instance, "output_claims": [...] per instance}; artifact = {"ood_point", "claims_to_verify", "n_variables"}."""
    n_inst = len(input_layers)
    n_layers_by = [n_vars_of(l) for l in input_layers]
    n_layers = max(n_layers_by)
    stacks = [list(reversed(gen_layers(l))) for l in input_layers]
    output_claims = [None] * n_inst
    masks = [[] for _ in range(n_inst)]
    sumcheck_proofs = []
    ood = []
    claims_to_verify = [None] * n_inst
    for layer in range(n_layers):
        rem = n_layers - layer
        for i in range(n_inst):
            if n_layers_by[i] == rem:
                vals = output_values(stacks[i].pop(0))
                claims_to_verify[i] = list(vals)
                output_claims[i] = vals
        for c in claims_to_verify:
            if c is not None:
                channel.mix_felts(c)
        eqe = eq_evals_generate(ood)
        alpha = channel.draw_felt()
        lam = channel.draw_felt()
        oracles, sclaims, insts = [], [], []
        for i, c in enumerate(claims_to_verify):
            if c is not None:
                oracles.append(Oracle(eqe, list(ood), stacks[i].pop(0), ONE, lam))
                sclaims.append(random_linear_combination(c, lam))
                insts.append(i)
        polys, s_ood, consts, _ = sumcheck_prove_batch(sclaims, oracles, alpha, channel)
        sumcheck_proofs.append(polys)
        ms = [o.mask() for o in consts]
        for i, m in zip(insts, ms):
            channel.mix_felts([v for col in m for v in col])
            masks[i].append(m)
        ch = channel.draw_felt()
        ood = list(s_ood) + [ch]
        for i, m in zip(insts, ms):
            claims_to_verify[i] = [fold_mle_evals(ch, a, b) for a, b in m]
    proof = {"sumcheck_proofs": sumcheck_proofs, "masks": masks, "output_claims": output_claims}
    artifact = {"ood_point": ood, "claims_to_verify": claims_to_verify, "n_variables": n_layers_by}
    return proof, artifact


# ---------------------------------------------------------------- independent checks
def eval_mle_at(col, point):
    """sum_x eq(x, point) col[x] (first variable = most significant bit), for the artifact's claims."""
    e = gen_eq_evals(list(point), ONE)
    c = lift(col) if col.ndim == 1 else col
    return vsum(vmul(c, e))


def direct_output(layer):
    """The circuit output computed directly: product of all values, or the fraction sum (numerator, denominator)."""
    d = layer["den"]
    if layer["kind"] == GP:
        acc = ONE
        for i in range(d.shape[1]):
            acc = qmul(acc, at(d, i))
        return [acc]
    num, den = ZERO, ONE
    for i in range(d.shape[1]):
        n_i = ONE if layer["kind"] == SINGLES else at(layer["num"], i)
        d_i = at(d, i)
        num, den = qadd(qmul(num, d_i), qmul(n_i, den)), qmul(den, d_i)
    return [num, den]

"""Integer model of AIR constraint evaluation and the composition polynomial (Rust stwo air/accumulation.rs, air/components.rs,
constraint_framework/component.rs, examples/wide_fibonacci; the reference's air/ and constraint_framework/ shapes), for the
wide-Fibonacci and mul-add (the Rust tutorial's example 05) AIRs.

It imports nothing from the package under test.  QM31 scalars come from tests/gkr_model.py (pinned there by the reference's
vectors); the polynomial steps (interpolate, evaluate, evaluate at a point) use the CPU oracle, as the other parity tests do.
Circle points and the vanishing polynomial are written out here from the definitions.

Columns are numpy uint64 arrays of M31 values; a secure column has shape (4, n).  Scalars are QM31 4-tuples of ints.
"""
from __future__ import annotations

import numpy as np

from gkr_model import P, qadd, qinv, qm, qmul, qsub
from oracle import oracle as orc

GEN = (2, 1268011823)                  # generator of the circle group of order 2^31
ONE_Q = (1, 0, 0, 0)


# ---------------------------------------------------------------- circle points over M31 (ints) or QM31 (tuples)
def _m_ops(secure):
    if secure:
        return qadd, qsub, qmul, lambda v: qsub((0, 0, 0, 0), v)
    return (lambda a, b: (a + b) % P, lambda a, b: (a - b) % P, lambda a, b: a * b % P, lambda a: (-a) % P)


def padd(p, q, secure=False):
    add, sub, mul, _ = _m_ops(secure)
    return (sub(mul(p[0], q[0]), mul(p[1], q[1])), add(mul(p[0], q[1]), mul(p[1], q[0])))


def pneg(p, secure=False):
    return (p[0], _m_ops(secure)[3](p[1]))


def index_to_point(idx):
    """idx * GEN (idx mod 2^31)."""
    idx %= 1 << 31
    res, cur = (1, 0), GEN
    while idx:
        if idx & 1:
            res = padd(res, cur)
        cur = padd(cur, cur)
        idx >>= 1
    return res


def lift(p):
    return (qm(p[0]), qm(p[1]))


# CanonicCoset(log): the coset of odds, initial index 2^(30 - log), step 2^(31 - log)
def canonic_coset(log):
    return (1 << (30 - log), log)          # (initial index, log size)


def eval_domain_index(log, i):
    """CanonicCoset(log).circle_domain().at(i) as an index: the half coset of odds of size 2^(log-1), then its negation."""
    h = 1 << (log - 1)
    init, step = 1 << (31 - log - 1), 1 << (31 - log + 1)
    if i < h:
        return (init + i * step) % (1 << 31)
    return (-(init + (i - h) * step)) % (1 << 31)


def domain_point(log, i):
    return index_to_point(eval_domain_index(log, i))


def half_initial(log):
    return (1 << (31 - log - 1)) % (1 << 31)     # initial index of CanonicCoset(log).circle_domain().half_coset


def coset_vanishing(coset, p, secure=False):
    """coset_vanishing(coset, p): shift p so that the coset maps onto the x = 0 points of the subgroup of its size, then double
    the x coordinate log_size - 1 times (2x^2 - 1)."""
    init_idx, log = coset
    init = index_to_point(init_idx)
    half = index_to_point(1 << (31 - log - 1))          # step / 2
    if secure:
        init, half = lift(init), lift(half)
    x = padd(padd(p, pneg(init, secure), secure), half, secure)[0]
    for _ in range(1, log):
        if secure:
            x = qsub(qadd(qmul(x, x), qmul(x, x)), ONE_Q)
        else:
            x = (2 * x * x - 1) % P
    return x


def bit_reverse_index(i, log):
    return int(format(i, f"0{log}b")[::-1], 2) if log else 0


def bit_reverse_perm(log):
    idx = np.arange(1 << log)
    r = np.zeros_like(idx)
    for k in range(log):
        r |= ((idx >> k) & 1) << (log - 1 - k)
    return r


def denom_inv(trace_log, eval_log):
    """The bit-reversed 1 / coset_vanishing(trace coset, eval_domain.at(j)), j < 2^(eval_log - trace_log)."""
    e = eval_log - trace_log
    vals = [pow(coset_vanishing(canonic_coset(trace_log), domain_point(eval_log, j)), P - 2, P) for j in range(1 << e)]
    return [vals[bit_reverse_index(j, e)] for j in range(1 << e)]


# ---------------------------------------------------------------- traces and constraints
def wide_fib_trace(a, b, n_cols):
    cols = [np.asarray(a, dtype=np.uint64) % P, np.asarray(b, dtype=np.uint64) % P]
    for _ in range(2, n_cols):
        cols.append((cols[-2] * cols[-2] % P + cols[-1] * cols[-1] % P) % P)
    return cols


def mul_add_trace(x0, x1):
    x0, x1 = np.asarray(x0, dtype=np.uint64) % P, np.asarray(x1, dtype=np.uint64) % P
    return [x0, x1, (x0 * x1 % P + x0) % P]


def example05_trace(log_n=4):
    """The table of the Rust tutorial's example 05: rows 0 and 1 set, the rest zero."""
    n = 1 << log_n
    c1, c2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    c1[0], c1[1], c2[0], c2[1] = 1, 7, 5, 11
    return mul_add_trace(c1, c2)


WIDE_FIB, MUL_ADD = "wide_fib", "mul_add"


def constraints_cols(kind, cols):
    """Row-wise constraint columns (M31) of one component."""
    if kind == MUL_ADD:
        return [(cols[0] * cols[1] % P + cols[0] + 2 * P - cols[2]) % P]
    sq = [c * c % P for c in cols]
    return [(cols[i + 2] + 2 * P - sq[i] - sq[i + 1]) % P for i in range(len(cols) - 2)]


def constraints_point(kind, vals):
    """The same constraints on QM31 values (the OODS evaluations of the columns)."""
    if kind == MUL_ADD:
        return [qsub(qadd(qmul(vals[0], vals[1]), vals[0]), vals[2])]
    return [qsub(vals[i + 2], qadd(qmul(vals[i], vals[i]), qmul(vals[i + 1], vals[i + 1]))) for i in range(len(vals) - 2)]


def n_constraints(kind, n_cols):
    return 1 if kind == MUL_ADD else n_cols - 2


# ---------------------------------------------------------------- QM31 powers and accumulation
def qpow(x, e):
    r = ONE_Q
    while e:
        if e & 1:
            r = qmul(r, x)
        x = qmul(x, x)
        e >>= 1
    return r


def component_coeffs(alpha, counts):
    """Coefficients of every component's constraints: over the constraints of all components in order (global index g), constraint
    g gets alpha^(total - 1 - g)."""
    total = sum(counts)
    out, g = [], 0
    for n in counts:
        out.append([qpow(alpha, total - 1 - (g + i)) for i in range(n)])
        g += n
    return out


def point_horner(alpha, evals):
    acc = (0, 0, 0, 0)
    for e in evals:
        acc = qadd(qmul(acc, alpha), e)
    return acc


def row_combination(coeffs, cons):
    """sum_i coeffs[i] * cons[i] as a (4, n) secure column."""
    n = cons[0].shape[0]
    out = np.zeros((4, n), dtype=np.uint64)
    for c, col in zip(coeffs, cons):
        for j in range(4):
            out[j] = (out[j] + c[j] * col % P) % P
    return out


def quotients_on_domain(kind, eval_cols, trace_log, log_expand, coeffs, dinv, accum=None):
    """accum[r] + row_res(r) * dinv[r >> trace_log] (the device kernel's contract)."""
    n = 1 << (trace_log + log_expand)
    rr = row_combination(coeffs, constraints_cols(kind, eval_cols))
    d = np.asarray(dinv, dtype=np.uint64)[np.arange(n) >> trace_log]
    out = np.zeros((4, n), dtype=np.uint64) if accum is None else np.asarray(accum, dtype=np.uint64).copy()
    for j in range(4):
        out[j] = (out[j] + rr[j] * d % P) % P
    return out


# ---------------------------------------------------------------- polynomials (CPU oracle)
def _tw(log):
    return orc.precompute_twiddles(half_initial(log), log - 1)


def interpolate(vals, log):
    _, itw = _tw(log)
    return orc.cfft_interpolate(np.asarray(vals, dtype=np.uint32), log, half_initial(log), itw, log - 1).astype(np.uint64)


def evaluate(coeffs, log_from, log_to):
    """A polynomial of 2^log_from coefficients on CanonicCoset(log_to).circle_domain() (bit-reversed order)."""
    c = np.zeros(1 << log_to, dtype=np.uint32)
    c[:1 << log_from] = np.asarray(coeffs, dtype=np.uint32)
    tw, _ = _tw(log_to)
    return orc.cfft_evaluate(c, log_to, half_initial(log_to), tw, log_to - 1).astype(np.uint64)


def extend(vals, log, log_to):
    return evaluate(interpolate(vals, log), log, log_to)


def eval_at(coeffs, log, point):
    return tuple(orc.eval_at_point(np.asarray(coeffs, dtype=np.uint32), log, point[0], point[1]))


def from_partial_evals(e):
    basis = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    acc = (0, 0, 0, 0)
    for v, b in zip(e, basis):
        acc = qadd(acc, qmul(v, b))
    return acc


def random_point(t):
    """((1 - t^2) / (1 + t^2), 2t / (1 + t^2)): a QM31 point on the circle."""
    t2 = qmul(t, t)
    inv = qinv(qadd(t2, ONE_Q))
    return (qmul(qsub(ONE_Q, t2), inv), qmul(qadd(t, t), inv))


# ---------------------------------------------------------------- composition polynomial
def composition_polynomial(components, alpha):
    """components: [(kind, trace_log, columns on the trace domain)].  Returns (log size, 4 coefficient arrays): the sub-accumulations
    per evaluation-domain size (log + 1), combined in ascending order (evaluate the previous polynomial, add, interpolate)."""
    coeffs = component_coeffs(alpha, [n_constraints(k, len(cols)) for k, _, cols in components])
    subs = {}
    for (kind, log, cols), cf in zip(components, coeffs):
        el = log + 1
        eval_cols = [extend(c, log, el) for c in cols]
        subs[el] = quotients_on_domain(kind, eval_cols, log, 1, cf, denom_inv(log, el), subs.get(el))
    cur, cur_log = None, None
    for el in sorted(subs):
        vals = subs[el].copy()
        if cur is not None:
            for j in range(4):
                vals[j] = (vals[j] + evaluate(cur[j], cur_log, el)) % P
        cur, cur_log = [interpolate(vals[j], el) for j in range(4)], el
    return cur_log, cur


def eval_composition_at_point(components, alpha, point):
    """The verifier's side: sum over constraints of alpha^(total-1-g) c_g(trace values at point) / vanishing(trace coset, point)."""
    evals = []
    for kind, log, cols in components:
        vals = [eval_at(interpolate(c, log), log, point) for c in cols]
        dinv = qinv(coset_vanishing(canonic_coset(log), point, secure=True))
        evals += [qmul(c, dinv) for c in constraints_point(kind, vals)]
    return point_horner(alpha, evals)

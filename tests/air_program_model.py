"""Integer model of user-defined constraints evaluated at row offsets (Rust stwo constraint_framework: masks at offsets,
offset_bit_reversed_circle_domain_index; the reference's utils.ts and mask.ts), for the program interpreter of
tstwo_air_eval_program and the FibonacciRows AIR.

It imports nothing from the package under test.  Row neighbours are found geometrically: the point of a row, plus `offset`
trace steps, looked up among the evaluation domain's points.  Circle points, QM31 scalars and the polynomial steps come from
tests/air_model.py (and through it tests/gkr_model.py and the CPU oracle).
"""
from __future__ import annotations

import numpy as np

import air_model as M
from gkr_model import P, qadd, qinv, qm, qmul, qsub

# include/tstwo_hip.h TSTWO_AIR_OP_*
LOAD, CONST, ADD, SUB, MUL, SQR, NEG, ACC = range(8)
MASK31 = (1 << 31) - 1


# ---------------------------------------------------------------- neighbours, from the geometry
def neighbour_map(trace_log, eval_log, offset):
    """nb[r] = the row (bit-reversed position on CanonicCoset(eval_log).circle_domain()) whose point is the point of row r plus
    `offset` steps of CanonicCoset(trace_log)."""
    n, h = 1 << eval_log, 1 << (eval_log - 1)
    i = M.bit_reverse_perm(eval_log).astype(np.int64)           # circle-domain index of each row
    init, step2 = 1 << (31 - eval_log - 1), 1 << (31 - eval_log + 1)
    idx = np.where(i < h, init + i * step2, -(init + (i - h) * step2)) & MASK31        # the point of each row, as an index
    target = (idx + offset * (1 << (31 - trace_log))) & MASK31
    order = np.argsort(idx)
    nb = order[np.searchsorted(idx[order], target)]
    assert np.array_equal(idx[nb], target) and n == len(nb)
    return nb


# ---------------------------------------------------------------- the program interpreter
def encode(op, dst=0, x=0, w1=0):
    return [op | (dst << 8) | (x << 16), w1 & 0xffffffff]


def run_program(words, cols, trace_log, log_expand):
    """The constraint values e_k (one numpy column each, in ACC order) of a program over `cols` on the evaluation domain."""
    eval_log = trace_log + log_expand
    regs, out, nbs = {}, [], {}
    for pc in range(len(words) // 2):
        w0, w1 = words[2 * pc], words[2 * pc + 1]
        op, dst, x = w0 & 0xff, (w0 >> 8) & 0xff, w0 >> 16
        if op == LOAD:
            off = w1 - (1 << 32) if w1 >= 1 << 31 else w1
            if off == 0:
                v = cols[x] % P
            else:
                if off not in nbs:
                    nbs[off] = neighbour_map(trace_log, eval_log, off)
                v = cols[x][nbs[off]] % P
        elif op == CONST:
            v = np.full(1 << eval_log, w1, dtype=np.uint64)
        elif op == ACC:
            out.append(regs[x])
            continue
        elif op == SQR:
            v = regs[x] * regs[x] % P
        elif op == NEG:
            v = (P - regs[x]) % P
        else:
            a, b = regs[x], regs[w1]
            v = {ADD: (a + b) % P, SUB: (a + P - b) % P, MUL: a * b % P}[op]
        regs[dst] = np.asarray(v, dtype=np.uint64)
    return out


def eval_program_on_domain(words, cols, trace_log, log_expand, coeffs, dinv, accum=None):
    """accum[r] + (sum_k coeffs[k] e_k(r)) * dinv[r >> trace_log] (the kernel's contract)."""
    cons = run_program(words, cols, trace_log, log_expand)
    n = 1 << (trace_log + log_expand)
    rr = M.row_combination(coeffs, cons)
    d = np.asarray(dinv, dtype=np.uint64)[np.arange(n) >> trace_log]
    out = np.zeros((4, n), dtype=np.uint64) if accum is None else np.asarray(accum, dtype=np.uint64).copy()
    for j in range(4):
        out[j] = (out[j] + rr[j] * d % P) % P
    return out


def random_program(rng, n_cols, n_constraints, n_ops, max_regs=32, max_offset=3):
    """A random DAG of loads at offsets, constants, add, sub, mul, square and neg, with n_constraints ACCs, as raw words.  Every
    register read was written before; registers are < max_regs."""
    words, live = [], []                    # live: registers holding a value

    def dst():
        if len(live) < max_regs:
            r = len(live)
        else:
            r = int(rng.integers(0, max_regs))
        return r

    for _ in range(n_ops):
        kind = rng.integers(0, 10) if live else 0
        d = dst()
        if kind <= 2:
            words += encode(LOAD, d, int(rng.integers(0, n_cols)), int(rng.integers(-max_offset, max_offset + 1)))
        elif kind == 3:
            words += encode(CONST, d, 0, int(rng.integers(0, P)))
        elif kind in (4, 5, 6):
            op = (ADD, SUB, MUL)[kind - 4]
            words += encode(op, d, int(rng.choice(live)), int(rng.choice(live)))
        else:
            words += encode(SQR if kind < 9 else NEG, d, int(rng.choice(live)))
        if d not in live:
            live.append(d)
    for _ in range(n_constraints):
        words += encode(ACC, 0, int(rng.choice(live)))
    return words


# ---------------------------------------------------------------- FibonacciRows: the AIR and its DEEP-ALI identity
def coset_positions(log):
    """Storage position of coset-order row k: bit_reverse(circle-domain index of coset index k), from the geometry."""
    init = 1 << (30 - log)
    step = 1 << (31 - log)
    where = {M.eval_domain_index(log, i): i for i in range(1 << log)}
    return [M.bit_reverse_index(where[(init + k * step) & MASK31], log) for k in range(1 << log)]


def fib_rows_trace(log, a0, b0, break_at=None, bad_a0=None):
    """(a, b, is_first) in storage order; break_at: the coset row whose b is bumped (a broken transition); bad_a0: a wrong start."""
    n = 1 << log
    a, b = (a0 if bad_a0 is None else bad_a0) % P, b0 % P
    seq = []
    for k in range(n):
        if k == break_at:
            b = (b + 1) % P
        seq.append((a, b))
        a, b = b, (a * a + b * b) % P
    pos = coset_positions(log)
    ca, cb, first = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    for k, (x, y) in enumerate(seq):
        ca[pos[k]], cb[pos[k]] = x, y
    first[pos[0]] = 1
    return ca, cb, first


def fib_rows_constraints(a, b, pa, pb, first, a0, b0, mul, sub, one):
    nf = sub(one, first)
    return [mul(nf, sub(a, pb)), mul(nf, sub(sub(b, mul(pa, pa)), mul(pb, pb))), mul(first, sub(a, a0)), mul(first, sub(b, b0))]


def fib_rows_composition(log, cols, a0, b0, alpha):
    """The composition polynomial of FibonacciRows alone (eval domain log + 2): 4 coefficient arrays of 2^(log + 2)."""
    el = log + 2
    a, b, first = (M.extend(c, log, el) for c in cols)
    nb = neighbour_map(log, el, -1)
    mul = lambda x, y: x * y % P
    sub = lambda x, y: (x + P - y) % P
    one = np.ones(1 << el, dtype=np.uint64)
    cons = fib_rows_constraints(a, b, a[nb], b[nb], first, np.full_like(a, a0 % P), np.full_like(a, b0 % P), mul, sub, one)
    coeffs = M.component_coeffs(alpha, [len(cons)])[0]
    vals = _quotients(cons, log, 2, coeffs, M.denom_inv(log, el))
    return [M.interpolate(vals[j], el) for j in range(4)]


def _quotients(cons, trace_log, log_expand, coeffs, dinv):
    n = 1 << (trace_log + log_expand)
    rr = M.row_combination(coeffs, cons)
    d = np.asarray(dinv, dtype=np.uint64)[np.arange(n) >> trace_log]
    return np.stack([rr[j] * d % P for j in range(4)])


def shifted_point(point, log, offset):
    """point + offset * CanonicCoset(log).step (QM31 coordinates)."""
    s = M.lift(M.index_to_point((offset << (31 - log)) & MASK31))
    return M.padd(point, s, secure=True)


def fib_rows_point_values(log, cols, point):
    """Sampled values the verifier sees: a, b at [point - step, point] and is_first at point."""
    polys = [M.interpolate(c, log) for c in cols]
    prev = shifted_point(point, log, -1)
    return ([M.eval_at(polys[0], log, prev), M.eval_at(polys[0], log, point)],
            [M.eval_at(polys[1], log, prev), M.eval_at(polys[1], log, point)], M.eval_at(polys[2], log, point))


def fib_rows_composition_at_point(log, sampled, a0, b0, alpha, point):
    (pa, a), (pb, b), first = sampled
    cons = fib_rows_constraints(a, b, pa, pb, first, qm(a0), qm(b0), qmul, qsub, (1, 0, 0, 0))
    dinv = qinv(M.coset_vanishing(M.canonic_coset(log), point, secure=True))
    return M.point_horner(alpha, [qmul(c, dinv) for c in cons])


def deep_ali_holds(log, cols, a0, b0, alpha, t):
    """The composition polynomial (from the domain side) at a random point equals the constraints at that point over the mask."""
    point = M.random_point(t)
    comp = fib_rows_composition(log, cols, a0, b0, alpha)
    lhs = M.from_partial_evals([M.eval_at(comp[j], log + 2, point) for j in range(4)])
    rhs = fib_rows_composition_at_point(log, fib_rows_point_values(log, cols, point), a0, b0, alpha, point)
    return lhs == rhs

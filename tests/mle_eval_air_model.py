"""Integer model of the mle_eval component (tstwo_amd/mle_eval.py, csrc/mle_eval_air.hip) for
tests/test_cpu_mle_eval_air.py, tests/test_gpu_mle_eval_air.py and tests/test_gpu_gkr_stark.py.

It imports nothing from the package under test.  QM31 arithmetic and the eq table come from tests/gkr_model.py, the coset-order
running sum from tests/logup_model.py, and the row a mask offset reads from the geometry (air_program_model.neighbour_map on the
trace domain itself): nothing here assumes that an offset of +2 moves the circle-domain index by one, the tests check it.

Secure columns are numpy uint64 arrays of shape (4, n), base columns of shape (n,); scalars are QM31 4-tuples of ints."""
from __future__ import annotations

import numpy as np

import air_program_model as X
import gkr_model as G
import logup_model as LM
from gkr_model import ONE, P, ZERO, qadd, qinv, qm, qmul, qsub


def trailing_ones(x: int) -> int:
    t = 0
    while x & 1:
        x, t = x >> 1, t + 1
    return t


def t_of(p: int, n: int):
    """(first half?, t(p)) of storage position p: d = rev(p), d' = d mod h, t = trailing ones of d' (n - 1 for d' = h - 1)."""
    h = 1 << (n - 1)
    d = LM.rev(p, n)
    return d < h, trailing_ones(d % h)          # d' = h - 1 has n - 1 one bits: the same number


def selectors(n: int) -> list:
    """The 2n + 2 preprocessed columns G_0 .. G_{n-1}, K_0 .. K_{n-1}, F0, F1, from the definition, row by row."""
    size, h = 1 << n, 1 << (n - 1)
    cols = [np.zeros(size, dtype=np.uint64) for _ in range(2 * n + 2)]
    for p in range(size):
        first, t = t_of(p, n)
        cols[t if first else n + t][p] = 1
        d = LM.rev(p, n)
        if d == 0:
            cols[2 * n][p] = 1
        if d == h:
            cols[2 * n + 1][p] = 1
    return cols


def selectors_vec(n: int) -> np.ndarray:
    """The same columns as one (2n + 2, 2^n) uint32 array, vectorised (for the larger device cases)."""
    size, h = 1 << n, 1 << (n - 1)
    p = np.arange(size, dtype=np.int64)
    d = np.zeros(size, dtype=np.int64)
    for b in range(n):
        d |= ((p >> b) & 1) << (n - 1 - b)
    dp = d & (h - 1)
    t = np.zeros(size, dtype=np.int64)
    run = np.ones(size, dtype=bool)
    for b in range(n - 1):
        run &= ((dp >> b) & 1).astype(bool)
        t += run
    code = np.where(d < h, t, n + t)
    out = np.zeros((2 * n + 2, size), dtype=np.uint32)
    out[code, p] = 1
    out[2 * n, d == 0] = 1
    out[2 * n + 1, d == h] = 1
    return out


def constants(point):
    """(A, B, anchor_0, anchor_1): A_t = (1 - r_t) prod_{j<t} r_j, B_t = r_t prod_{j<t} (1 - r_j) for t < n - 1;
    A_{n-1} = prod_{j<n-1} r_j, B_{n-1} = prod_{j<n-1} (1 - r_j); the anchors prod_j (1 - r_j), r_{n-1} prod_{j<n-1} (1 - r_j)."""
    n = len(point)
    a, b = [], []
    for t in range(n - 1):
        pa, pb = qsub(ONE, point[t]), point[t]
        for j in range(t):
            pa, pb = qmul(pa, point[j]), qmul(pb, qsub(ONE, point[j]))
        a.append(pa)
        b.append(pb)
    pa = pb = ONE
    for j in range(n - 1):
        pa, pb = qmul(pa, point[j]), qmul(pb, qsub(ONE, point[j]))
    a.append(pa)
    b.append(pb)
    return a, b, qmul(pb, qsub(ONE, point[n - 1])), qmul(pb, point[n - 1])


def eq_table(point) -> np.ndarray:
    return G.gen_eq_evals(list(point), ONE)


def form_values(cols, coeffs, constant, size: int) -> np.ndarray:
    """constant + sum_k coeffs_k cols_k as a (4, n) array."""
    out = np.stack([np.full(size, int(c) % P, dtype=np.uint64) for c in constant])
    for col, w in zip(cols, coeffs):
        col = np.asarray(col, dtype=np.uint64)
        for j in range(4):
            out[j] = (out[j] + np.uint64(int(w[j])) * col % P) % P
    return out


def terms(eq, cols, coeffs, constant) -> np.ndarray:
    """tstwo_mle_eval_terms: eq[p] * form[p]."""
    eq = np.asarray(eq, dtype=np.uint64)
    return G.vmul(eq, form_values(cols, coeffs, constant, eq.shape[1]))


def interaction_trace(point, cols, coeffs, constant):
    """(E, S, sum): the eq table, the shifted coset-order running sum of E L, and sum_p E[p] L[p]."""
    e = eq_table(point)
    s, total = LM.finalize_last(terms(e, cols, coeffs, constant), len(point))
    return e, s, total


def _scaled(sel, consts, size):
    """sum_t consts_t sel_t as a (4, n) array."""
    out = np.zeros((4, size), dtype=np.uint64)
    for col, c in zip(sel, consts):
        for j in range(4):
            out[j] = (out[j] + np.uint64(int(c[j])) * np.asarray(col, dtype=np.uint64)) % P
    return out


def constraints(n, point, claim, cols, coeffs, constant, e, s, sel=None) -> list:
    """The three constraints on every storage row, as (4, 2^n) arrays; neighbours through the project's offset map."""
    size = 1 << n
    sel = selectors(n) if sel is None else sel
    a, b, anchor0, anchor1 = constants(point)
    g, k, f0, f1 = sel[:n], sel[n:2 * n], sel[2 * n], sel[2 * n + 1]
    e, s = np.asarray(e, dtype=np.uint64), np.asarray(s, dtype=np.uint64)
    e_next, e_prev = e[:, X.neighbour_map(n, n, 2)], e[:, X.neighbour_map(n, n, -2)]
    s_prev = s[:, X.neighbour_map(n, n, -1)]
    both = [(gt + kt) % P for gt, kt in zip(g, k)]
    step = G.vsub(G.vadd(G.vmul(_scaled(g, a, size), e_next), G.vmul(_scaled(k, a, size), e_prev)), G.vmul(_scaled(both, b, size), e))
    c0 = np.stack([np.full(size, v, dtype=np.uint64) for v in anchor0])
    c1 = np.stack([np.full(size, v, dtype=np.uint64) for v in anchor1])
    anchors = G.vadd(G.vmul_base(G.vsub(e, c0), np.asarray(f0, dtype=np.uint64)), G.vmul_base(G.vsub(e, c1), np.asarray(f1, dtype=np.uint64)))
    shift = qmul(claim, qm(pow(size, P - 2, P)))
    sh = np.stack([np.full(size, v, dtype=np.uint64) for v in shift])
    total = G.vadd(G.vsub(G.vsub(s, s_prev), G.vmul(e, form_values(cols, coeffs, constant, size))), sh)
    return [step, anchors, total]


def constraints_at(n, point, claim, coeffs, constant, sel, cols, e_prev, e, e_next, s_prev, s) -> list:
    """The three constraints over QM31 scalars: sel (2n + 2 values), cols (the form's columns) and the mask values of E at
    [-2, 0, 2] and S at [-1, 0], all QM31 4-tuples (what the verifier holds at the out-of-domain point)."""
    a, b, anchor0, anchor1 = constants(point)
    g, k, f0, f1 = sel[:n], sel[n:2 * n], sel[2 * n], sel[2 * n + 1]
    a_next = a_prev = b_here = ZERO
    for t in range(n):
        a_next = qadd(a_next, qmul(a[t], g[t]))
        a_prev = qadd(a_prev, qmul(a[t], k[t]))
        b_here = qadd(b_here, qmul(b[t], qadd(g[t], k[t])))
    step = qsub(qadd(qmul(a_next, e_next), qmul(a_prev, e_prev)), qmul(b_here, e))
    anchors = qadd(qmul(f0, qsub(e, anchor0)), qmul(f1, qsub(e, anchor1)))
    form = constant
    for w, c in zip(coeffs, cols):
        form = qadd(form, qmul(w, c))
    total = qadd(qsub(qsub(s, s_prev), qmul(e, form)), qmul(claim, qm(pow(1 << n, P - 2, P))))
    return [step, anchors, total]


def failing_rows(values) -> np.ndarray:
    """The storage rows on which a constraint (a (4, n) array) is non-zero."""
    return np.nonzero(np.asarray(values).any(axis=0))[0]


def walk(n, point) -> np.ndarray:
    """The table constraints 1 and 2 force: from the anchors, row by row along the offsets +2 (first half) and -2 (second)."""
    size = 1 << n
    a, b, anchor0, anchor1 = constants(point)
    sel = selectors(n)
    nxt, prv = X.neighbour_map(n, n, 2), X.neighbour_map(n, n, -2)
    out = [None] * size
    for start_col, value, step in ((2 * n, anchor0, nxt), (2 * n + 1, anchor1, prv)):
        [p] = np.nonzero(sel[start_col])[0]
        p = int(p)
        for _ in range(size // 2):
            assert out[p] is None
            out[p] = value
            _, t = t_of(p, n)
            value = qmul(value, qmul(b[t], qinv(a[t])))         # A_t E[neighbour] = B_t E[here]
            p = int(step[p])
    assert all(v is not None for v in out)
    return np.array(out, dtype=np.uint64).T


def coset_row_of(p: int, n: int) -> int:
    """The coset-order row stored at position p."""
    return int(np.nonzero(LM.positions(n) == p)[0][0])


def random_point(rng, n):
    return [G.random_felt(rng) for _ in range(n)]


__all__ = ["ONE", "P", "ZERO", "qadd", "constants", "constraints", "coset_row_of", "eq_table", "failing_rows", "form_values",
           "interaction_trace", "random_point", "selectors", "selectors_vec", "t_of", "terms", "trailing_ones", "walk"]

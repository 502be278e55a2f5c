"""Integer model of LogUp (Rust stwo constraint_framework/logup.rs) for tests/test_cpu_logup.py and tests/test_gpu_logup.py.

It imports nothing from the package under test: QM31 arithmetic comes from tests/gkr_model.py, coset-order positions from the
geometry (tests/air_program_model.py).  Secure columns are numpy uint64 arrays of shape (4, n)."""
from __future__ import annotations

import numpy as np

import air_program_model as X
from gkr_model import P, ONE, ZERO, qadd, qinv, qm, qmul, qsub, vmul, vmul_base, lift


def rev(x, bits):
    r = 0
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


def position(k, n):
    """Storage position of coset row k of a column of 2^n rows (the formula of csrc/logup.hip)."""
    j, half = k >> 1, 1 << (n - 1)
    r = rev(j, n - 1)
    return 2 * r if k % 2 == 0 else 2 * (half - 1 - r) + 1


def positions(log):
    """position(k, log) for every k, vectorised."""
    k = np.arange(1 << log, dtype=np.int64)
    j, r = k >> 1, np.zeros(1 << log, dtype=np.int64)
    for _ in range(log - 1):
        r, j = (r << 1) | (j & 1), j >> 1
    return np.where(k % 2 == 0, 2 * r, 2 * ((1 << (log - 1)) - 1 - r) + 1)


def alpha_powers(alpha, size):
    out = [ONE]
    while len(out) < size:
        out.append(qmul(out[-1], alpha))
    return out


def combine(z, alpha, values):
    """sum_i alpha^i values[i] - z over QM31 4-tuples (ints are M31 values)."""
    acc = ZERO
    for v, p in zip(values, alpha_powers(alpha, len(values))):
        acc = qadd(acc, qmul(p, v if isinstance(v, tuple) else qm(v)))
    return qsub(acc, z)


def combine_cols(z, alpha, values, n):
    """combine() on columns: values are (n,) uint64 arrays or ints; a (4, n) array."""
    out = np.zeros((4, n), dtype=np.uint64)
    for j in range(4):
        out[j] = (P - z[j]) % P
    for v, p in zip(values, alpha_powers(alpha, len(values))):
        col = np.full(n, int(v) % P, dtype=np.uint64) if isinstance(v, int) else np.asarray(v, dtype=np.uint64)
        out = (out + vmul_base(np.stack([np.full(n, c, dtype=np.uint64) for c in p]), col)) % P
    return out


def column_identity_holds(out, prev, fracs):
    """(out - prev) * prod den == sum_b num_b * prod_{b' != b} den_b' on every row (no inversion).  fracs: [(num (n,), den (4, n))]."""
    diff = (out + (P - prev)) % P
    dens = [d for _, d in fracs]
    full = dens[0]
    for d in dens[1:]:
        full = vmul(full, d)
    lhs = vmul(diff, full)
    rhs = np.zeros_like(lhs)
    for b, (num, _) in enumerate(fracs):
        t = lift(np.asarray(num, dtype=np.uint64) % P)
        for b2, d in enumerate(dens):
            if b2 != b:
                t = vmul(t, d)
        rhs = (rhs + t) % P
    return np.array_equal(lhs, rhs)


def column(fracs, prev, n):
    """prev + sum num / den, with a per-row inversion (small n only)."""
    out = np.zeros((4, n), dtype=np.uint64) if prev is None else prev.copy()
    for r in range(n):
        acc = tuple(int(v) for v in out[:, r])
        for num, den in fracs:
            acc = qadd(acc, qmul(qm(int(num[r])), qinv(tuple(int(v) for v in den[:, r]))))
        out[:, r] = acc
    return out


def finalize_last(col, log):
    """(the shifted coset-order running sum, claimed sum): claimed = sum of all rows, value at coset row k = sum_{k' <= k}
    (col[pos(k')] - claimed / 2^log)."""
    n = 1 << log
    claimed = tuple(int(v) for v in col.sum(axis=1, dtype=np.uint64) % P)
    inv_n = pow(n, P - 2, P)
    s = [c * inv_n % P for c in claimed]
    pos = np.asarray(X.coset_positions(log)) if log <= 11 else positions(log)
    out = np.empty_like(col)
    for j in range(4):
        vals = (col[j][pos] + (P - s[j])) % P
        out[j][pos] = np.cumsum(vals, dtype=np.uint64) % P
    return out, claimed

"""Integer model of tstwo_air_check_constraints, for tests/test_cpu_air_check.py, tests/test_gpu_air_check.py and
tests/test_gpu_air_diagnose.py.

It imports nothing from the package under test.  The per-ACC values are air_program_model.run_program with log_expand 0 (what
columns_model.run_columns uses: loads at offsets go through neighbour_map(log, log, offset), which finds neighbours from the
geometry); the coset row of a storage position comes from logup_model.positions.  A constraint is a group of ACCs: it is
non-zero on a row when one of its ACCs is.
"""
from __future__ import annotations

import numpy as np

import air_program_model as X
import logup_model as LM

P = LM.P
NO_ROW = 0xffffffff


def with_groups(words, groups):
    """The program with the k-th ACC's w1 set to groups[k] (what constraint_framework.check_program uploads)."""
    words, k = list(words), 0
    for pc in range(len(words) // 2):
        if words[2 * pc] & 0xff == X.ACC:
            words[2 * pc + 1] = groups[k] & 0xffffffff
            k += 1
    assert k == len(groups)
    return words


def grouping(sizes):
    """ACC k -> constraint index, for constraints of the given numbers of ACCs: grouping([1, 4, 1]) = [0, 1, 1, 1, 1, 2]."""
    return [c for c, size in enumerate(sizes) for _ in range(size)]


def coset_rows(log):
    """coset_rows(log)[r] = the coset-order row stored at position r."""
    pos = LM.positions(log)
    rows = np.empty(1 << log, dtype=np.int64)
    rows[pos] = np.arange(1 << log)
    return rows


def report(words, cols, log, groups):
    """[(n_rows, first_row)] per constraint: the number of rows on which one of its ACCs is non-zero and the smallest of them in
    coset order (NO_ROW when there is none)."""
    values = X.run_program(words, [np.asarray(c, dtype=np.uint64) for c in cols], log, 0)
    assert len(values) == len(groups)
    rows = coset_rows(log)
    out = []
    for c in range(groups[-1] + 1):
        nz = np.zeros(1 << log, dtype=bool)
        for v, g in zip(values, groups):
            if g == c:
                nz |= (np.asarray(v, dtype=np.uint64) % P) != 0
        out.append((int(nz.sum()), int(rows[nz].min()) if nz.any() else NO_ROW))
    return out


def report_words(words, cols, log, groups):
    """The report as the device writes it: 2 words per constraint."""
    return np.array([w for pair in report(words, cols, log, groups) for w in pair], dtype=np.uint32)

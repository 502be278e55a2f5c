"""Integer model of tstwo_air_eval_columns and of an interaction trace derived from `evaluate`, for
tests/test_cpu_interaction_trace.py, tests/test_gpu_air_columns.py and tests/test_gpu_interaction_trace.py.

It imports nothing from the package under test.  A columns program is a constraint program on the trace domain itself with STORE
in place of ACC, so run_columns is air_program_model.run_program with log_expand 0: its loads at offsets go through
neighbour_map(log, log, offset), which finds neighbours from the geometry.  interaction_trace is logup_model.column per batch and
logup_model.finalize_last on the last column.
"""
from __future__ import annotations

import numpy as np

import air_program_model as X
import logup_model as LM

P = LM.P
STORE = 8                       # include/tstwo_hip.h TSTWO_AIR_OP_STORE


def stores_for_accs(words):
    """A program of air_program_model.random_program with its k-th ACC turned into STORE k."""
    words, k = list(words), 0
    for pc in range(len(words) // 2):
        if words[2 * pc] & 0xff == X.ACC:
            words[2 * pc:2 * pc + 2] = X.encode(STORE, 0, words[2 * pc] >> 16, k)
            k += 1
    return words, k


def run_columns(words, cols, log, n_out):
    """The n_out output columns (numpy uint64) of a columns program over `cols` on CanonicCoset(log).circle_domain()."""
    acc_words, index = [], []
    for pc in range(len(words) // 2):
        w0, w1 = words[2 * pc], words[2 * pc + 1]
        if w0 & 0xff == STORE:
            acc_words += X.encode(X.ACC, 0, w0 >> 16)
            index.append(w1)
        else:
            assert w0 & 0xff != X.ACC, "ACC is a bad opcode in a columns program"
            acc_words += [w0, w1]
    assert sorted(index) == list(range(n_out)), "every output index below n_out is stored exactly once"
    cols = [np.asarray(c, dtype=np.uint64) for c in cols]
    values = X.run_program(acc_words, cols, log, 0)
    out = [None] * n_out
    for k, v in zip(index, values):
        out[k] = np.asarray(v, dtype=np.uint64) % P
    return out


def shift_in_coset_order(col, log, offset):
    """col read `offset` rows further in coset order, through logup_model.positions: the second definition of a row offset."""
    pos = LM.positions(log)
    seq = np.asarray(col)[pos]
    out = np.empty_like(seq)
    out[pos] = np.roll(seq, -offset)
    return out


def interaction_trace(fracs_per_batch, log):
    """(columns, claimed sum): one (4, n) uint64 column per batch, column j = column j - 1 + sum num / den over the batch's
    fractions [(num (n,), den (4, n))], the last one turned into its shifted running sum."""
    n = 1 << log
    cols, prev = [], None
    for fracs in fracs_per_batch:
        prev = LM.column([(np.asarray(num, dtype=np.uint64) % P, den) for num, den in fracs], prev, n)
        cols.append(prev)
    cols[-1], claimed = LM.finalize_last(cols[-1], log)
    return cols, claimed

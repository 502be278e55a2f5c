#!/usr/bin/env python3
"""The interpreted constraint kernel (tstwo_air_eval_program) on one MI355X, against the hand-written one.

Per log size (16, 18, 20, 22 by default), each kernel alone, timed with HIP events (median of --reps launches after a warm-up):
  wide_fib_hand     k_constraint_quotients<WIDE_FIB, 4>: wide Fibonacci, N = 100 columns, on the evaluation domain (log + 1)
  wide_fib_program  the same trace through tstwo_air_eval_program, WideFibonacciEval compiled by the constraint framework
  fib_rows_program  FibonacciRowsEval (2 main columns read at offsets -1 and 0, the is_first column; degree 3, domain log + 2)
Both wide-Fibonacci runs read the same device columns and must give the same accumulation (checked once per size).
Algorithmic bytes = (columns + 8) * 4 * rows: every column read once plus the accumulator's read-modify-write (4 coordinates); the
HBM bound is those bytes at 6.3 TB/s (as tools/bench_prove.py).  Prints one JSON line.

    python tools/bench_air_program.py [--logs 16,18,20,22] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tstwo_amd import _lib as L                                   # noqa: E402
from tstwo_amd import air as A                                    # noqa: E402
from tstwo_amd import constraint_framework as F                   # noqa: E402
from tstwo_amd.backend import HipColumn, SecureColumnByCoords     # noqa: E402
from tstwo_amd.fields import P, QM31                              # noqa: E402

HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)
N_COLS = 100


def time_ms(fn, reps):
    fn()
    L.sync()
    ts = []
    for _ in range(reps):
        e0, e1 = L.Event(), L.Event()
        e0.record()
        fn()
        e1.record()
        ts.append(e0.elapsed_ms(e1))
    return statistics.median(ts)


def entry(ms, n_cols, rows):
    b = (n_cols + 8) * 4 * rows
    return {"ms": ms, "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3, "achieved_tb_s": b / ms / 1e9,
            "frac_hbm": b / HBM_COPY * 1e3 / ms}


def run(log, reps, rng):
    res = {"log": log}
    coeff = QM31.from_u32_unchecked(*[int(v) for v in rng.integers(0, P, size=4)])
    # wide Fibonacci on its evaluation domain (log + 1): the trace kernel writes the 100 columns straight there
    el = log + 1
    rows = 1 << el
    cols = [e.values for e in A.generate_wide_fib_trace(el, rng.integers(0, P, size=rows), rng.integers(0, P, size=rows), N_COLS)]
    dinv = A.denominator_inverses(log, el)
    acc_h, acc_p = SecureColumnByCoords.zeros(rows), SecureColumnByCoords.zeros(rows)
    pe = F.ProgramEvaluator()                  # the library eval runs on the hand-written kernel: compile its program here
    F.WideFibonacciEval(log, N_COLS).evaluate(pe)
    program = pe.compile()
    coeffs = [coeff] * program.n_constraints
    A.evaluate_constraint_quotients(A.AIR_WIDE_FIB, cols, log, 1, coeffs, dinv, acc_h)
    F.evaluate_program(cols, log, 1, program, coeffs, dinv, acc_p)
    same = all(np.array_equal(x, y) for x, y in zip(acc_h.to_numpy(), acc_p.to_numpy()))
    hand = time_ms(lambda: A.evaluate_constraint_quotients(A.AIR_WIDE_FIB, cols, log, 1, coeffs, dinv, acc_h), reps)
    prog = time_ms(lambda: F.evaluate_program(cols, log, 1, program, coeffs, dinv, acc_p), reps)
    res["wide_fib_hand"] = entry(hand, N_COLS, rows)
    res["wide_fib_program"] = entry(prog, N_COLS, rows)
    res["wide_fib_program"].update({"n_instr": program.n_instr, "n_regs": program.n_regs, "same_result": same})
    res["program_over_hand"] = prog / hand
    del cols, acc_h, acc_p
    # FibonacciRowsEval on its evaluation domain (log + 2); random values: the kernel's work does not depend on them
    el = log + 2
    rows = 1 << el
    fr = F.FrameworkComponent(F.FibonacciRowsEval(log, 1, 1), None, [0])
    fcols = [HipColumn(rng.integers(0, P, size=rows).astype(np.uint32)) for _ in range(3)]
    acc = SecureColumnByCoords.zeros(rows)
    fdinv = A.denominator_inverses(log, el)
    fcoeffs = [coeff] * fr.n_constraints
    ms = time_ms(lambda: F.evaluate_program(fcols, log, 2, fr.program, fcoeffs, fdinv, acc), reps)
    res["fib_rows_program"] = entry(ms, 3, rows)
    res["fib_rows_program"].update({"n_instr": fr.program.n_instr, "n_regs": fr.program.n_regs})
    L.sync()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20,22")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L.init(0)
    rng = np.random.default_rng(0)
    run(10, 3, rng)                                  # warm-up: kernels loaded, pools filled
    out = {"tool": "bench_air_program", "device": L.device_name(), "runs": [run(int(x), args.reps, rng) for x in args.logs.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

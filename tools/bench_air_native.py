#!/usr/bin/env python3
"""The native constraint kernels (tstwo_air_program_compile / tstwo_air_eval_compiled) on one MI355X, against the interpreter and
the hand-written kernel.

Per log size (16, 18, 20, 22 by default), timed with HIP events; the methods ALTERNATE launch by launch in one process (one round
= one launch of each), and each is reported as the median of --reps rounds after a warm-up round, with the min and max beside it:
  wide_fib   wide Fibonacci, N = 100 columns, on the evaluation domain (log + 1): hand (k_constraint_quotients<WIDE_FIB, 4>),
             interp (tstwo_air_eval_program) and native, on the same device columns; the three accumulations must agree
  fib_rows   FibonacciRowsEval (2 main columns read at offsets -1 and 0, the is_first column; degree 3, domain log + 2): interp
             and native
The compile wall time and the resource figures (tstwo_air_kernel_info) are recorded per program.  Algorithmic bytes and the HBM
bound as tools/bench_air_program.py.  Prints one JSON line.

    python tools/bench_air_native.py [--logs 16,18,20,22] [--reps 20]
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


def time_alternating(fns: dict, reps: int) -> dict:
    """{name: [ms per round]}: every round launches each method once, in order, each between its own pair of events"""
    for fn in fns.values():                # warm-up round
        fn()
    L.sync()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = L.Event(), L.Event()
            e0.record()
            fn()
            e1.record()
            ts[name].append(e0.elapsed_ms(e1))
    return ts


def entry(ts, n_cols, rows):
    ms = statistics.median(ts)
    b = (n_cols + 8) * 4 * rows
    return {"ms": ms, "min_ms": min(ts), "max_ms": max(ts), "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3, "achieved_tb_s": b / ms / 1e9,
            "frac_hbm": b / HBM_COPY * 1e3 / ms}


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.to_numpy(), b.to_numpy()))


def run(log, reps, rng):
    res = {"log": log}
    coeff = QM31.from_u32_unchecked(*[int(v) for v in rng.integers(0, P, size=4)])
    # wide Fibonacci on its evaluation domain (log + 1): the trace kernel writes the 100 columns straight there
    el = log + 1
    rows = 1 << el
    cols = [e.values for e in A.generate_wide_fib_trace(el, rng.integers(0, P, size=rows), rng.integers(0, P, size=rows), N_COLS)]
    dinv = A.denominator_inverses(log, el)
    accs = {m: SecureColumnByCoords.zeros(rows) for m in ("hand", "interp", "native")}
    pe = F.ProgramEvaluator()                  # the library eval runs on the hand-written kernel: compile its program here
    F.WideFibonacciEval(log, N_COLS).evaluate(pe)
    program = pe.compile()
    kernel = F.compile_native(program, N_COLS)
    coeffs = [coeff] * program.n_constraints
    fns = {"hand": lambda: A.evaluate_constraint_quotients(A.AIR_WIDE_FIB, cols, log, 1, coeffs, dinv, accs["hand"]),
           "interp": lambda: F.evaluate_program(cols, log, 1, program, coeffs, dinv, accs["interp"]),
           "native": lambda: F.evaluate_program_native(cols, log, 1, kernel, coeffs, dinv, accs["native"])}
    for fn in fns.values():
        fn()
    agree = same(accs["hand"], accs["interp"]) and same(accs["hand"], accs["native"])
    ts = time_alternating(fns, reps)
    wf = {m: entry(t, N_COLS, rows) for m, t in ts.items()}
    wf.update({"n_instr": program.n_instr, "same_result": agree, "kernel": kernel.info(),
               "native_over_hand": wf["native"]["ms"] / wf["hand"]["ms"], "interp_over_native": wf["interp"]["ms"] / wf["native"]["ms"],
               # faster by more than the spread of the two: the slowest native launch against the fastest interpreted one
               "native_max_below_interp_min": wf["native"]["max_ms"] < wf["interp"]["min_ms"]})
    res["wide_fib"] = wf
    del cols, accs, fns
    # FibonacciRowsEval on its evaluation domain (log + 2); random values: the kernel's work does not depend on them
    el = log + 2
    rows = 1 << el
    fr = F.FrameworkComponent(F.FibonacciRowsEval(log, 1, 1), None, [0], native=True)
    fcols = [HipColumn(rng.integers(0, P, size=rows).astype(np.uint32)) for _ in range(3)]
    faccs = {m: SecureColumnByCoords.zeros(rows) for m in ("interp", "native")}
    fdinv = A.denominator_inverses(log, el)
    fcoeffs = [coeff] * fr.n_constraints
    ffns = {"interp": lambda: F.evaluate_program(fcols, log, 2, fr.program, fcoeffs, fdinv, faccs["interp"]),
            "native": lambda: F.evaluate_program_native(fcols, log, 2, fr.native, fcoeffs, fdinv, faccs["native"])}
    for fn in ffns.values():
        fn()
    agree = same(faccs["interp"], faccs["native"])
    ts = time_alternating(ffns, reps)
    rw = {m: entry(t, 3, rows) for m, t in ts.items()}
    rw.update({"n_instr": fr.program.n_instr, "same_result": agree, "kernel": fr.native_info(),
               "interp_over_native": rw["interp"]["ms"] / rw["native"]["ms"],
               "native_max_below_interp_min": rw["native"]["max_ms"] < rw["interp"]["min_ms"]})
    res["fib_rows"] = rw
    L.sync()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20,22")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L.init(0)
    rng = np.random.default_rng(0)
    run(10, 3, rng)                                  # warm-up: kernels compiled and loaded, pools filled
    out = {"tool": "bench_air_native", "device": L.device_name(), "reps": args.reps,
           "runs": [run(int(x), args.reps, rng) for x in args.logs.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

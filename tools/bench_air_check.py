#!/usr/bin/env python3
"""tstwo_air_check_constraints on one MI355X against the way to get the same answer without it.

The 100-column wide Fibonacci program (98 constraints) on a clean trace at log 20 (by default):
  check    one tstwo_air_check_constraints call: 2 words per constraint come back.
  columns  the same constraints as outputs of tstwo_air_eval_columns, in two calls of at most 64 outputs (64 + 34): one
           2^log column per constraint is written (and would still have to be read back and searched).
Both timed with HIP events around the call(s), alternating inside every repetition after a warm-up of each; median and range of
--reps.  The report is checked to be clean and every output column to be zero before anything is timed.  Algorithmic bytes: the
100 input columns once for the check, and for the columns calls 66 + 36 input columns and 98 output columns.
Prints one JSON line and writes it to --out.

    python tools/bench_air_check.py [--log 20] [--reps 30] [--out profiles/bench_air_check.json]
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
from tstwo_amd.backend import HipColumn                           # noqa: E402
from tstwo_amd.fields import P                                    # noqa: E402

N_COLS = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_air_check.json"))
    args = ap.parse_args()
    log, n = args.log, 1 << args.log
    L.init(0)
    rng = np.random.default_rng(0)
    cols = [e.values for e in A.generate_wide_fib_trace(log, rng.integers(0, P, size=n), rng.integers(0, P, size=n), N_COLS)]
    ptrs = L.ptr_array([c.ptr for c in cols])
    comp = F.WideFibonacciComponent(log, N_COLS)
    program = comp._constraint_program()
    n_constraints = comp.n_constraints
    words = list(program.words)
    k = 0
    for pc in range(program.n_instr):                   # ACC k belongs to constraint k
        if words[2 * pc] & 0xff == F.OP_ACC:
            words[2 * pc + 1] = k
            k += 1
    assert k == n_constraints == N_COLS - 2
    check_words = L.u32x(words)
    report = HipColumn.uninitialized(2 * n_constraints)

    def check():
        L.call("tstwo_air_check_constraints", ptrs, N_COLS, log, check_words, program.n_instr, n_constraints, L.vp(report.ptr))

    # the same constraints as output columns: two programs of at most MAX_OUT outputs over all 100 columns
    pe = F.ProgramEvaluator()
    comp.eval.evaluate(pe)
    halves = [F.compile_columns(pe.constraints[i:i + F.MAX_OUT], N_COLS) for i in range(0, n_constraints, F.MAX_OUT)]
    outs = [[HipColumn.uninitialized(n) for _ in range(h.n_out)] for h in halves]
    calls = [(L.u32x(h.words), h.n_instr, L.ptr_array([c.ptr for c in o]), h.n_out) for h, o in zip(halves, outs)]

    def columns():
        for w, n_instr, out, n_out in calls:
            L.call("tstwo_air_eval_columns", ptrs, N_COLS, log, w, n_instr, out, n_out)

    check(); columns(); L.sync()
    assert report.to_numpy().tolist() == [0, 0xffffffff] * n_constraints, "the trace is not clean"
    assert all(not o[j].to_numpy().any() for o in outs for j in (0, len(o) - 1)), "a constraint column is not zero"
    ts = {"check": [], "columns": []}
    for _ in range(args.reps):
        for name, fn in (("check", check), ("columns", columns)):
            e0, e1 = L.Event(), L.Event()
            e0.record()
            fn()
            e1.record()
            ts[name].append(e0.elapsed_ms(e1))
    res = {"device": L.device_name(), "log": log, "n_cols": N_COLS, "n_constraints": n_constraints, "reps": args.reps,
           "check_instr": program.n_instr, "columns_instr": [h.n_instr for h in halves], "columns_outputs": [h.n_out for h in halves]}
    for name, t in ts.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    res["columns_over_check"] = round(res["columns_ms"]["median"] / res["check_ms"]["median"], 2)
    res["check_bytes"] = 4 * n * N_COLS
    res["columns_bytes"] = 4 * n * (sum(h.n_out + 2 for h in halves) + n_constraints)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

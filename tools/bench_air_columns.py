#!/usr/bin/env python3
"""tstwo_air_eval_columns and derive_interaction_trace on one MI355X.

(a) The kernel, per log size (16, 20, 22 by default), timed with HIP events (median of --reps calls after a warm-up), for two
    programs: `negation` (LOAD, NEG, STORE: what RangeCheckTableEval's -multiplicity compiles to) and `general` (the five
    expressions m s, a b - c@-1, a^2, -m, c@+2 over five columns).  Algorithmic bytes: (distinct loads + stores) x 4 x rows; the
    HBM bound is those bytes at 6.3 TB/s.
(b) The interaction trace of RangeCheckTableEval from a multiplicity column that is on the device: derive_interaction_trace
    (one columns program for -multiplicity, the preprocessed column on the device as well) against the hand-written
    range_check_table_interaction_trace (downloads the multiplicities, negates them in numpy, uploads them and the table column
    again).  Host wall time ended by a device synchronisation, the two alternating, median of --reps; `ratio` is hand-written
    over derived.
(c) --native: part (a) for the interpreter (tstwo_air_eval_columns) and for the native kernel of the same program
    (tstwo_air_columns_compile / tstwo_air_eval_columns_compiled) in the same process, the two alternating inside every
    repetition, with the outputs of both compared at every size; the compile wall time and the kernel's resources
    (tstwo_air_kernel_info) are reported per program, apart from the run times.  Part (b) is timed with native=False and True.
Prints one JSON line and writes it to --out.

    python tools/bench_air_columns.py [--logs 16,20,22] [--reps 10] [--out profiles/r14_bench_air_columns.json]
    python tools/bench_air_columns.py --native [--out profiles/bench_air_columns_native.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tstwo_amd import _lib as L                                   # noqa: E402
from tstwo_amd import constraint_framework as F                   # noqa: E402
from tstwo_amd import logup as LG                                 # noqa: E402
from tstwo_amd.air import ORIGINAL_TRACE_IDX                      # noqa: E402
from tstwo_amd.backend import HipColumn                           # noqa: E402
from tstwo_amd.fields import P, QM31                              # noqa: E402

HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)


class GeneralEval:
    """Main columns a, b, c (read at rows -1 and +2), m; preprocessed s.  Entries (m s, [a b - c@-1, a^2, 7]) and (-m, [c@+2])."""

    def __init__(self, log, elements):
        self.log, self.elements = log, elements

    def log_size(self):
        return self.log

    def evaluate(self, eval):
        s = eval.get_preprocessed_column(0)
        a, b = eval.next_trace_mask(), eval.next_trace_mask()
        c_prev, c_next = eval.next_interaction_mask(ORIGINAL_TRACE_IDX, [-1, 2])
        m = eval.next_trace_mask()
        eval.add_to_relation(LG.RelationEntry(self.elements, m * s, [a * b - c_prev, a.square(), 7]))
        eval.add_to_relation(LG.RelationEntry(self.elements, -m, [c_next]))
        eval.finalize_logup_in_pairs()
        return eval


def event_ms(fn, reps):
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


def event_ms_alternating(fns, reps):
    """event_ms for several functions at once: each warmed up, then one call of each per repetition, in turn."""
    for fn in fns:
        fn()
    L.sync()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = L.Event(), L.Event()
            e0.record()
            fn()
            e1.record()
            ts[k].append(e0.elapsed_ms(e1))
    return [statistics.median(t) for t in ts]


def entry(ms, b):
    return {"ms": ms, "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3, "achieved_tb_s": b / ms / 1e9, "frac_hbm": b / HBM_COPY * 1e3 / ms}


def felt(rng):
    return QM31.from_u32_unchecked(*[int(v) for v in rng.integers(0, P, size=4)])


def kernel(log, reps, rng, native=False):
    n = 1 << log
    le = LG.LookupElements(felt(rng), felt(rng), 3)
    cols = [HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(5)]
    res = {"log": log}
    for name, eval_, n_main, n_pre in (("negation", F.RangeCheckTableEval(log, le), 1, 1), ("general", GeneralEval(log, le), 4, 1)):
        plan = LG.plan_interaction_trace(eval_)
        program = F.compile_columns(plan.exprs, n_main, n_pre)
        loads = {(program.words[2 * i] >> 16, program.words[2 * i + 1]) for i in range(program.n_instr) if program.words[2 * i] & 0xff == F.OP_LOAD}
        ins, nbytes = cols[:n_main + n_pre], (len(loads) + program.n_out) * 4 * n
        shape = dict(n_instr=program.n_instr, n_regs=program.n_regs, distinct_loads=len(loads), stores=program.n_out)
        if not native:
            ms = event_ms(lambda: F.evaluate_columns(ins, log, program, program.n_out), reps)
            res[name] = dict(entry(ms, nbytes), **shape)
            continue
        kernel_ = F.compile_columns_native(program, len(ins))          # compiled here, outside every timed window
        same = all(np.array_equal(a.to_numpy(), b.to_numpy()) for a, b in zip(F.evaluate_columns(ins, log, program, program.n_out),
                                                                             F.evaluate_columns(ins, log, program, program.n_out, native=True)))
        ms_i, ms_n = event_ms_alternating([lambda: F.evaluate_columns(ins, log, program, program.n_out),
                                           lambda: F.evaluate_columns(ins, log, program, program.n_out, native=True)], reps)
        res[name] = dict(shape, bytes=nbytes, hbm_bound_ms=nbytes / HBM_COPY * 1e3, interpreter=entry(ms_i, nbytes), native=entry(ms_n, nbytes),
                         speedup=ms_i / ms_n, same_outputs=bool(same), compile_seconds=kernel_.compile_seconds,
                         kernel_info={k: v for k, v in kernel_.info().items() if k != "compile_seconds"})
    return res


def wall_ms(fn):
    L.sync()
    t0 = time.perf_counter()
    fn()
    L.sync()
    return (time.perf_counter() - t0) * 1e3


def range_check_table(log, reps, rng, native=False):
    le = LG.LookupElements(felt(rng), felt(rng), 1)
    mult = HipColumn(F.range_check_multiplicities(log, rng.integers(0, 1 << log, size=1 << log)))
    table = HipColumn(F.range_check_table_column(log))
    eval_ = F.RangeCheckTableEval(log, le)
    derived = lambda: LG.derive_interaction_trace(eval_, [mult], [table])                 # noqa: E731
    hand = lambda: F.range_check_table_interaction_trace(log, mult, le)                   # noqa: E731
    (d_ev, d_sum), (h_ev, h_sum) = derived(), hand()
    same = d_sum == h_sum and all(np.array_equal(d.values.to_numpy(), h.values.to_numpy()) for d, h in zip(d_ev, h_ev))
    del d_ev, h_ev
    td, th = [], []
    for _ in range(reps):
        td.append(wall_ms(derived))
        th.append(wall_ms(hand))
    d, h = statistics.median(td), statistics.median(th)
    res = {"log": log, "derived_ms": d, "hand_written_ms": h, "ratio": h / d, "same_trace": bool(same)}
    if native:
        derived_native = lambda: LG.derive_interaction_trace(eval_, [mult], [table], native=True)     # noqa: E731
        n_ev, n_sum = derived_native()
        (d_ev, d_sum) = derived()
        res["same_trace_native"] = bool(n_sum == d_sum and all(np.array_equal(a.values.to_numpy(), b.values.to_numpy()) for a, b in zip(n_ev, d_ev)))
        del n_ev, d_ev
        td, tn = [], []
        for _ in range(reps):
            td.append(wall_ms(derived))
            tn.append(wall_ms(derived_native))
        res.update(derived_ms=statistics.median(td), derived_native_ms=statistics.median(tn))
        res["ratio"] = h / res["derived_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20,22")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--native", action="store_true", help="time the interpreter and the native kernels side by side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bench_air_columns_native.json" if a.native else "r14_bench_air_columns.json")
    if a.reps < 10:
        raise SystemExit("--reps: at least 10")
    logs = [int(x) for x in a.logs.split(",") if x]
    L.init(0)
    rng = np.random.default_rng(0)
    out = {"device": L.device_name(), "reps": a.reps, "hbm_tb_s": HBM_COPY / 1e12,
           "kernel": [kernel(lg, a.reps, rng, a.native) for lg in logs],
           "range_check_table": [range_check_table(lg, a.reps, rng, a.native) for lg in logs]}
    if a.native:
        out["native"] = True
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

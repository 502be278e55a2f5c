#!/usr/bin/env python3
"""The device steps of the mle_eval component on one MI355X (csrc/mle_eval_air.hip), beside the closest existing kernel.

Per log size (20 and 24 by default) and per number of terms (1 and 4), in ONE run, timed with HIP events (median of --reps
launches after 2 warm-ups, min and max kept):
  terms_t{T}          tstwo_mle_eval_terms over T columns: reads 16 (eq) + 4 T, writes 16 bytes per row
  logup_column_t{T}   tstwo_logup_column with one fraction of T terms over the SAME columns, a column numerator, no previous
                      column: reads 4 (T + 1), writes 16 bytes per row, and inverts besides
  trace_t{T}          the whole interaction-trace build (mle_eval.mle_eval_interaction_trace: tstwo_gkr_gen_eq_evals,
                      tstwo_mle_eval_terms, tstwo_logup_finalize_last and its 16-byte read-back); bytes: 16 written by the eq
                      table, the terms call's, 48 moved by the prefix sum
  selectors           tstwo_mle_eval_selectors: writes 4 (2 log + 2) bytes per row, reads nothing
The HBM bound is the bytes at the measured copy rate of 6.3 TB/s.  Appends one JSON line per entry to --out.

    python tools/bench_mle_eval_air.py [--logs 20,24] [--terms 1,4] [--reps 10] [--out profiles/mle_eval_air.jsonl]
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
from tstwo_amd import logup as LG                                 # noqa: E402
from tstwo_amd import mle_eval as ME                              # noqa: E402
from tstwo_amd.backend import HipColumn, SecureColumnByCoords     # noqa: E402
from tstwo_amd.fields import P, QM31                              # noqa: E402
from tstwo_amd.gkr import HipGkrOps, Mle                          # noqa: E402

HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)
WARMUPS = 2


def time_ms(fn, reps):
    for _ in range(WARMUPS):
        fn()
    L.sync()
    ts = []
    for _ in range(reps):
        e0, e1 = L.Event(), L.Event()
        e0.record()
        fn()
        e1.record()
        ts.append(e0.elapsed_ms(e1))
    return statistics.median(ts), min(ts), max(ts)


def entry(name, log, timing, b):
    ms, lo, hi = timing
    return {"entry": name, "log": log, "ms": ms, "min_ms": lo, "max_ms": hi, "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3,
            "achieved_tb_s": b / ms / 1e9, "frac_hbm": b / HBM_COPY * 1e3 / ms}


def felt(rng):
    return QM31.from_u32_unchecked(*[int(v) for v in rng.integers(1, P, size=4)])


def run(log, terms, reps, rng):
    n = 1 << log
    out = []
    cols = [HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(max(terms))]
    num = HipColumn(rng.integers(0, P, size=n, dtype=np.uint32))
    point = [felt(rng) for _ in range(log)]
    eq = HipGkrOps.genEqEvals(point, QM31.one())
    dst = SecureColumnByCoords.uninitialized(n)
    for t in terms:
        form = LG.LinearForm([(felt(rng), c) for c in cols[:t]], felt(rng))
        out.append(entry(f"terms_t{t}", log, time_ms(lambda: ME.mle_eval_terms(eq, form, dst), reps), (32 + 4 * t) * n))
        out.append(entry(f"logup_column_t{t}", log, time_ms(lambda: LG.logup_column([(num, form)], None, log, dst), reps), (4 * (t + 1) + 16) * n))
        L.call("tstwo_check_zero_flag")
        claim = Mle(ME.mle_eval_terms(eq, form, SecureColumnByCoords.uninitialized(n)))
        total = LG.logup_finalize_last(claim.col, log)
        claim.free()
        out.append(entry(f"trace_t{t}", log, time_ms(lambda: ME.mle_eval_interaction_trace(point, total, form), reps), (16 + 32 + 4 * t + 48) * n))
    sel = [HipColumn.uninitialized(n) for _ in range(ME.n_selector_columns(log))]
    tab = L.ptr_array([c.ptr for c in sel])
    out.append(entry("selectors", log, time_ms(lambda: L.call("tstwo_mle_eval_selectors", log, tab), reps), 4 * len(sel) * n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,24")
    ap.add_argument("--terms", default="1,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_eval_air.jsonl"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps: at least 10")
    L.init(0)
    rng = np.random.default_rng(0)
    device = L.device_name()
    lines = []
    for lg in (int(x) for x in a.logs.split(",") if x):
        for e in run(lg, [int(x) for x in a.terms.split(",") if x], a.reps, rng):
            e.update(device=device, reps=a.reps, warmups=WARMUPS)
            lines.append(json.dumps(e))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Out-of-domain sampling at k points on one MI355X: k calls of tstwo_eval_at_point_batch (version A: what prove_values did for a
column opened at k points) against one call of tstwo_eval_at_points (version B), run alternately in one process on the same
columns.  Shapes 1 x 2^22, 32 x 2^20, 256 x 2^16 and 256 x 2^22 coefficients, k = 1..4.  Both calls are synchronous, so the
clock is the host's around the call; per (shape, k) one JSON line with the median, the quartiles, min and max of both versions,
the algorithmic bytes (A reads every coefficient k times, B once per sweep) and the verdict: B beats A when the medians differ
by more than the spread, which is the larger of the two interquartile ranges of that run.

    python tools/bench_eval_points.py [--shapes 1x22,32x20,256x16,256x22] [--reps 30] [--warmup 5] [--out profiles/bench_eval_points.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_points_plan as EP  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402

P = 2147483647
HBM = 8e12


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    us = lambda v: round(v * 1e6, 2)
    return {"median_us": us(statistics.median(xs)), "p25_us": us(q[0]), "p75_us": us(q[2]), "min_us": us(min(xs)), "max_us": us(max(xs)),
            "iqr_us": us(q[2] - q[0])}


def bench(cols, log, k, reps, warmup, buf, rng):
    n = 1 << log
    ptrs = L.ptr_array([buf.ptr + 4 * n * i for i in range(cols)])
    pts = [[int(w) for w in rng.integers(0, P, size=8)] for _ in range(k)]
    out_a = [(C.c_uint32 * (4 * cols))() for _ in range(k)]
    out_b = (C.c_uint32 * (4 * cols * k))()
    xs, ys = [L.u32x(p[:4]) for p in pts], [L.u32x(p[4:]) for p in pts]
    g_cols, g_logs, g_pts, words = L.u32x([cols]), L.u32x([log]), L.u32x([k]), L.u32x([w for p in pts for w in p])

    def version_a():
        for j in range(k):
            L.call("tstwo_eval_at_point_batch", ptrs, cols, log, xs[j], ys[j], out_a[j])

    def version_b():
        L.call("tstwo_eval_at_points", ptrs, g_cols, g_logs, g_pts, 1, words, out_b)

    version_a(); version_b()
    for i in range(cols):
        for j in range(k):
            assert list(out_a[j][4 * i:4 * i + 4]) == list(out_b[4 * (i * k + j):4 * (i * k + j) + 4]), "the two versions disagree"
    for _ in range(warmup):
        version_a(); version_b()
    ta, tb = [], []
    for _ in range(reps):                          # alternate, so that both see the same clocks and the same neighbours
        t0 = time.perf_counter(); version_a(); t1 = time.perf_counter(); version_b(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    a, b = quartiles(ta), quartiles(tb)
    spread = max(a["iqr_us"], b["iqr_us"])
    p = EP.plan(log, cols, k, True)
    bytes_a, bytes_b = 4 * n * cols * k, 4 * n * cols * p.sweeps
    return {"tool": "bench_eval_points", "cols": cols, "log": log, "points": k, "reps": reps, "warmup": warmup, "plan": EP.render(p),
            "A_batch_calls": a, "B_one_call": b, "spread_us": spread, "A_minus_B_us": round(a["median_us"] - b["median_us"], 2),
            "B_beats_A_by_more_than_spread": a["median_us"] - b["median_us"] > spread,
            "B_within_spread_of_A": abs(a["median_us"] - b["median_us"]) <= spread,
            "bytes_A": bytes_a, "bytes_B": bytes_b, "GBps_A": round(bytes_a / (a["median_us"] * 1e-6) / 1e9, 1),
            "GBps_B": round(bytes_b / (b["median_us"] * 1e-6) / 1e9, 1), "frac_8TBps_B": round(bytes_b / (b["median_us"] * 1e-6) / HBM, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x22,32x20,256x16,256x22")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file (profiles/bench_eval_points.jsonl)")
    a = ap.parse_args()
    L.init(0)
    device = L.device_name()
    lines = []
    for shape in a.shapes.split(","):
        cols, log = (int(v) for v in shape.split("x"))
        n = 1 << log
        rng = np.random.default_rng(1000 * log + cols)
        buf = L.DeviceBuffer(4 * n * cols)
        buf.upload(rng.integers(0, P, size=n, dtype=np.uint32))            # column 0 from the host, the others device copies of it
        for i in range(1, cols):
            L.call("tstwo_copy", C.c_void_p(buf.ptr + 4 * n * i), C.c_void_p(buf.ptr), 4 * n)
        L.sync()
        for k in (1, 2, 3, 4):
            rec = bench(cols, log, k, a.reps, a.warmup, buf, rng)
            rec["device"] = device
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        buf.free()
        L.call("tstwo_trim")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

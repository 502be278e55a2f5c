#!/usr/bin/env python3
"""Lookup multiplicities on one MI355X (csrc/lookup.hip) against the host path they replace.

Per case (log_range in 8, 14, 16, 20 x two columns of 2^16, 2^20, 2^22 uniformly random values, and two columns of 2^22 equal
values per log_range: the worst case for the atomics), two paths, timed in turn (device, host, device, host, ...), the median
of --reps after a warm-up of each:
  device   logup.lookup_multiplicities(check=False) on columns that are in device memory: HIP events around the call, and wall
           time ended by a device synchronisation
  host     what a prover did before: download every value column, constraint_framework.range_check_multiplicities (np.bincount
           and the permutation into coset order on one core), upload the counts; wall time ended by a device synchronisation
Algorithmic bytes of the device path: every value read once (4 bytes) and the table zeroed and added to (8 bytes per bin); the
HBM bound is those bytes at 6.3 TB/s.  Prints one JSON line per case and writes them to --out.

    python tools/bench_lookup.py [--reps 10] [--out profiles/bench_lookup.jsonl]
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
from tstwo_amd.backend import HipColumn                           # noqa: E402

HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)
LOG_RANGES = (8, 14, 16, 20)
LOG_VALUES = (16, 20, 22)
N_COLS = 2


def device_path(log_range, cols):
    return LG.lookup_multiplicities(log_range, *cols, check=False)


def host_path(log_range, cols):
    return HipColumn(F.range_check_multiplicities(log_range, *[c.to_numpy() for c in cols]))


def timed(fn):
    """(HIP-event ms, wall ms ended by a synchronisation, the result) of one call."""
    L.sync()
    e0, e1 = L.Event(), L.Event()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    L.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return e0.elapsed_ms(e1), wall, r


def case(log_range, log_values, kind, reps, rng):
    n = 1 << log_values
    if kind == "uniform":
        cols = [HipColumn(rng.integers(0, 1 << log_range, size=n, dtype=np.uint32)) for _ in range(N_COLS)]
    else:
        cols = [HipColumn(np.full(n, (1 << log_range) - 1, dtype=np.uint32)) for _ in range(N_COLS)]
    paths = {"device": lambda: device_path(log_range, cols), "host": lambda: host_path(log_range, cols)}
    results = {name: timed(fn)[2].to_numpy() for name, fn in paths.items()}             # the warm-up, and the two must agree
    assert np.array_equal(results["device"], results["host"])
    ev, wall = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            e, w, _ = timed(fn)
            ev[name].append(e)
            wall[name].append(w)
    b = 4 * N_COLS * n + 8 * (1 << log_range)
    dev_ev, dev_wall, host_wall = (statistics.median(x) for x in (ev["device"], wall["device"], wall["host"]))
    return {"log_range": log_range, "log_values": log_values, "n_cols": N_COLS, "values": kind, "reps": reps,
            "device_event_ms": dev_ev, "device_wall_ms": dev_wall, "host_event_ms": statistics.median(ev["host"]), "host_wall_ms": host_wall,
            "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3, "achieved_tb_s": b / dev_ev / 1e9, "host_over_device_wall": host_wall / dev_wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lookup.jsonl"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps: at least 10")
    L.init(0)
    rng = np.random.default_rng(0)
    lines = [json.dumps({"device": L.device_name(), "hbm_tb_s": HBM_COPY / 1e12})]
    print(lines[0], flush=True)
    for log_range in LOG_RANGES:
        for log_values, kind in [(lv, "uniform") for lv in LOG_VALUES] + [(22, "all-equal")]:
            lines.append(json.dumps(case(log_range, log_values, kind, a.reps, rng)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

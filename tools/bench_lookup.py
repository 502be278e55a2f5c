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

--keyed PARENT_LIB measures tstwo_lookup_multiplicities_keyed instead (lines to profiles/bench_lookup_keyed.jsonl).  PARENT_LIB is
the library of the commit before, built from its own tree: it is loaded beside the current one (its own context and stream on
the same device; the columns are shared, every timed call is bracketed by a synchronisation of both) so that both are measured
in one process on one box.  Per table of 2^8, 2^14, 2^16, 2^20 bins and per key distribution (uniform; all rows one key; half
the rows one key, the rest uniform), 2 groups x 2^22 rows, the paths of a variant in turn (their order drawn anew for every round, fixed seed), median and min-max of --reps:
  1limb    one limb, no weights: the keyed entry | the parent's tstwo_lookup_multiplicities | the current library's
           tstwo_lookup_multiplicities (it was not touched: it must not have moved) | the host path above
  2limbs   two limbs, no weights: the keyed entry | the parent's pack-then-count (tstwo_air_eval_columns a + 2^bits b, then
           tstwo_lookup_multiplicities on the packed columns)
  weights  one limb and a 0/1 weight column: the keyed entry | the host path (download, np.bincount(weights=), upload)
and, with --old-table, the rows of the table above for the old entry in both libraries.
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


# ------------------------------------------------------------------ --keyed
KEYED_LOGS = (8, 14, 16, 20)
KEYED_ROWS = 1 << 22
KINDS = ("uniform", "all-equal", "half-equal")


class Parent:
    """The library of the commit before, loaded beside the current one: the prototypes it shares with it, its own events."""

    def __init__(self, path):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        for name in ("tstwo_init", "tstwo_sync", "tstwo_event_create", "tstwo_event_record", "tstwo_event_elapsed_ms",
                     "tstwo_lookup_multiplicities", "tstwo_air_eval_columns"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = C.c_int, L._SIGS[name]
        self.lib.tstwo_last_error.restype = C.c_char_p
        self.call("tstwo_init", 0)

    def call(self, name, *args):
        if getattr(self.lib, name)(*args):
            raise RuntimeError(f"parent {name}: {self.lib.tstwo_last_error().decode()}")

    def event(self):
        e = self.C.c_void_p()
        self.call("tstwo_event_create", self.C.byref(e))
        return e

    def lookup(self, log_range, cols, out):
        C = self.C
        self.call("tstwo_lookup_multiplicities", L.ptr_array([c.ptr for c in cols]), (C.c_size_t * len(cols))(*[c.len() for c in cols]),
                  len(cols), log_range, 1, out.ptr, None)
        return out


def timed_on(parent, fn):
    """timed() for a path that runs on the parent library's stream."""
    C = parent.C
    L.sync()
    parent.call("tstwo_sync")
    e0, e1 = parent.event(), parent.event()
    t0 = time.perf_counter()
    parent.call("tstwo_event_record", e0)
    r = fn()
    parent.call("tstwo_event_record", e1)
    parent.call("tstwo_sync")
    wall = (time.perf_counter() - t0) * 1e3
    ms = C.c_float(0)
    parent.call("tstwo_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value, wall, r


def keys(kind, log_range, rng):
    n = 1 << log_range
    v = rng.integers(0, n, size=KEYED_ROWS, dtype=np.uint32)
    if kind == "all-equal":
        v[:] = n - 1
    elif kind == "half-equal":
        v[rng.permutation(KEYED_ROWS)[:KEYED_ROWS // 2]] = n - 1
    return v


def stats(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples)}


def run_paths(paths, reps, same=True):
    """paths: {name: (fn, parent or None)}.  A warm-up of each (their results must agree), then reps rounds, the paths in turn."""
    def one(fn, parent):
        return timed_on(parent, fn) if parent is not None else timed(fn)
    first = {name: one(fn, parent)[2].to_numpy() for name, (fn, parent) in paths.items()}
    ref = next(iter(first.values()))
    assert not same or all(np.array_equal(ref, r) for r in first.values()), "the paths disagree"
    ev, wall = {k: [] for k in paths}, {k: [] for k in paths}
    # The order of the paths is drawn anew for every round (a fixed seed): the path that runs right after a host path finds a GPU
    # that has idled for tens of milliseconds and takes 35 to 70 us longer for it, whichever path it is, and with a fixed or merely rotated
    # order that is always the same one.  after_host / after_device split a path's samples by what ran before it.
    import random
    order_rng = random.Random(len(paths))
    names, prev = list(paths), None
    split = {k: {"after_host": [], "after_device": []} for k in paths}
    for rep in range(reps):
        order = names[:]
        order_rng.shuffle(order)
        for name in order:
            fn, parent = paths[name]
            e, w, _ = one(fn, parent)
            ev[name].append(e)
            wall[name].append(w)
            if prev is not None:
                split[name]["after_host" if prev.startswith("host") else "after_device"].append(e)
            prev = name
    med = lambda x: statistics.median(x) if x else None
    return {name: {"events": stats(ev[name]), "wall": stats(wall[name]), "events_after_host_median_ms": med(split[name]["after_host"]),
                   "events_after_device_median_ms": med(split[name]["after_device"])} for name in paths}


def keyed_case(parent, log_range, kind, reps, rng):
    from tstwo_amd.constraint_framework import Expr, compile_columns
    C = parent.C
    vals = [keys(kind, log_range, rng) for _ in range(N_COLS)]
    cols = [HipColumn(v) for v in vals]
    lo = log_range // 2
    a = [HipColumn(v & ((1 << lo) - 1)) for v in vals]
    b = [HipColumn(v >> lo) for v in vals]
    wts = [rng.integers(0, 2, size=KEYED_ROWS, dtype=np.uint32) for _ in range(N_COLS)]
    wcols = [HipColumn(w) for w in wts]
    program = compile_columns([Expr.load(("main", 0), 0) + Expr.load(("main", 1), 0) * (1 << lo)], 2)
    words = L.u32x(program.words)

    def pack_then_count():
        packed = []
        for x, y in zip(a, b):
            out = HipColumn.uninitialized(KEYED_ROWS)
            parent.call("tstwo_air_eval_columns", L.ptr_array([x.ptr, y.ptr]), 2, 22, words, program.n_instr, L.ptr_array([out.ptr]), 1)
            packed.append(out)
        return parent.lookup(log_range, packed, HipColumn.uninitialized(1 << log_range))

    def host_weighted():
        # a timing reference for the 0/1 weights of this benchmark only: float64 sums without the reduction mod P are not the
        # entry's semantics for general weights (tests/lookup_keyed_model.py is the reference for those)
        counts = np.zeros(1 << log_range, dtype=np.float64)
        for c, w in zip(cols, wcols):
            counts += np.bincount(c.to_numpy(), weights=w.to_numpy(), minlength=1 << log_range)
        m = np.empty(1 << log_range, dtype=np.uint32)
        m[F._coset_positions(log_range)] = counts.astype(np.uint32)
        return HipColumn(m)

    g1 = [LG.LookupGroup([(c, log_range)]) for c in cols]
    g2 = [LG.LookupGroup([(x, lo), (y, log_range - lo)]) for x, y in zip(a, b)]
    gw = [LG.LookupGroup([(c, log_range)], weight=w) for c, w in zip(cols, wcols)]
    variants = {
        "1limb": {"keyed": (lambda: LG.lookup_multiplicities_keyed(g1, check=False), None),
                  "parent_old": (lambda: parent.lookup(log_range, cols, HipColumn.uninitialized(1 << log_range)), parent),
                  "old": (lambda: device_path(log_range, cols), None),
                  "host": (lambda: host_path(log_range, cols), None)},
        "2limbs": {"keyed": (lambda: LG.lookup_multiplicities_keyed(g2, check=False), None),
                   "parent_pack_then_count": (pack_then_count, parent)},
        "weights": {"keyed": (lambda: LG.lookup_multiplicities_keyed(gw, check=False), None),
                    "host": (host_weighted, None)},
    }
    return [{"mode": "keyed", "variant": name, "log_range": log_range, "rows_per_group": KEYED_ROWS, "groups": N_COLS, "keys": kind, "reps": reps,
             "paths": run_paths(paths, reps)} for name, paths in variants.items()]


def old_table_case(parent, log_range, log_values, kind, reps, rng):
    n = 1 << log_values
    if kind == "uniform":
        cols = [HipColumn(rng.integers(0, 1 << log_range, size=n, dtype=np.uint32)) for _ in range(N_COLS)]
    else:
        cols = [HipColumn(np.full(n, (1 << log_range) - 1, dtype=np.uint32)) for _ in range(N_COLS)]
    paths = {"old": (lambda: device_path(log_range, cols), None),
             "parent_old": (lambda: parent.lookup(log_range, cols, HipColumn.uninitialized(1 << log_range)), parent)}
    return {"mode": "old-table", "log_range": log_range, "log_values": log_values, "n_cols": N_COLS, "values": kind, "reps": reps,
            "paths": run_paths(paths, reps)}


def keyed_main(a):
    L.init(0)
    parent = Parent(a.keyed)
    rng = np.random.default_rng(0)
    lines = [json.dumps({"device": L.device_name(), "parent": os.path.basename(os.path.dirname(a.keyed)) or a.keyed, "label": a.label})]
    print(lines[0], flush=True)
    for log_range in a.logs or KEYED_LOGS:
        for kind in KINDS:
            for rec in keyed_case(parent, log_range, kind, a.reps, rng):
                rec["label"] = a.label
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if a.old_table:
        for log_range in LOG_RANGES:
            for log_values, kind in [(lv, "uniform") for lv in LOG_VALUES] + [(22, "all-equal")]:
                lines.append(json.dumps(old_table_case(parent, log_range, log_values, kind, a.reps, rng)))
                print(lines[-1], flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "bench_lookup_keyed.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyed", metavar="PARENT_LIB", help="measure the keyed entry against this library of the commit before")
    ap.add_argument("--old-table", action="store_true", help="with --keyed: the old entry at every row of the table, in both libraries")
    ap.add_argument("--logs", type=int, nargs="*", help="with --keyed: these table sizes only")
    ap.add_argument("--label", default="", help="with --keyed: a name for the library under test in every line")
    ap.add_argument("--append", action="store_true", help="with --keyed: add to --out")
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps: at least 10")
    if a.keyed:
        return keyed_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "bench_lookup.jsonl")
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

#!/usr/bin/env python3
"""Mle.evalAtPoint on one MI355X: the one-pass call (tstwo_mle_eval_at_point_base / _secure) against the only path the library
offered before it — log_n successive fixFirstVariable calls and the read of the last value — run alternately in one process on
the same columns.  Per case (2^16, 2^20, 2^24 values; base and secure; 1 and 8 MLEs): HIP-event time and wall time ended by the
read-back, median of --reps after --warmup with min and max; algorithmic bytes (4 per base value, 16 per secure one) over the
event time against 8 TB/s; and the VALU bound of pass 1 (VALU instructions of the straight-line kernel per lane, from the ISA,
over the values a lane owns, at the one-port integer peak of DESIGN §4).  The same tool times tstwo_gkr_logup_denominators at 1,
4 and 16 terms.  Prints one JSON line.

    python tools/bench_mle_eval.py [--sizes 16,20,24] [--reps 20] [--warmup 3] [--out profiles/bench_mle_eval.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mle_eval_plan as MP  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import gkr as G  # noqa: E402
from tstwo_amd.backend import HipColumn, SecureColumnByCoords  # noqa: E402
from tstwo_amd.fields import P, QM31  # noqa: E402

HBM = 8e12
VALU_ONE_PORT = 35.3e12          # integer lane-ops/s, one issue port
FIRST = {("base", 1): "k_mle_firstILb0ELb1ELi1E", ("base", 4): "k_mle_firstILb0ELb1ELi4E", ("secure", 4): "k_mle_firstILb1ELb1ELi4E"}


def kernel_valu_counts():
    """VALU instructions of each fast pass-1 kernel (straight-line code: every lane issues each of them once)."""
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "mle_eval.s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                               os.path.join(ROOT, "tstwo_amd", "csrc", "mle_eval.hip"), "-o", s], stderr=subprocess.DEVNULL)
        asm = open(s).read()
    out = {}
    for key, sym in FIRST.items():
        m = re.search(r"^(\S*" + re.escape(sym) + r"\S*):", asm, flags=re.M)
        body = asm[m.end():asm.index("s_endpgm", m.end())]
        out[key] = sum(1 for line in body.split("\n") if line.split(";")[0].strip().startswith("v_"))
    return out


def rand_felt(rng):
    return QM31.from_u32_unchecked(*[int(x) for x in rng.integers(0, P, size=4)])


def distinct_columns(seed_col: HipColumn, count: int):
    """`count` columns at their own addresses with the seed column's words (device copies: no host generation per column)."""
    cols = []
    for _ in range(count):
        c = HipColumn.uninitialized(seed_col.len())
        L.call("tstwo_copy", C.c_void_p(c.ptr), C.c_void_p(seed_col.ptr), 4 * seed_col.len())
        cols.append(c)
    return cols


def timed(fn, reps, warmup):
    """(event seconds, wall seconds) per repetition; fn ends with its own read-back."""
    for _ in range(warmup):
        fn()
    L.sync()
    ev, wall = [], []
    for _ in range(reps):
        a, b = L.Event(), L.Event()
        t0 = time.perf_counter()
        a.record()
        fn()
        wall.append(time.perf_counter() - t0)
        b.record()
        L.sync()
        ev.append(a.elapsed_ms(b) * 1e-3)
    return ev, wall


def stats(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 2), "min_us": round(min(xs) * 1e6, 2), "max_us": round(max(xs) * 1e6, 2)}


def bench_eval(n, secure, n_mles, reps, warmup, valu, seed_col):
    rng = np.random.default_rng(100 * n + n_mles)
    N = 1 << n
    point = [rand_felt(rng) for _ in range(n)]
    if secure:
        mles = [G.Mle(SecureColumnByCoords(distinct_columns(seed_col, 4))) for _ in range(n_mles)]
    else:
        mles = [G.Mle(c) for c in distinct_columns(seed_col, n_mles)]
    folded = [G.Mle.uninitialized_secure(N // 2) for _ in range(n_mles)]

    def one_pass():
        return G.eval_mles_at_point(mles, point)

    def fold_chain():
        for m, out in zip(mles, folded):
            G.HipMleOps.fix_first_variable_into(m, point[0], out)
            for k in range(1, n):
                cur = G._shrink(out, n - k)
                G.HipMleOps.fix_first_variable_into(cur, point[k], cur)
        words = L.download_many([(p, 1) for out in folded for p in out.ptr_list()])
        return [G._qs([int(w[0]) for w in words[4 * i:4 * i + 4]]) for i in range(n_mles)]

    assert [v.tup() for v in one_pass()] == [v.tup() for v in fold_chain()], "the two paths disagree"
    # alternate: one repetition of each in turn, so that both see the same clocks and the same neighbours
    new_ev, new_wall, old_ev, old_wall = [], [], [], []
    for fn in (one_pass, fold_chain):
        for _ in range(warmup):
            fn()
    for _ in range(reps):
        e, w = timed(one_pass, 1, 0)
        new_ev += e
        new_wall += w
        e, w = timed(fold_chain, 1, 0)
        old_ev += e
        old_wall += w
    nbytes = (16 if secure else 4) * N * n_mles
    p = MP.plan(n, n_mles, secure, True)
    per_lane = 16 * (1 if secure else p.groups)                       # values a lane of pass 1 owns
    v = valu[("secure" if secure else "base", p.groups)]
    bound = N * n_mles / per_lane * v / VALU_ONE_PORT
    t = statistics.median(new_ev)
    rec = {"log_n": n, "kind": "secure" if secure else "base", "n_mles": n_mles, "plan": MP.render(p),
           "one_pass_event": stats(new_ev), "one_pass_wall": stats(new_wall), "fold_chain_event": stats(old_ev), "fold_chain_wall": stats(old_wall),
           "bytes": nbytes, "GBps": round(nbytes / t / 1e9, 1), "frac_8TBps": round(nbytes / t / HBM, 3),
           "hbm_bound_us": round(nbytes / HBM * 1e6, 2), "valu_per_lane": v, "valu_bound_us": round(bound * 1e6, 2),
           "slowest_one_pass_beats_fastest_chain": max(new_wall) < min(old_wall)}
    for m in mles + folded:
        m.free()
    return rec


def bench_denominators(n, n_terms, reps, warmup, seed_col):
    rng = np.random.default_rng(7 * n + n_terms)
    N = 1 << n
    cols = distinct_columns(seed_col, n_terms)
    out = G.Mle.uninitialized_secure(N)
    ptrs = L.ptr_array([c.ptr for c in cols])
    coeffs = L.u32x([int(x) for x in rng.integers(0, P, size=4 * n_terms)])
    const = L.u32x([int(x) for x in rng.integers(0, P, size=4)])

    def run():
        L.call("tstwo_gkr_logup_denominators", ptrs, coeffs, n_terms, const, n, out.ptrs())
        L.sync()

    ev, _ = timed(run, reps, warmup)
    nbytes = (4 * n_terms + 16) * N
    t = statistics.median(ev)
    out.free()
    return {"log_n": n, "n_terms": n_terms, "event": stats(ev), "bytes": nbytes, "GBps": round(nbytes / t / 1e9, 1),
            "frac_8TBps": round(nbytes / t / HBM, 3), "hbm_bound_us": round(nbytes / HBM * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file (profiles/bench_mle_eval.json)")
    a = ap.parse_args()
    L.init(0)
    valu = kernel_valu_counts()
    res = {"tool": "bench_mle_eval", "device": L.device_name(), "reps": a.reps, "warmup": a.warmup, "valu_one_port_lane_ops": VALU_ONE_PORT,
           "eval_at_point": [], "logup_denominators": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        seed_col = HipColumn(np.random.default_rng(n).integers(0, P, size=1 << n, dtype=np.uint32))
        for secure in (False, True):
            for n_mles in (1, 8):
                res["eval_at_point"].append(bench_eval(n, secure, n_mles, a.reps, a.warmup, valu, seed_col))
                L.call("tstwo_trim")
        for n_terms in (1, 4, 16):
            res["logup_denominators"].append(bench_denominators(n, n_terms, a.reps, a.warmup, seed_col))
            L.call("tstwo_trim")
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

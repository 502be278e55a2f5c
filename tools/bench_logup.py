#!/usr/bin/env python3
"""The LogUp interaction trace on one MI355X (csrc/logup.hip), and the phases of a range-check proof.

Kernels, per log size (16, 18, 20, 22, 24 by default), timed with HIP events (median of --reps launches after a warm-up):
  column_f{F}_t{T}   tstwo_logup_column with F fractions (1, 2) of T terms (1, 2, 4) each, column numerators, a previous column
  finalize_last      tstwo_logup_finalize_last on one QM31 column (its 3 launches and the 16-byte read-back)
Algorithmic bytes: a column reads F (T + 1) M31 columns and the 4 words of prev and writes 4 words per row; finalize_last moves
12 bytes per M31 word (two reads and one write), 48 per row.  The HBM bound is those bytes at 6.3 TB/s.
Range-check prove phases (log 16 .. 20, the values component at log + 1): interaction generation (both components), its commit,
the composition polynomial (alpha to the composition tree root), prove_values; wall time ended by a device synchronisation.
Prints one JSON line and writes it to --out.

    python tools/bench_logup.py [--logs 16,18,20,22,24] [--prove-logs 16,18,20] [--reps 10] [--out profiles/r11_bench_logup.json]
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
from tstwo_amd import air as A                                    # noqa: E402
from tstwo_amd import constraint_framework as F                   # noqa: E402
from tstwo_amd import logup as LG                                 # noqa: E402
from tstwo_amd.backend import HipColumn, SecureColumnByCoords     # noqa: E402
from tstwo_amd.channel import Blake2sChannel                      # noqa: E402
from tstwo_amd.circle import CanonicCoset                         # noqa: E402
from tstwo_amd.fields import P, QM31                              # noqa: E402
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig       # noqa: E402
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles  # noqa: E402
from tstwo_amd.air import ComponentProvers, Trace                 # noqa: E402

HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)


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


def entry(ms, b):
    return {"ms": ms, "bytes": b, "hbm_bound_ms": b / HBM_COPY * 1e3, "achieved_tb_s": b / ms / 1e9, "frac_hbm": b / HBM_COPY * 1e3 / ms}


def felt(rng):
    return QM31.from_u32_unchecked(*[int(v) for v in rng.integers(0, P, size=4)])


def kernels(log, reps, rng):
    n = 1 << log
    res = {"log": log}
    cols = [HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(9)]
    le = LG.LookupElements(felt(rng), felt(rng), 4)
    prev = SecureColumnByCoords([HipColumn(rng.integers(0, P, size=n, dtype=np.uint32)) for _ in range(4)])
    out = SecureColumnByCoords.uninitialized(n)
    for f in (1, 2):
        for t in (1, 2, 4):
            fracs = [(cols[8 - b], le.combine_columns(cols[4 * b:4 * b + t])) for b in range(f)]
            ms = time_ms(lambda: LG.logup_column(fracs, prev, log, out), reps)
            res[f"column_f{f}_t{t}"] = entry(ms, (f * (t + 1) + 8) * 4 * n)
    ms = time_ms(lambda: LG.logup_finalize_last(out, log), reps)
    res["finalize_last"] = entry(ms, 48 * n)
    return res


def sync_ms(fn):
    L.sync()
    t0 = time.perf_counter()
    r = fn()
    L.sync()
    return (time.perf_counter() - t0) * 1e3, r


def prove_phases(log, rng):
    """Range check over [0, 2^log) with a values component of 2^(log + 1) rows (two checked columns)."""
    lv = log + 1
    v0, v1 = (rng.integers(0, 1 << log, size=1 << lv) for _ in range(2))
    mult = F.range_check_multiplicities(log, v0, v1)
    tw = precompute_twiddles(CanonicCoset(lv + 3).circleDomain().halfCoset)
    ch = Blake2sChannel()
    config = PcsConfig()
    scheme = CommitmentSchemeProver(config, tw)

    def commit(evs):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(ch)

    dom = lambda lg: CanonicCoset(lg).circleDomain()                                      # noqa: E731
    commit([HipCircleEvaluation(dom(log), HipColumn(F.range_check_table_column(log)))])
    commit([HipCircleEvaluation(dom(log), HipColumn(mult))] + [HipCircleEvaluation(dom(lv), HipColumn(v.astype(np.uint32))) for v in (v0, v1)])
    le = LG.LookupElements.draw(ch, 1)
    # the device columns the generators read, uploaded before the timed phase
    dv0, dv1 = HipColumn(v0.astype(np.uint32)), HipColumn(v1.astype(np.uint32))
    dval = HipColumn(F.range_check_table_column(log))
    dneg = HipColumn(((P - mult.astype(np.uint64)) % P).astype(np.uint32))

    def generate():
        t = LG.LogupTraceGenerator(log)
        c = t.new_col()
        c.write_frac(dneg, le.combine_columns([dval]))
        c.finalize_col()
        v = LG.LogupTraceGenerator(lv)
        c = v.new_col()
        c.write_frac(1, le.combine_columns([dv0]))
        c.write_frac(1, le.combine_columns([dv1]))
        c.finalize_col()
        return t.finalize_last(), v.finalize_last()
    res = {"log": log}
    res["interaction_gen_ms"], ((t_ev, t_sum), (v_ev, v_sum)) = sync_ms(generate)
    ch.mix_felts([t_sum, v_sum])
    res["interaction_commit_ms"], _ = sync_ms(lambda: commit(t_ev + v_ev))
    alloc = A.TraceLocationAllocator()
    comps = [F.FrameworkComponent(F.RangeCheckTableEval(log, le), alloc, [0], claimed_sum=t_sum),
             F.FrameworkComponent(F.RangeCheckValuesEval(lv, le), alloc, claimed_sum=v_sum)]
    provers = ComponentProvers(comps, 1)
    alpha = ch.draw_felt()

    def composition():
        poly = provers.compute_composition_polynomial(alpha, Trace.of(scheme), tw)
        tb = scheme.tree_builder()
        tb.extend_polys(poly.into_coordinate_polys())
        tb.commit(ch)
    res["composition_ms"], _ = sync_ms(composition)
    from tstwo_amd.circle import CirclePoint
    from tstwo_amd.prover import _sample_points
    oods = CirclePoint.get_random_point(ch)
    res["prove_values_ms"], _ = sync_ms(lambda: scheme.prove_values(_sample_points(provers.components(), oods), ch))
    res["claimed_sum_total_zero"] = t_sum.add(v_sum) == QM31.zero()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20,22,24")
    ap.add_argument("--prove-logs", default="16,18,20")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_bench_logup.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps: at least 10")
    L.init(0)
    rng = np.random.default_rng(0)
    out = {"device": L.device_name(), "reps": a.reps, "hbm_tb_s": HBM_COPY / 1e12,
           "kernels": [kernels(lg, a.reps, rng) for lg in (int(x) for x in a.logs.split(",") if x)],
           "prove_phases": [prove_phases(lg, rng) for lg in (int(x) for x in a.prove_logs.split(",") if x)]}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

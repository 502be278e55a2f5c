#!/usr/bin/env python3
"""AIR proving on one MI355X: wide Fibonacci with N = 100 columns at log 16, 18 and 20 (22 with --log22), every proof verified.

Phases (milliseconds, each ended by a device synchronisation): trace generation, trace commit (the empty preprocessed tree and the
trace tree), the constraint kernel, finalize (the composition polynomial from the accumulation), the composition commit and
prove_values.  prove_total is one whole prove() call on the same committed trace (from drawing alpha to the proof); host_share is
prove_total minus the four device phases of the piecewise run.  The constraint kernel is also timed alone with HIP events (median
of --reps) and set against two bounds:
  HBM   algorithmic bytes (N + 8) * 4 * 2^(log + 1) — the trace read plus the accumulator read-modify-write — at 6.3 TB/s
  VALU  VALU instructions per row counted from the ISA (the constraint loop and the per-row remainder) times the rows at the one-port
        35.3e12 lane-ops/s of DESIGN §4
Prints one JSON line.

    python tools/bench_prove.py [--logs 16,18,20] [--log22] [--reps 10]
"""
from __future__ import annotations

import argparse
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

from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import air as A  # noqa: E402
from tstwo_amd import constraint_framework as F  # noqa: E402
from tstwo_amd.backend import HipColumn, SecureColumnByCoords  # noqa: E402
from tstwo_amd.channel import Blake2sChannel  # noqa: E402
from tstwo_amd.circle import CanonicCoset, CirclePoint  # noqa: E402
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig  # noqa: E402
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier  # noqa: E402
from tstwo_amd.poly import precompute_twiddles  # noqa: E402
from tstwo_amd.prover import StarkProof, prove, verify  # noqa: E402

VALU_ONE_PORT = 35.3e12          # integer lane-ops/s, one issue port
HBM_COPY = 6.3e12                # bytes/s, measured copy rate (MI355X_MICROARCH.md)
P = 2**31 - 1
N_COLS = 100
KERNEL = "k_constraint_quotientsILi0ELi4E"      # TSTWO_AIR_WIDE_FIB, 4 rows per lane


def _lines(asm: str, sym: str):
    m = re.search(r"^(\S*" + re.escape(sym) + r"\S*):", asm, flags=re.M)
    body = asm[m.end():asm.index("s_endpgm", m.end())].split("\n")
    labels, lines = {}, []
    for line in body:
        line = line.split(";")[0].strip()
        if not line or line.startswith("."):
            if re.match(r"^\.LBB\S+:", line):
                labels[line[:-1]] = len(lines)
            continue
        lines.append(line)
    return labels, lines


def isa_counts() -> dict:
    """The constraint loop is the innermost loop that loads columns (4 constraints x 4 rows per iteration); the grid-stride loop around
    it holds the per-row remainder (first two columns, reduction, denominator, accumulator update)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "air.s")
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                               os.path.join(ROOT, "tstwo_amd", "csrc", "air.hip"), "-o", out])
        asm = open(out).read()
    labels, lines = _lines(asm, KERNEL)
    loops = []
    for i, line in enumerate(lines):
        b = re.match(r"^s_cbranch_\w+\s+(\.LBB\S+)|^s_branch\s+(\.LBB\S+)", line)
        if b:
            tgt = b.group(1) or b.group(2)
            if tgt in labels and labels[tgt] <= i:
                loops.append((labels[tgt], i))
    valu = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_"))
    mad = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_mad_u64_u32"))
    inner = min((l for l in loops if any(x.startswith("global_load") for x in lines[l[0]:l[1] + 1])), key=lambda l: l[1] - l[0])
    outer = max(loops, key=lambda l: l[1] - l[0])
    loop_v, outer_v = valu(*inner), valu(*outer)
    n_groups = -(-(N_COLS - 2) // 4)
    per_lane = loop_v * n_groups + (outer_v - loop_v)
    return {"constraint_loop_valu_per_4_constraints_x_4_rows": loop_v, "constraint_loop_mad_u64_u32": mad(*inner),
            "per_row_remainder_valu": (outer_v - loop_v) / 4, "valu_per_row": per_lane / 4}


def sync_ms(fn):
    L.sync()
    t = time.perf_counter()
    r = fn()
    L.sync()
    return r, (time.perf_counter() - t) * 1e3


def commit_trace(log, trace, config):
    tw = precompute_twiddles(CanonicCoset(log + 1 + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    scheme, ch = CommitmentSchemeProver(config, tw), Blake2sChannel()
    for evs in ([], trace):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(ch)
    return scheme, ch


def verify_ms(comp, proof, config) -> float:
    t = time.perf_counter()
    v, ch = CommitmentSchemeVerifier(config), Blake2sChannel()
    sizes = A.Components([comp]).column_log_sizes()
    v.commit(proof.commitments[0], sizes[0], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    verify([comp], ch, v, proof)
    return (time.perf_counter() - t) * 1e3


def run(log, reps, isa) -> dict:
    rng = np.random.default_rng(log)
    a, b = HipColumn(rng.integers(0, P, size=1 << log, dtype=np.uint32)), HipColumn(rng.integers(0, P, size=1 << log, dtype=np.uint32))
    comp = F.WideFibonacciComponent(log, N_COLS)
    config = PcsConfig()
    res = {"log_n": log, "n_columns": N_COLS}
    trace, res["trace_gen_ms"] = sync_ms(lambda: A.generate_wide_fib_trace(log, a, b, N_COLS))
    (scheme, ch), res["trace_commit_ms"] = sync_ms(lambda: commit_trace(log, trace, config))
    # piecewise prove (the steps of prover.prove, each synchronised)
    alpha = ch.draw_felt()
    provers = A.ComponentProvers([comp])
    tr = A.Trace.of(scheme)
    acc = A.DomainEvaluationAccumulator.new(alpha, log + 1, comp.n_constraints)
    _, res["constraint_kernel_ms"] = sync_ms(lambda: comp.evaluate_constraint_quotients_on_domain(tr, acc, scheme.twiddles))
    poly, res["finalize_ms"] = sync_ms(lambda: acc.finalize(scheme.twiddles))

    def comp_commit():
        tb = scheme.tree_builder()
        tb.extend_polys(poly.into_coordinate_polys())
        tb.commit(ch)
    _, res["composition_commit_ms"] = sync_ms(comp_commit)
    oods = CirclePoint.get_random_point(ch)
    pts = provers.components().mask_points(oods) + [[[oods]] * 4]
    pproof, res["prove_values_ms"] = sync_ms(lambda: scheme.prove_values(pts, ch))
    # the same proof checked through the verifier
    v1 = verify_ms(comp, StarkProof(pproof), config)
    # one whole prove() on a freshly committed trace
    scheme2, ch2 = commit_trace(log, trace, config)
    proof, res["prove_total_ms"] = sync_ms(lambda: prove([comp], ch2, scheme2))
    res["device_phases_ms"] = res["constraint_kernel_ms"] + res["finalize_ms"] + res["composition_commit_ms"] + res["prove_values_ms"]
    res["host_share_ms"] = res["prove_total_ms"] - res["device_phases_ms"]
    res["verify_ms"] = verify_ms(comp, proof, config)
    res["verified"] = True
    res["piecewise_proof_verify_ms"] = v1
    # the constraint kernel alone (HIP events) against its bounds
    cols = comp.trace_on_eval_domain(tr, scheme.twiddles)
    scratch = SecureColumnByCoords.zeros(1 << (log + 1))
    coeffs = [alpha] * comp.n_constraints
    dinv = A.denominator_inverses(log, log + 1)

    def kernel():
        A.evaluate_constraint_quotients(A.AIR_WIDE_FIB, cols, log, 1, coeffs, dinv, scratch)
    kernel()
    L.sync()
    ts = []
    for _ in range(reps):
        e0, e1 = L.Event(), L.Event()
        e0.record()
        kernel()
        e1.record()
        ts.append(e0.elapsed_ms(e1))
    rows = 1 << (log + 1)
    k = {"ms": statistics.median(ts), "bytes": (N_COLS + 8) * 4 * rows}
    k["hbm_bound_ms"] = k["bytes"] / HBM_COPY * 1e3
    k["valu_bound_ms"] = isa["valu_per_row"] * rows / VALU_ONE_PORT * 1e3
    k["achieved_tb_s"] = k["bytes"] / k["ms"] / 1e9
    k["x_larger_bound"] = k["ms"] / max(k["hbm_bound_ms"], k["valu_bound_ms"])
    res["constraint_kernel"] = k
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20")
    ap.add_argument("--log22", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    L.init(0)
    isa = isa_counts()
    logs = [int(x) for x in args.logs.split(",")] + ([22] if args.log22 else [])
    run(10, 2, isa)                                  # warm-up: kernels loaded, pools filled
    out = {"tool": "bench_prove", "device": L.device_name(), "isa": isa, "runs": [run(lg, args.reps, isa) for lg in logs]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

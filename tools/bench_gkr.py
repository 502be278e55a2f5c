#!/usr/bin/env python3
"""LogUp-GKR on one MI355X: per-op device time (HIP events, median of --reps after --warmup) at n = 20 and 24 with GB/s and
the fraction of 8 TB/s, the VALU issue bound of each sum kernel (VALU instructions of its loop body, from the ISA, times the
terms, at the one-port integer peak of DESIGN §4), and prove_batch wall time on each path (the whole proof in one library call /
sum-check rounds on the device / the host loop, run alternately in one process) split into device time, synchronous read-backs and
the host remainder.  Prints one JSON line.  The time of k_gkr_round_finish per launch comes from a separate `rocprofv3
--kernel-trace --stats -- python tools/bench_gkr.py --no-ops --sizes 20 --paths device` run; the transcript kernels of the one-call
path (k_gkr_layer_begin / k_gkr_layer_end) from one with `--paths one_call --sizes "" --batches 1,5,64`.

    python tools/bench_gkr.py [--sizes 20,24] [--reps 20] [--warmup 3] [--prove-reps 9] [--paths one_call,device,host] [--no-ops]
                              [--batches 1,5,64] [--batch-log 12] [--out FILE]
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

from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import gkr as G  # noqa: E402
from tstwo_amd.channel import Blake2sChannel  # noqa: E402
from tstwo_amd.fields import P, QM31  # noqa: E402

HBM = 8e12
VALU_ONE_PORT = 35.3e12          # integer lane-ops/s, one issue port
SUM_KERNELS = {"grand_product": "k_sumILi0ELb0E", "logup_generic": "k_sumILi1ELb0E", "logup_multiplicities": "k_sumILi2ELb0E",
               "logup_singles": "k_sumILi3ELb0E"}


def loop_valu(asm: str, sym: str) -> int:
    """VALU instructions in the body of the kernel's grid-stride loop (the largest backward branch region)."""
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
    best = 0
    for i, line in enumerate(lines):
        b = re.match(r"^s_cbranch_\w+\s+(\.LBB\S+)|^s_branch\s+(\.LBB\S+)", line)
        if b:
            tgt = b.group(1) or b.group(2)
            if tgt in labels and labels[tgt] <= i:
                best = max(best, sum(1 for x in lines[labels[tgt]:i + 1] if x.startswith("v_")))
    return best


def sum_valu_counts():
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "gkr_ops.s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                               os.path.join(ROOT, "tstwo_amd", "csrc", "gkr_ops.hip"), "-o", s], stderr=subprocess.DEVNULL)
        asm = open(s).read()
    return {k: loop_valu(asm, v) for k, v in SUM_KERNELS.items()}


def rand_secure(rng, n):
    return G.Mle.secure([rng.integers(0, P, size=n, dtype=np.uint32) for _ in range(4)])


def rand_felt(rng):
    return QM31.from_u32_unchecked(*[int(x) for x in rng.integers(0, P, size=4)])


def time_op(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    L.sync()
    ts = []
    for _ in range(reps):
        a, b = L.Event(), L.Event()
        a.record()
        fn()
        b.record()
        ts.append(a.elapsed_ms(b) * 1e-3)
    return statistics.median(ts)


def op_record(t, nbytes, extra=None):
    r = {"us": round(t * 1e6, 2), "GBps": round(nbytes / t / 1e9, 1), "frac_8TBps": round(nbytes / t / HBM, 3)}
    r.update(extra or {})
    return r


def bench_ops(n, reps, warmup, valu):
    rng = np.random.default_rng(n)
    N = 1 << n
    out = {}
    y = [rand_felt(rng) for _ in range(n)]
    v = rand_felt(rng)
    eq_out = G.Mle.uninitialized_secure(N)
    words = np.array([w for yi in y for w in yi.tup()], dtype=np.uint32)
    out["eq_table"] = op_record(time_op(lambda: L.call("tstwo_gkr_gen_eq_evals", words.ctypes.data_as(L.u32p), n, G._q(v), eq_out.ptrs()),
                                        reps, warmup), 16 * N)
    num, den, data = rand_secure(rng, N), rand_secure(rng, N), rand_secure(rng, N)
    mult = G.Mle.base(rng.integers(0, P, size=N, dtype=np.uint32))
    o1, o2 = G.Mle.uninitialized_secure(N // 2), G.Mle.uninitialized_secure(N // 2)
    out["next_layer_grand_product"] = op_record(time_op(
        lambda: L.call("tstwo_gkr_next_layer_grand_product", data.ptrs(), n, o1.ptrs()), reps, warmup), 16 * N + 8 * N)
    for name, kind, nm, rb in (("logup_generic", 1, num, 16), ("logup_multiplicities", 2, mult, 4), ("logup_singles", 3, None, 0)):
        out["next_layer_" + name] = op_record(time_op(
            lambda kind=kind, nm=nm: L.call("tstwo_gkr_next_layer_logup", kind, nm.ptrs() if nm else G._null4(), den.ptrs(), n, o1.ptrs(),
                                            o2.ptrs()), reps, warmup), (16 + rb) * N + 16 * N)
    r = rand_felt(rng)
    out["fold_secure"] = op_record(time_op(
        lambda: L.call("tstwo_mle_fix_first_variable_secure", data.ptrs(), n, G._q(r), o1.ptrs()), reps, warmup), 16 * N + 8 * N)
    out["fold_base"] = op_record(time_op(
        lambda: L.call("tstwo_mle_fix_first_variable_base", C.c_void_p(mult.col.ptr), n, G._q(r), o1.ptrs()), reps, warmup), 4 * N + 8 * N)
    # sums over a layer of N values (n_vars = n - 1 oracle variables, N / 4 terms)
    slot = L.DeviceBuffer(32)
    lam = rand_felt(rng)
    eqe = rand_secure(rng, N // 4)
    terms = N // 4
    for name, kind, nm, rb in (("grand_product", 0, None, 0), ("logup_generic", 1, num, 16), ("logup_multiplicities", 2, mult, 4),
                               ("logup_singles", 3, None, 0)):
        t = time_op(lambda kind=kind, nm=nm: L.call("tstwo_gkr_sum_poly_async", kind, eqe.ptrs(), nm.ptrs() if nm else G._null4(),
                                                    (data if kind == 0 else den).ptrs(), n - 1, G._q(lam), C.c_void_p(slot.ptr)),
                    reps, warmup)
        nbytes = (16 + rb) * N + 16 * terms
        bound = terms * valu[name] / VALU_ONE_PORT
        out["sum_" + name] = op_record(t, nbytes, {"valu_per_term": valu[name], "valu_bound_us": round(bound * 1e6, 2),
                                                    "frac_of_valu_bound": round(bound / t, 3),
                                                    "hbm_bound_us": round(nbytes / HBM * 1e6, 2)})
    return out


def make_instance(rng, kind, n):
    N = 1 << n
    den = rand_secure(rng, N)
    if kind == G.GRAND_PRODUCT:
        return G.Layer.grand_product(den)
    if kind == G.LOGUP_GENERIC:
        return G.Layer.logup_generic(rand_secure(rng, N), den)
    if kind == G.LOGUP_MULTIPLICITIES:
        return G.Layer.logup_multiplicities(G.Mle.base(rng.integers(0, P, size=N, dtype=np.uint32)), den)
    return G.Layer.logup_singles(den)


PATHS = {"one_call": {"one_call": True}, "device": {"device_rounds": True}, "host": {"device_rounds": False}, "default": {}}


def bench_prove(layers, reps, paths=("device", "host")):
    """Wall time of prove_batch on each of `paths` (PATHS: the sum-check rounds on the device, the host loop, or the call without
    the keyword), run alternately in this process on the same layers, split into: device time (HIP events from the first library
    call after a read-back to the next read-back: the kernels of that stretch plus the host's launch gaps between them), the count
    of synchronous read-backs, and the rest (host protocol work between a read-back and the next launch, the read-backs' own
    latency).  Per path: the median repetition, and the spread (min, max) of the wall time over the repetitions."""
    rec = {p: [] for p in paths}
    orig_dm, orig_call = L.download_many, L.call
    for it in range(reps + 1):
        for path in paths:
            st = {"readbacks": 0, "device_s": 0.0}
            seg = [None]

            def call(name, *args, seg=seg, st=st):
                if name == "tstwo_gkr_prove_batch":         # the one-call path: launches and the one read-back inside the call
                    start = L.Event().record()
                    res = orig_call(name, *args)
                    st["device_s"] += start.elapsed_ms(L.Event().record()) * 1e-3
                    st["readbacks"] += 1
                    return res
                if seg[0] is None and name.startswith(("tstwo_gkr_", "tstwo_mle_")) and name != "tstwo_gkr_prove_batch_words":
                    seg[0] = L.Event().record()              # the first launch of the stretch
                return orig_call(name, *args)

            def dm(pieces, st=st, seg=seg):
                if seg[0] is not None:
                    stop = L.Event().record()
                    st["device_s"] += seg[0].elapsed_ms(stop) * 1e-3
                res = orig_dm(pieces)
                st["readbacks"] += 1
                seg[0] = None
                return res
            L.sync()
            L.download_many, L.call = dm, call
            t0 = time.perf_counter()
            try:
                G.prove_batch(Blake2sChannel(), layers, **PATHS[path])
                L.sync()
            finally:
                L.download_many, L.call = orig_dm, orig_call
            wall = time.perf_counter() - t0
            if it:                              # the first run warms the allocator and the code paths
                rec[path].append((wall, st))
    out = {}
    for path in paths:
        runs = sorted(rec[path], key=lambda x: x[0])
        wall, st = runs[len(runs) // 2]
        out[path] = {"wall_ms": round(wall * 1e3, 2), "wall_ms_min": round(runs[0][0] * 1e3, 2), "wall_ms_max": round(runs[-1][0] * 1e3, 2),
                     "reps": len(runs), "device_ms": round(st["device_s"] * 1e3, 2), "readbacks": st["readbacks"],
                     "outside_kernels_ms": round((wall - st["device_s"]) * 1e3, 2),
                     "outside_kernels_frac": round(1 - st["device_s"] / wall, 3),
                     "per_readback_outside_us": round((wall - st["device_s"]) / max(st["readbacks"], 1) * 1e6, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prove-reps", type=int, default=9)
    ap.add_argument("--paths", default="device,host", help="prove_batch paths, run alternately: " + ", ".join(PATHS))
    ap.add_argument("--no-ops", action="store_true", help="skip the per-op timings")
    ap.add_argument("--batches", default="", help="also prove batches of this many LogUpGeneric instances of 2^--batch-log values")
    ap.add_argument("--batch-log", type=int, default=12)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file (profiles/gkr_device_rounds.json)")
    a = ap.parse_args()
    paths = tuple(a.paths.split(","))
    L.init(0)
    res = {"tool": "bench_gkr", "device": L.device_name(), "valu_one_port_lane_ops": VALU_ONE_PORT, "ops": {}, "prove_batch": {}}
    valu = None if a.no_ops else sum_valu_counts()
    for k in [int(s) for s in a.batches.split(",") if s]:
        rng = np.random.default_rng(2000 + k)
        batch = [make_instance(rng, G.LOGUP_GENERIC, a.batch_log) for _ in range(k)]
        res["prove_batch"][f"batch_{k}x{a.batch_log}"] = bench_prove(batch, a.prove_reps, paths)
        del batch
    for n in [int(s) for s in a.sizes.split(",") if s]:
        if not a.no_ops:
            res["ops"][str(n)] = bench_ops(n, a.reps, a.warmup, valu)
            L.call("tstwo_trim")
        rng = np.random.default_rng(1000 + n)
        single = [make_instance(rng, G.LOGUP_GENERIC, n)]
        res["prove_batch"][f"logup_generic_{n}"] = bench_prove(single, a.prove_reps, paths)
        mixed = [make_instance(rng, G.LOGUP_GENERIC, n), make_instance(rng, G.GRAND_PRODUCT, n - 2),
                 make_instance(rng, G.LOGUP_MULTIPLICITIES, n - 4), make_instance(rng, G.LOGUP_SINGLES, n - 6)]
        res["prove_batch"][f"mixed_{n}"] = bench_prove(mixed, a.prove_reps, paths)
        del single, mixed
        L.call("tstwo_trim")
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

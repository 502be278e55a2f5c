#!/usr/bin/env python3
"""The 8-lanes-per-hash Poseidon252 kernels (csrc/poseidon_coop.hip) against the lane-per-hash ones on one MI355X, by the method of
the DESIGN §4.6 table: HIP events, median of --reps after --warmup, min and max beside it.  One JSON object per line:

  lone       hash_many_coop against hash_many at n_msgs = 1, felts_per_msg = 1 (one sponge step = one permutation + conversions)
  layer      commit_layer_coop against commit_layer at log 4 .. 18, children-only nodes and 4-column leaves; "coop_wins" where the
             cooperative kernel is faster by more than the two spreads: the largest such log common to both is kP252CoopMaxLog
  fri        FriProver.commit over Poseidon252, one column: the one-call path against the host transcript; wall time and device time
  channel    one device channel step (mix + draw) against the host step: 3 host permutations and a 32-byte read-back
  isa        (--isa, no GPU needed) VALU instructions of a partial and of a full Hades round of both hash_many kernels

    python tools/bench_poseidon_coop.py [--reps 10] [--warmup 2] [--out profiles/poseidon_coop.jsonl] [--only lone,layer,fri,channel]
    python tools/bench_poseidon_coop.py --isa
    python tools/bench_poseidon_coop.py --only fri --root <a checkout of another commit with its library built>   # host transcript there
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M31_P = 2**31 - 1


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def device_times(L, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    L.sync()
    ts = []
    for _ in range(reps):
        a, b = L.Event(), L.Event()
        a.record()
        fn()
        b.record()
        ts.append(a.elapsed_ms(b))
    return stats(ts)


def wall_times(L, fn, reps, warmup):
    """host clock around work that ends synchronised, and the device time of the same calls"""
    for _ in range(warmup):
        fn()
    L.sync()
    wall, dev = [], []
    for _ in range(reps):
        a, b = L.Event(), L.Event()
        L.sync()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        L.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_ms(b))
    return stats(wall), stats(dev)


def faster_beyond_spread(new, old):
    return new["median"] + (new["max"] - new["min"]) + (old["max"] - old["min"]) < old["median"]


# ---------------------------------------------------------------- ISA
def _lines(asm, sym):
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


def round_counts(asm, sym):
    """The Hades round loops are the backward-branch regions that hold Montgomery products: the smallest is the partial round (the
    S-box on s2 only), the smallest one enclosing it with more products the full round."""
    labels, lines = _lines(asm, sym)
    loops = []
    for i, line in enumerate(lines):
        b = re.match(r"^s_cbranch_\w+\s+(\.LBB\S+)|^s_branch\s+(\.LBB\S+)", line)
        if b and (b.group(1) or b.group(2)) in labels and labels[b.group(1) or b.group(2)] <= i:
            loops.append((labels[b.group(1) or b.group(2)], i))
    valu = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_"))
    mad = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_mad_u64_u32"))
    dpp = lambda a, b: sum(1 for x in lines[a:b + 1] if "_dpp" in x.split()[0])
    rounds = sorted((b - a, a, b) for a, b in loops if mad(a, b))
    _, pa, pb = rounds[0]
    fulls = [(a, b) for _, a, b in rounds if a <= pa and b >= pb and mad(a, b) > mad(pa, pb)]
    fa, fb = fulls[0] if fulls else (pa, pb)
    return {"round_partial_valu": valu(pa, pb), "round_full_valu": valu(fa, fb), "round_partial_mad_u64_u32": mad(pa, pb),
            "round_full_mad_u64_u32": mad(fa, fb), "round_partial_dpp": dpp(pa, pb), "per_permutation_valu": 83 * valu(pa, pb) + 8 * valu(fa, fb)}


def isa_rows():
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for src, sym in (("poseidon.hip", "k_p252_hash_many"), ("poseidon_coop.hip", "k_p252c_hash_many")):
            out = os.path.join(d, src + ".s")
            subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                                   os.path.join(HERE, "tstwo_amd", "csrc", src), "-o", out])
            rows.append({"row": "isa", "kernel": sym, **round_counts(open(out).read(), sym)})
    return rows


# ---------------------------------------------------------------- timings
def bench_lone(L, a):
    src, dst = L.DeviceBuffer(32), L.DeviceBuffer(32)
    src.upload(np.arange(1, 9, dtype=np.uint32))
    call = lambda e: (lambda: L.call(e, C.c_void_p(src.ptr), 1, 1, C.c_void_p(dst.ptr)))
    rows = []
    for _ in range(2):                                     # the two entries alternate
        old = device_times(L, call("tstwo_poseidon252_hash_many"), a.reps, a.warmup)
        new = device_times(L, call("tstwo_poseidon252_hash_many_coop"), a.reps, a.warmup)
        rows.append({"row": "lone", "n_msgs": 1, "felts_per_msg": 1, "hash_many_ms": old, "hash_many_coop_ms": new,
                     "ratio": old["median"] / new["median"]})
    return rows


def bench_layers(L, a):
    rng = np.random.default_rng(2)
    rows = []
    empty = L.ptr_array([])
    for log in range(4, 19):
        n = 1 << log
        prev, out = L.DeviceBuffer(64 * n), L.DeviceBuffer(32 * n)
        w = rng.integers(0, 2**32, size=(2 * n, 8), dtype=np.uint32)
        w[:, 7] &= 0x03FFFFFF                             # canonical
        prev.upload(w.reshape(-1))
        cols = [L.DeviceBuffer(4 * n) for _ in range(4)]
        for c in cols:
            c.upload(rng.integers(0, M31_P, size=n, dtype=np.uint32))
        ptrs = L.ptr_array([c.ptr for c in cols])
        row = {"row": "layer", "log": log}
        for shape, args in (("children_only", (C.c_void_p(prev.ptr), empty, 0)), ("leaves_4_columns", (None, ptrs, 4))):
            call = lambda e: (lambda: L.call(e, log, *args, C.c_void_p(out.ptr)))
            old = device_times(L, call("tstwo_poseidon252_merkle_commit_layer"), a.reps, a.warmup)
            new = device_times(L, call("tstwo_poseidon252_merkle_commit_layer_coop"), a.reps, a.warmup)
            row[shape] = {"lane_per_node_ms": old, "coop_ms": new, "coop_wins": faster_beyond_spread(new, old)}
        rows.append(row)
        for b in [prev, out] + cols:
            b.free()
    wins = [r["log"] for r in rows if r["children_only"]["coop_wins"] and r["leaves_4_columns"]["coop_wins"]]
    rows.append({"row": "threshold", "coop_wins_both_shapes_at_logs": wins, "kP252CoopMaxLog_measured": max(wins) if wins else -1})
    return rows


def bench_fri(L, T, a, where):
    rows = []
    has_one_call = hasattr(T, "DevicePoseidon252Channel")
    for circle_log in (16, 20):
        domain = T.CanonicCoset(circle_log).circleDomain()
        tw = T.precompute_twiddles(domain.halfCoset)
        rng = np.random.default_rng(circle_log)
        polys = [T.HipCirclePoly(T.HipColumn(rng.integers(0, M31_P, size=1 << (circle_log - 1), dtype=np.uint32))) for _ in range(4)]
        evs = T.evaluate_polynomials(polys, domain, tw)
        col = T.SecureEvaluation(domain, T.SecureColumnByCoords([e.values for e in evs]))
        cfg = T.FriConfig(5, 1, 20)
        commit = lambda dev: (lambda: T.FriProver.commit(T.Poseidon252Channel(), cfg, [col], tw, device_channel=dev,
                                                         merkle_channel=T.Poseidon252MerkleChannel))
        row = {"row": "fri", "where": where, "circle_log": circle_log}
        for _ in range(2 if has_one_call else 1):          # alternate the two paths; keep the later pass
            row["host_transcript_wall_ms"], row["host_transcript_device_ms"] = wall_times(L, commit(False), a.reps, a.warmup)
            if has_one_call:
                row["one_call_wall_ms"], row["one_call_device_ms"] = wall_times(L, commit(True), a.reps, a.warmup)
        if has_one_call:
            row["one_call_wins"] = faster_beyond_spread(row["one_call_wall_ms"], row["host_transcript_wall_ms"])
        rows.append(row)
    return rows


def bench_channel(L, T, a):
    from tstwo_amd.poseidon import DevicePoseidon252Channel, FieldElement252, Poseidon252Channel
    host = Poseidon252Channel()
    host.mix_u64(1)
    dch = DevicePoseidon252Channel(host)
    root = L.DeviceBuffer(32)
    root.upload(np.arange(1, 9, dtype=np.uint32))
    felt = L.DeviceBuffer(16)
    dev = device_times(L, lambda: dch.mix_root_draw_felt(root.ptr, felt.ptr), a.reps, a.warmup)

    def host_step():
        r = FieldElement252.from_words(root.download(count=8))          # the 32-byte read-back (synchronises)
        host.mix_root(r)
        host.draw_felt()
    ts = []
    for i in range(a.reps + a.warmup):
        t0 = time.perf_counter()
        host_step()
        if i >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return [{"row": "channel", "device_step_ms": dev, "host_step_wall_ms": stats(ts)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    ap.add_argument("--only", default="lone,layer,fri,channel")
    ap.add_argument("--isa", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose tstwo_amd package is measured")
    a = ap.parse_args()
    rows = []
    if a.isa:
        rows += isa_rows()
    else:
        sys.path.insert(0, os.path.abspath(a.root))
        import tstwo_amd as T
        from tstwo_amd import _lib as L
        L.init(0)
        where = "this checkout" if os.path.abspath(a.root) == HERE else os.path.relpath(os.path.abspath(a.root), HERE)
        only = a.only.split(",")
        rows.append({"row": "device", "name": L.device_name(), "reps": a.reps, "warmup": a.warmup, "where": where})
        if "lone" in only:
            rows += bench_lone(L, a)
        if "layer" in only:
            rows += bench_layers(L, a)
        if "fri" in only:
            rows += bench_fri(L, T, a, where)
        if "channel" in only:
            rows += bench_channel(L, T, a)
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

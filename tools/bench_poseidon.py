#!/usr/bin/env python3
"""Poseidon252 on one MI355X: hash_many permutations/s (k = 2), Merkle commits of 32 columns x 2^20 and 2^22 and of 256 columns
in 8 trees x 2^22 (BASELINE config 5's shape), the column-free top of a tree in one launch against one launch per layer, and the
grind in nonces/s.  Device times are HIP events, median of --reps after --warmup.  Each kernel is VALU-bound: its bound is the
VALU instructions of the Hades round loop (from the ISA: partial and full rounds, v_mad_u64_u32 counted apart) times the
permutations at the one-port integer rate of DESIGN §4.  The CPU figure
is the Python model's permutation rate (tests/poseidon_model.py) on one thread.  Prints one JSON line.

    python tools/bench_poseidon.py [--reps 10] [--warmup 2] [--quick]
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

from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import poseidon as PS  # noqa: E402
from tstwo_amd.backend import HipColumn  # noqa: E402

VALU_ONE_PORT = 35.3e12          # integer lane-ops/s, one issue port
M31_P = 2**31 - 1
KERNELS = {"hash_many": "k_p252_hash_many", "layer_leaf": "k_p252_layerILb0E", "layer_node": "k_p252_layerILb1E",
           "tail": "k_p252_tail", "grind": "k_p252_grind"}


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


def _loops(labels, lines):
    """Backward-branch regions (start, end) of the kernel."""
    out = []
    for i, line in enumerate(lines):
        b = re.match(r"^s_cbranch_\w+\s+(\.LBB\S+)|^s_branch\s+(\.LBB\S+)", line)
        if b:
            tgt = b.group(1) or b.group(2)
            if tgt in labels and labels[tgt] <= i:
                out.append((labels[tgt], i))
    return out


def isa_counts(asm: str, sym: str) -> dict:
    """Hades round loops are the loops that read the round constants (s_load of kArk).  The compiler keeps the partial round as
    the innermost one (the S-box on s2: 2 Montgomery products) and the full round as the enclosing loop that also takes the
    cubes of s0 and s1 (6 products); a region's VALU count is what one iteration of it issues."""
    labels, lines = _lines(asm, sym)
    loops = _loops(labels, lines)
    valu = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_"))
    mad = lambda a, b: sum(1 for x in lines[a:b + 1] if x.startswith("v_mad_u64_u32"))
    rounds = sorted(((b - a, a, b) for a, b in loops if any(x.startswith("s_load") for x in lines[a:b + 1])))
    _, pa, pb = rounds[0]
    partial, partial_mad = valu(pa, pb), mad(pa, pb)
    fulls = [(a, b) for _, a, b in rounds if a <= pa and b >= pb and mad(a, b) > partial_mad]
    fa, fb = fulls[0] if fulls else (pa, pb)
    full, full_mad = valu(fa, fb), mad(fa, fb)
    kinds = {}
    for x in lines[pa:pb + 1]:
        if x.startswith("v_"):
            op = x.split()[0]
            kinds[op] = kinds.get(op, 0) + 1
    return {"round_full_valu": full, "round_partial_valu": partial, "round_full_mad_u64_u32": full_mad,
            "round_partial_mad_u64_u32": partial_mad, "per_permutation_valu": 83 * partial + 8 * full,
            "per_permutation_mad_u64_u32": 83 * partial_mad + 8 * full_mad,
            "partial_round_mix_top": dict(sorted(kinds.items(), key=lambda kv: -kv[1])[:8])}


def compile_isa() -> dict:
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "poseidon.s")
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                               os.path.join(ROOT, "tstwo_amd", "csrc", "poseidon.hip"), "-o", out])
        asm = open(out).read()
    return {k: isa_counts(asm, sym) for k, sym in KERNELS.items()}


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
        ts.append(a.elapsed_ms(b))
    return statistics.median(ts)


def bound_ms(isa, n_lanes, perms_per_lane):
    """VALU issue time of the permutations alone (the sponge's conversions and loads add ~2 %)."""
    return n_lanes * isa["per_permutation_valu"] * perms_per_lane / VALU_ONE_PORT * 1e3


def commit_perms(n_cols, log):
    """Permutations of one tree: leaves absorb ceil(C/8) elements, nodes 2."""
    leaf = (-(-n_cols // 8) + 2) // 2
    return leaf * (1 << log) + 2 * ((1 << log) - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a profiler run)")
    a = ap.parse_args()
    L.init(0)
    res = {"device": L.device_name()}
    isa = compile_isa()
    res["isa"] = isa
    rng = np.random.default_rng(1)

    # hash_many, k = 2
    n = 1 << (18 if a.quick else 22)
    words = np.zeros((n, 16), dtype=np.uint32)
    words[:, :7] = rng.integers(0, 2**32, size=(n, 7), dtype=np.uint32)
    words[:, 8:15] = rng.integers(0, 2**32, size=(n, 7), dtype=np.uint32)
    src, dst = L.DeviceBuffer(words.nbytes), L.DeviceBuffer(32 * n)
    src.upload(words.reshape(-1))
    t = time_op(lambda: L.call("tstwo_poseidon252_hash_many", C.c_void_p(src.ptr), n, 2, C.c_void_p(dst.ptr)), a.reps, a.warmup)
    b = bound_ms(isa["hash_many"], n, 2)
    res["hash_many_k2"] = {"n": n, "ms": t, "perms_per_s": 2 * n / t * 1e3, "valu_bound_ms": b, "fraction_of_bound": b / t}
    del src, dst

    # commits
    res["commit"] = {}
    shapes = [(32, 16)] if a.quick else [(32, 20), (32, 22)]
    for n_cols, log in shapes:
        cols = [HipColumn(rng.integers(0, M31_P, size=1 << log, dtype=np.uint32)) for _ in range(n_cols)]
        buf = L.DeviceBuffer(32 * ((2 << log) - 1))
        ptrs, logs = L.ptr_array([c.ptr for c in cols]), L.u32x([log] * n_cols)
        t = time_op(lambda: L.call("tstwo_poseidon252_merkle_commit", ptrs, logs, n_cols, C.c_void_p(buf.ptr), None), a.reps, a.warmup)
        perms = commit_perms(n_cols, log)
        leaf_abs = (-(-n_cols // 8) + 2) // 2
        b = (bound_ms(isa["layer_leaf"], 1 << log, leaf_abs) + bound_ms(isa["layer_node"], (1 << log) - 1, 2))
        res["commit"][f"{n_cols}x2^{log}"] = {"ms": t, "permutations": perms, "perms_per_s": perms / t * 1e3, "valu_bound_ms": b,
                                             "fraction_of_bound": b / t}
        del cols, buf
    if not a.quick:
        log, n_trees = 22, 8
        trees = [[HipColumn(rng.integers(0, M31_P, size=1 << log, dtype=np.uint32)) for _ in range(32)] for _ in range(n_trees)]
        t0 = time.perf_counter()
        L.sync()
        ev0, ev1 = L.Event(), L.Event()
        ev0.record()
        provers = PS.Poseidon252MerkleProver.commit_many(trees, sync_root=False)
        ev1.record()
        t = ev0.elapsed_ms(ev1)
        perms = n_trees * commit_perms(32, log)
        b = n_trees * (bound_ms(isa["layer_leaf"], 1 << log, 3) + bound_ms(isa["layer_node"], (1 << log) - 1, 2))
        res["commit"]["8 trees x 32x2^22"] = {"ms": t, "permutations": perms, "perms_per_s": perms / t * 1e3, "valu_bound_ms": b,
                                             "fraction_of_bound": b / t, "wall_ms": (time.perf_counter() - t0) * 1e3}
        del trees, provers

    # the column-free top: one single-workgroup launch (layers 2^8 .. 1) against one launch per layer
    cols = [HipColumn(rng.integers(0, M31_P, size=1 << 9, dtype=np.uint32)) for _ in range(4)]
    buf = L.DeviceBuffer(32 * ((2 << 9) - 1))
    ptrs, logs = L.ptr_array([c.ptr for c in cols]), L.u32x([9] * 4)
    t_tail = time_op(lambda: L.call("tstwo_poseidon252_merkle_commit", ptrs, logs, 4, C.c_void_p(buf.ptr), None), a.reps, a.warmup)
    empty = L.ptr_array([])

    def per_layer():
        L.call("tstwo_poseidon252_merkle_commit_layer", 9, None, ptrs, 4, C.c_void_p(buf.ptr + 32 * ((1 << 9) - 1)))
        for lg in range(8, -1, -1):
            L.call("tstwo_poseidon252_merkle_commit_layer", lg, C.c_void_p(buf.ptr + 32 * ((2 << lg) - 1)), empty, 0,
                   C.c_void_p(buf.ptr + 32 * ((1 << lg) - 1)))
    t_layers = time_op(per_layer, a.reps, a.warmup)
    res["top_of_tree_4x2^9"] = {"tail_launch_ms": t_tail, "one_launch_per_layer_ms": t_layers}

    # grind: nonces evaluated = the host's batches (2^16, then x4 up to 2^22) up to the one holding the answer
    ch = PS.Poseidon252Channel()
    ch.mix_u64(7)
    bits = 16 if a.quick else 22
    for _ in range(a.warmup):
        PS.grind_poseidon252(ch, 8)
    t0 = time.perf_counter()
    nonce = PS.grind_poseidon252(ch, bits)
    wall = time.perf_counter() - t0
    done, batch = 0, 1 << 16
    while done <= nonce:
        done += batch
        batch = min(batch * 4, 1 << 22)
    b = bound_ms(isa["grind"], done, 2)
    res["grind"] = {"pow_bits": bits, "nonce": nonce, "nonces_evaluated": done, "wall_ms": wall * 1e3, "nonces_per_s": done / wall,
                    "valu_bound_ms": b, "fraction_of_bound": b / (wall * 1e3)}

    # CPU figures (one thread): the independent model and the host implementation of tstwo_amd
    import poseidon_model as M
    t0 = time.perf_counter()
    for i in range(50):
        M.hades([i, 2, 3])
    res["cpu_model_perms_per_s"] = 50 / (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for i in range(200):
        PS.hades_permutation(i, 2, 3)
    res["cpu_host_perms_per_s"] = 200 / (time.perf_counter() - t0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

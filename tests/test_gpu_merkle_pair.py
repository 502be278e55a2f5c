"""-m gpu: k_merkle_leaf_pair (tstwo_amd/csrc/merkle.hip) — the leaf layer of a 16 / 32 / 48 / 64-column tree hashed together with
the column-free layer above it, one lane per pair of sibling leaves.  Every layer of every tree, bit for bit, against a reference:
the hashlib model of tests/merkle_plan.py up to 2^17 leaves, the oracle above; a failure names layer and node.

The shipped library takes the kernel from 2^19 leaves up (Knobs::merkle_pair_log).  Its small sizes — one pair, half a wave, one
wave, several workgroups, two pairs per lane with a partial last row — run in one fresh child process on the experiments build
with TSTWO_MERKLE_PAIR_LOG=1 and TSTWO_MERKLE_CAP=3, the pattern of test_gpu_merkle_plan.py's grid-stride test."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import rand_column
from oracle import oracle as orc

import merkle_plan as MP

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402
from gpu_util import dev, ptrs, vp  # noqa: E402
from test_gpu_merkle_plan import assert_wraps, n_cus  # noqa: E402

# the shapes live in merkle_plan.py (PAIR_TEST), where the coverage condition of test_cpu_merkle_plan.py reads them too
PAIR_LOG, CAP = MP.PAIR_TEST["pair_log"], MP.PAIR_TEST["cap"]      # 1, 3: TSTWO_MERKLE_PAIR_LOG / TSTWO_MERKLE_CAP of the child
SMALL_LOGS = MP.PAIR_TEST["small_logs"]                  # (1, 6, 7, 8, 10): one pair, half a wave, exactly one wave, 2 and 8 workgroups of pairs
MANY_TREES, MANY_COLS = MP.PAIR_TEST["many_trees"], MP.PAIR_TEST["many_cols"]      # (2, 8), 32
MANY_LOGS = MP.PAIR_TEST["many_logs"]                    # (8, 17).  2^8: committed tree by tree (commit_many shares launches from 2^17 leaves up); 2^17:
                                                         # ONE pair launch for all trees — 8 trees under CAP have 96 workgroups each for 256
                                                         # workgroups of pairs: three rows per lane, a partial last one
WRAP_COLS, WRAP_LOG = MP.PAIR_TEST["wrap"]               # 16, 19: 2^18 pairs under a cap of 768 workgroups: two pairs per lane, a partial second row
SHIPPED_COLS, SHIPPED_LOG = MP.PAIR_TEST["shipped"]      # 32, 19


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def tree_columns(n_cols, log, tree=0):
    """The host columns of tree number `tree` of a shape (seeded by shape, tree and column)."""
    return [rand_column(41000 + 4096 * tree + 64 * log + k, 1 << log) for k in range(n_cols)]


_refs = {}


def reference(n_cols, log, tree=0):
    """Layers root first, computed once per (shape, tree) and shared, never modified."""
    key = (n_cols, log, tree)
    if key not in _refs:
        cols, logs = tree_columns(n_cols, log, tree), [log] * n_cols
        _refs[key] = MP.model_layers(cols, logs) if (1 << log) <= 1 << 17 else orc.merkle_commit(cols, logs)[0]
    return _refs[key]


def commit_one(dcols, log):
    """tstwo_merkle_commit into a zeroed layers buffer (no digest is all zeros): (layers as uint8 [2^(log+1) - 1, 32], root)."""
    layers = L.DeviceBuffer(32 * ((2 << log) - 1))
    layers.zero()
    root = (C.c_uint8 * 32)()
    L.call("tstwo_merkle_commit", ptrs(dcols), L.u32x([log] * len(dcols)), len(dcols), vp(layers), root)
    flat = layers.download(np.uint8).reshape(-1, 32)
    layers.free()
    return flat, bytes(root)


def commit_many(dtrees, log):
    """tstwo_merkle_commit_many of equally shaped trees into zeroed layers buffers: (layers per tree, roots)."""
    n = len(dtrees)
    bufs = [L.DeviceBuffer(32 * ((2 << log) - 1)) for _ in range(n)]
    reqs, keep = (L.CommitRequest * n)(), []
    for t in range(n):
        bufs[t].zero()
        cp, lgs = ptrs(dtrees[t]), L.u32x([log] * len(dtrees[t]))
        keep += [cp, lgs]
        reqs[t] = L.CommitRequest(cp, lgs, len(dtrees[t]), bufs[t].ptr)
    roots = (C.c_uint8 * (32 * n))()
    L.call("tstwo_merkle_commit_many", reqs, n, roots)
    flats = [b.download(np.uint8).reshape(-1, 32) for b in bufs]
    for b in bufs:
        b.free()
    return flats, [bytes(roots)[32 * t:32 * t + 32] for t in range(n)]


def verdict(flat, root, ref):
    """'ok', or what is wrong: the first wrong digest from the leaves up, or the root argument."""
    bad = MP.first_mismatch(flat, ref)
    if bad is not None:
        return f"layer_{bad[0]}_node_{bad[1]}"
    return "ok" if root == ref[0].tobytes() else "root_argument"


def forced_case_names():
    names = [f"{c}x{lg}" for c in (16, 32, 48, 64) for lg in SMALL_LOGS]
    names += [f"many{n}x{lg}_tree{t}{how}" for lg in MANY_LOGS for n in MANY_TREES for t in range(n) for how in ("", "_single")]
    return names + [f"{WRAP_COLS}x{WRAP_LOG}"]


def forced_child_main():
    """The child process of test_pair_kernel_forced_at_small_sizes: one line per case, its name and `ok` or the first wrong node."""
    L.init(0)
    ver = L.version()
    print("version", ver.replace(" ", "_"), flush=True)
    assert "experiments" in ver
    assert os.environ.get("TSTWO_MERKLE_PAIR_LOG") == str(PAIR_LOG) and os.environ.get("TSTWO_MERKLE_CAP") == str(CAP)
    assert_wraps(1 << (WRAP_LOG - 1), 1, n_cus(), CAP, tail=True)       # lanes of the pair kernel own pairs: 2^(log - 1) of them
    assert_wraps(1 << (max(MANY_LOGS) - 1), max(MANY_TREES), n_cus(), CAP, tail=True)      # the shared launch of 8 trees
    for n_cols in (16, 32, 48, 64):
        for log in SMALL_LOGS:
            flat, root = commit_one([dev(c) for c in tree_columns(n_cols, log)], log)
            print(f"{n_cols}x{log}", verdict(flat, root, reference(n_cols, log)), flush=True)
    for lg in MANY_LOGS:
        for n in MANY_TREES:
            dtrees = [[dev(c) for c in tree_columns(MANY_COLS, lg, t)] for t in range(n)]
            flats, roots = commit_many(dtrees, lg)
            for t in range(n):
                ref = reference(MANY_COLS, lg, t)
                print(f"many{n}x{lg}_tree{t}", verdict(flats[t], roots[t], ref), flush=True)
                flat1, root1 = commit_one(dtrees[t], lg)             # the same tree committed on its own
                same = np.array_equal(flat1, flats[t]) and root1 == roots[t]
                print(f"many{n}x{lg}_tree{t}_single", verdict(flat1, root1, ref) if same else "differs_from_commit_many", flush=True)
    flat, root = commit_one([dev(c) for c in tree_columns(WRAP_COLS, WRAP_LOG)], WRAP_LOG)
    print(f"{WRAP_COLS}x{WRAP_LOG}", verdict(flat, root, reference(WRAP_COLS, WRAP_LOG)), flush=True)
    L.sync()


_CHILD_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_merkle_pair as M
M.forced_child_main()
"""
CHILD_TIMEOUT = 60                                       # seconds


def test_pair_kernel_forced_at_small_sizes():
    """k_merkle_leaf_pair<1..4> where the shipped plan never runs it: 16 / 32 / 48 / 64 columns at 2^1 (one pair: the parent is
    the root), 2^6 (half a wave of pairs), 2^7 (exactly one wave), 2^8 and 2^10 leaves (several workgroups); 2 and 8 trees of
    32 x 2^8 through tstwo_merkle_commit_many and of 32 x 2^17 against the model
    and against the same trees committed one by one — at 2^8 commit_many commits tree by tree, at 2^17 all trees share ONE pair
    launch (blockIdx.y = tree: its columns, its layers, its layer log - 1), and with 8 trees the capped grid (96 workgroups per
    tree) gives every lane three pairs with a partial last row; 16 x 2^19,
    where the capped grid (768 workgroups on 256 CUs) gives every lane two pairs and leaves a partial second row: the deferred
    parent store, the clamped loads and the skipped stores of tail lanes.  One fresh child process on the experiments build
    with TSTWO_MERKLE_PAIR_LOG=1 and TSTWO_MERKLE_CAP=3; it asserts that it runs that build with those variables and, from the CU
    count the library reports, that the last launch is capped with a partial row.  The grid itself cannot be observed from here."""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    script = _CHILD_SCRIPT.format(root=os.path.dirname(tests_dir), tests=tests_dir)
    env = dict(os.environ, TSTWO_HIP_LIB=L.LIB_EXP_PATH, TSTWO_MERKLE_PAIR_LOG=str(PAIR_LOG), TSTWO_MERKLE_CAP=str(CAP))
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the child was killed after {CHILD_TIMEOUT} s: {err[-2000:]}")
    print(f"child process: {time.time() - t0:.1f} s")
    assert out.returncode == 0, f"child exit status {out.returncode}: {out.stderr[-2000:]}"
    got = dict(ln.split(" ", 1) for ln in out.stdout.strip().splitlines())
    assert "experiments" in got["version"]
    wrong = {name: got.get(name, "missing") for name in forced_case_names() if got.get(name) != "ok"}
    assert not wrong, f"first wrong digest (from the leaves up) per case: {wrong}"


@pytest.mark.parametrize("n_trees", [1, 2])
def test_shipped_library_takes_the_pair_kernel_at_log_19(n_trees):
    """One tree (tstwo_merkle_commit) and two trees (tstwo_merkle_commit_many, shared launches) of 32 x 2^19 on the shipped
    library, whose plan takes k_merkle_leaf_pair<2> from 2^19 leaves up: roots and all layers against the oracle."""
    assert "experiments" not in L.version()
    dtrees = [[dev(c) for c in tree_columns(SHIPPED_COLS, SHIPPED_LOG, t)] for t in range(n_trees)]
    if n_trees == 1:
        flat, root = commit_one(dtrees[0], SHIPPED_LOG)
        flats, roots = [flat], [root]
    else:
        flats, roots = commit_many(dtrees, SHIPPED_LOG)
    for t in range(n_trees):
        ref = reference(SHIPPED_COLS, SHIPPED_LOG, t)
        bad = MP.first_mismatch(flats[t], ref)
        assert bad is None, f"tree {t} of {n_trees}: first wrong digest (from the leaves up) at layer {bad[0]}, node {bad[1]}"
        assert roots[t] == ref[0].tobytes(), f"tree {t} of {n_trees}: root argument"


def test_columns_at_odd_word_offsets_keep_the_static_leaf():
    """The pair kernel's loads fetch two words, so the plan takes it only for 8-byte aligned columns.  32 x 2^19 on the shipped
    library with every column, then with the last column only, starting 4 bytes into its buffer: all layers and the root are
    the oracle's, as for aligned columns of the same words."""
    cols = tree_columns(SHIPPED_COLS, SHIPPED_LOG, 0)
    ref = reference(SHIPPED_COLS, SHIPPED_LOG, 0)
    padded = [dev(np.concatenate([np.zeros(1, dtype=np.uint32), c])) for c in cols]
    plain = [dev(c) for c in cols[:-1]]
    for name, addr in (("all", [b.ptr + 4 for b in padded]), ("last", [b.ptr for b in plain] + [padded[-1].ptr + 4])):
        assert any(a & 7 for a in addr) and not any(a & 3 for a in addr)
        layers = L.DeviceBuffer(32 * ((2 << SHIPPED_LOG) - 1))
        layers.zero()
        root = (C.c_uint8 * 32)()
        L.call("tstwo_merkle_commit", L.ptr_array(addr), L.u32x([SHIPPED_LOG] * SHIPPED_COLS), SHIPPED_COLS, vp(layers), root)
        flat = layers.download(np.uint8).reshape(-1, 32)
        layers.free()
        bad = MP.first_mismatch(flat, ref)
        assert bad is None, f"{name} skewed: first wrong digest (from the leaves up) at layer {bad[0]}, node {bad[1]}"
        assert bytes(root) == ref[0].tobytes(), name

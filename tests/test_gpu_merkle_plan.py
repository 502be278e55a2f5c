"""-m gpu: every branch of the Merkle launch plan (tstwo_amd/csrc/merkle_plan.h, walked by merkle.hip) and the grid-stride paths
of its one-lane-per-node kernels, every layer bit for bit against a
reference: the hashlib model of tests/merkle_plan.py up to 2^17 leaves, the oracle above.  Which shape takes which launches is
accounted for without a GPU in test_cpu_merkle_plan.py."""
import ctypes as C
import hashlib
import os
import re
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
from gpu_util import dev, dev_empty, ptrs, vp  # noqa: E402

POOL = 37          # columns above 2^12 rows repeat this many device buffers (inputs are read only; the reference gets the same repeats)


def half_odds(k):
    return orc.lib().orc_half_odds_initial(k)


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def columns(logs, seed=7000):
    """(key per column, host array per key): the j-th column of a log size is array j of that size, modulo POOL for long ones."""
    keys, count = [], {}
    for lg in logs:
        j = count.get(lg, 0)
        count[lg] = j + 1
        keys.append((lg, j if lg <= 12 else j % POOL))
    return keys, {k: rand_column(seed + 1000 * k[0] + k[1], 1 << k[0]) for k in set(keys)}


def upload(hostc):
    return {k: dev(a) for k, a in hostc.items()}


def commit(keys, devc, logs):
    """tstwo_merkle_commit into a zeroed layers buffer (no digest is all zeros): (layers as uint8 [2^(max+1) - 1, 32], root)."""
    layers = L.DeviceBuffer(32 * ((2 << max(logs)) - 1))
    layers.zero()
    root = (C.c_uint8 * 32)()
    L.call("tstwo_merkle_commit", ptrs([devc[k] for k in keys]), L.u32x(logs), len(logs), vp(layers), root)
    return layers.download(np.uint8).reshape(-1, 32), bytes(root)


def reference(cols, logs):
    if MP.n_leaves(logs) <= 1 << 17:
        return MP.model_layers(cols, logs)
    return orc.merkle_commit(cols, logs)[0]


def check_tree(name, logs):
    keys, hostc = columns(logs)
    flat, root = commit(keys, upload(hostc), logs)
    ref = reference([hostc[k] for k in keys], logs)
    bad = MP.first_mismatch(flat, ref)
    assert bad is None, f"{name}: first wrong digest (from the leaves up) at layer {bad[0]}, node {bad[1]}; launches {MP.plan(logs)}"
    assert root == ref[0].tobytes(), f"{name}: root argument"


@pytest.mark.parametrize("name", list(MP.MATRIX))
def test_matrix(name):
    check_tree(name, MP.MATRIX[name])


@pytest.mark.parametrize("log", [0, 1, 8, 13])
def test_commit_layer_children_only(log):
    """tstwo_merkle_commit_layer with a child layer and no columns is k_merkle_inner; a null and an empty column table."""
    prev = np.random.default_rng(7700 + log).integers(0, 256, size=(2 << log, 32), dtype=np.uint8)
    want = orc.commit_on_layer(log, prev, [])
    dprev = dev(prev)
    for table in (C.c_void_p(0), ptrs([])):
        out = dev_empty(8 << log)
        out.zero()
        L.call("tstwo_merkle_commit_layer", log, vp(dprev), table, 0, vp(out))
        got = out.download(np.uint8, 32 << log).reshape(-1, 32)
        bad = (got != want).any(axis=1)
        assert not bad.any(), f"log {log}: first wrong node {int(np.argmax(bad))}"


def n_cus():
    m = re.search(r"(\d+) CUs", L.device_name())
    assert m, L.device_name()
    return int(m.group(1))


def assert_wraps(n_nodes, n_trees, cus, cap_per_cu, tail):
    """The precondition of a grid-stride case: layer_blocks caps the launch, so lanes take a second node; tail: and the last row
    is partial, so some lanes clamp their loads and skip their store."""
    launched, needed = MP.layer_blocks(n_nodes, n_trees, cus, cap_per_cu)
    assert needed > launched, f"{n_nodes} nodes x {n_trees} trees on {cus} CUs, cap {cap_per_cu}: {needed} workgroups fit the cap of {launched}"
    if tail:
        assert n_nodes % (launched * 256) != 0, f"{n_nodes} nodes: {launched} workgroups leave no partial row"


@pytest.mark.parametrize("kind", ["layer<F>", "layer<T>"])
def test_shipped_wrap_points(kind):
    """The smallest trees at which the shipped library itself (merkle_cap = 32 workgroups per CU) makes a lane of k_merkle_layer
    take a second node: 5 columns at the first log size whose layer exceeds the cap (<false>), and 2 columns at that size under
    one column a size above (<true>).  On 256 CUs: [22]*5 and [23] + [22]*2, two rows per lane.  The shapes follow from the CU
    count the library reports; the grid itself cannot be observed from here."""
    cus = n_cus()
    w = next((lg for lg in range(24) if MP.layer_blocks(1 << lg, 1, cus)[1] > MP.layer_blocks(1 << lg, 1, cus)[0]), None)
    assert w is not None, f"{cus} CUs: no layer of at most 2^23 nodes exceeds the cap of {cus * MP.MERKLE_CAP} workgroups"
    logs = [w] * 5 if kind == "layer<F>" else [w + 1] + [w] * 2
    assert_wraps(1 << w, 1, cus, MP.MERKLE_CAP, tail=False)
    assert any(l.kind.startswith(kind) and l.args[0] == w for l in MP.launches(logs))
    check_tree(f"{kind} at log {w}", logs)


# ------------------------------------------------------------------ grid stride and tail lanes at small sizes: experiments build
CAP = 3            # TSTWO_MERKLE_CAP of the child: 768 workgroups on 256 CUs, a lane stride of 196608 nodes
TREE_CASES = {"5x18": [18] * 5, "260x18": [18] * 260, "3x19+5x18": [19] * 3 + [18] * 5, "1x19+260x18": [19] + [18] * 260,
              "16x18": [18] * 16, "32x18": [18] * 32, "48x18": [18] * 48, "64x18": [18] * 64, "4x18": [18] * 4}
MANY = MP.CAP_TEST_MANY                                  # (5, 16, 17): trees, columns, log size of the tstwo_merkle_commit_many case
FRI_LOG, FRI_LAST = 20, 12                               # circle evaluation of 2^20 rows: the first fused fold + leaf launch has 2^18 nodes


def digests(layers):
    return [hashlib.blake2s(np.ascontiguousarray(l).tobytes()).hexdigest() for l in layers]


def split_layers(flat):
    return [flat[(1 << k) - 1:(2 << k) - 1] for k in range(flat.shape[0].bit_length())]


def inner_case_prev():
    return np.random.default_rng(7800).integers(0, 256, size=(2 << 18, 32), dtype=np.uint8)


def many_case_columns():
    n_trees, n_cols, lg = MANY
    pool = [rand_column(7900 + i, 1 << lg) for i in range(20)]
    return pool, [[(t * 7 + k) % len(pool) for k in range(n_cols)] for t in range(n_trees)]


def run_fri():
    """tstwo_fri_commit_layers on one circle evaluation of 2^FRI_LOG rows from a fresh channel: every tree's root, the alphas, the
    channel state, and a digest over every tree and every evaluation it returned."""
    log, last, tw_log = FRI_LOG, FRI_LAST, FRI_LOG + 1
    cols = [dev(rand_column(8800 + k, 1 << log)) for k in range(4)]
    tw, itw = dev_empty(1 << tw_log), dev_empty(1 << tw_log)
    L.call("tstwo_twiddles_build", half_odds(tw_log), tw_log, vp(tw), vp(itw))
    n_trees = 1 + (log - 1 - last)
    chan, alphas = dev(np.zeros(10, dtype=np.uint32)), dev_empty(4 * (n_trees + 3))
    alphas.zero()
    outs, n_out, first = (L.FriLayerOut * (n_trees + 1))(), C.c_size_t(0), L.vp()
    L.call("tstwo_fri_commit_layers", ptrs(cols), L.u32x([log]), 1, vp(itw), tw_log, last, vp(chan), vp(alphas), n_trees + 3,
           C.byref(first), outs, n_trees + 1, C.byref(n_out))
    assert n_out.value == n_trees
    h, roots = hashlib.blake2s(), []
    owned = [L.DeviceBuffer.adopt(first.value, 32 * ((2 << log) - 1))]
    trees = [owned[0]]
    for i in range(n_out.value):
        lg = outs[i].log_size
        ev = [L.DeviceBuffer.adopt(outs[i].cols[k], 4 << lg) for k in range(4)]
        owned += ev
        for e in ev:
            h.update(e.download().tobytes())
        if outs[i].layers:
            trees.append(L.DeviceBuffer.adopt(outs[i].layers, 32 * ((2 << lg) - 1)))
            owned.append(trees[-1])
    for t in trees:
        b = t.download(np.uint8).tobytes()
        roots.append(b[:32].hex())
        h.update(b)
    res = roots + [alphas.download(np.uint32, 4 * n_trees).tobytes().hex(), chan.download(np.uint32, 10).tobytes().hex(), h.hexdigest()]
    for b in owned:
        b.free()
    return res


def cap_child_main():
    """The child process of test_grid_stride_and_tail_lanes_at_small_sizes: one line per case, the case's name and a digest per layer."""
    L.init(0)
    ver = L.version()
    print("version", ver.replace(" ", "_"), flush=True)
    assert "experiments" in ver and os.environ.get("TSTWO_MERKLE_CAP") == str(CAP)
    cus = n_cus()
    for n_nodes, n_trees in [(1 << 18, 1), (1 << 19, 1), (1 << MANY[2], MANY[0]), (1 << 16, MANY[0])]:
        assert_wraps(n_nodes, n_trees, cus, CAP, tail=True)
    for name, logs in TREE_CASES.items():
        keys, hostc = columns(logs)
        flat, _ = commit(keys, upload(hostc), logs)
        print(name, *digests(split_layers(flat)), flush=True)
    dprev, out = dev(inner_case_prev()), dev_empty(8 << 18)
    out.zero()
    L.call("tstwo_merkle_commit_layer", 18, vp(dprev), C.c_void_p(0), 0, vp(out))
    print("inner18", *digests([out.download(np.uint8, 32 << 18)]), flush=True)
    n_trees, n_cols, lg = MANY
    pool, idx = many_case_columns()
    dpool = [dev(c) for c in pool]
    nbytes = 32 * ((2 << lg) - 1)
    bufs = [L.DeviceBuffer(nbytes) for _ in range(n_trees)]
    reqs, keep = (L.CommitRequest * n_trees)(), []
    for t in range(n_trees):
        bufs[t].zero()
        cp, lgs = ptrs([dpool[i] for i in idx[t]]), L.u32x([lg] * n_cols)
        keep += [cp, lgs]
        reqs[t] = L.CommitRequest(cp, lgs, n_cols, bufs[t].ptr)
    L.call("tstwo_merkle_commit_many", reqs, n_trees, None)
    print("many", *[d for b in bufs for d in digests(split_layers(b.download(np.uint8).reshape(-1, 32)))], flush=True)
    print("fri", *run_fri(), flush=True)
    L.sync()


def expected_cap_lines():
    """What the child must print, from the oracle (the FRI case: from the shipped library, in this process)."""
    want = {}
    for name, logs in TREE_CASES.items():
        keys, hostc = columns(logs)
        want[name] = digests(orc.merkle_commit([hostc[k] for k in keys], logs)[0])
    want["inner18"] = digests([orc.commit_on_layer(18, inner_case_prev(), [])])
    n_trees, n_cols, lg = MANY
    pool, idx = many_case_columns()
    want["many"] = [d for t in range(n_trees) for d in digests(orc.merkle_commit([pool[i] for i in idx[t]], [lg] * n_cols)[0])]
    assert "experiments" not in L.version()
    want["fri"] = run_fri()
    return want


_CAP_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_merkle_plan as M
M.cap_child_main()
"""
CHILD_TIMEOUT = 10                                       # seconds: the child took 1.4 to 1.5 s on an MI355X


def test_grid_stride_and_tail_lanes_at_small_sizes():
    """The grid-stride code of every one-lane-per-node kernel — rows > 1, the deferred digest store, the clamped loads of tail
    lanes — at 2^16 to 2^19 nodes: one fresh child process runs the experiments build with TSTWO_MERKLE_CAP=3, so that a launch
    has at most 3 workgroups per CU (768 on 256 CUs: a lane stride of 196608 nodes, two rows and a partial last row from 2^18
    nodes; 153 workgroups per tree for five trees).  Its cases: k_merkle_layer<false> in one and two launches, <true> in one and
    two, k_merkle_leaf_static<1..4>, k_merkle_leaf4<false>, k_merkle_inner, five trees through k_merkle_leaf_static and
    k_merkle_inner_set, and a FRI commit whose fused fold + leaf launch (k_merkle_leaf4<true>) has 2^18 nodes.  Every layer of
    every tree must be the oracle's; the FRI roots, alphas, channel and evaluations must be what the shipped library, which stays
    under its own cap at these sizes, gives in this process.

    What this cannot verify: the grid.  The child asserts, from the CU count the library reports, that every such launch exceeds
    its cap and leaves a partial row, and that it runs the experiments build with the variable set; that the experiments build
    reads the variable is test_libraries_read_only_the_kept_switches's assertion.  No more is claimed.

    The child took 1.4 to 1.5 s on an MI355X (the whole test 4.2 s, most of it the oracle's trees); it is killed
    after CHILD_TIMEOUT, and a child that exits non-zero or is killed fails the test with the tail of its stderr."""
    want = expected_cap_lines()
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    script = _CAP_SCRIPT.format(root=os.path.dirname(tests_dir), tests=tests_dir)
    env = dict(os.environ, TSTWO_HIP_LIB=L.LIB_EXP_PATH, TSTWO_MERKLE_CAP=str(CAP))
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the child was killed after {CHILD_TIMEOUT} s: {err[-2000:]}")
    print(f"child process: {time.time() - t0:.1f} s")
    assert out.returncode == 0, f"child exit status {out.returncode}: {out.stderr[-2000:]}"
    got = {ln.split(" ", 1)[0]: ln.split(" ")[1:] for ln in out.stdout.strip().splitlines()}
    assert "experiments" in got["version"][0]
    for name, w in want.items():
        assert name in got and len(got[name]) == len(w), name
        wrong = [i for i, (a, b) in enumerate(zip(got[name], w)) if a != b]
        assert not wrong, f"{name}: differs at entries {wrong} of {len(w)} (a tree's layers are listed root first)"

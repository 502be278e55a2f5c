"""Helpers of the Merkle launch-plan tests (test_cpu_merkle_plan.py, test_gpu_merkle_plan.py); no GPU, nothing from oracle/
or tstwo_amd/.

model_layers: the tree stated directly with hashlib.blake2s (the reference of every matrix shape of at most 2^17 leaves).
plan:         a plain restatement of the host dispatch of tstwo_amd/csrc/merkle.hip, used ONLY for coverage accounting.
MATRIX:       the named shapes the GPU test commits; EXPECTED: the launches some of them were chosen for.
"""
import hashlib
from typing import NamedTuple, Optional

import numpy as np

# the constants of the dispatch; test_cpu_merkle_plan.py checks them against the source
K_UP_LOG = 16             # merkle.hip: kUpLog
K_MAX_TREES = 8           # merkle.hip: kMaxTrees
K_MAX_HASH_COLS = 256     # common.h:   kMaxHashCols
MERKLE_CAP = 32           # common.h:   Knobs::merkle_cap (workgroups per CU of a one-lane-per-node launch)


# ------------------------------------------------------------------ the tree, by its definition
def model_layers(cols, log_sizes):
    """MerkleProver.commit by its definition: node i of layer lg = Blake2s(left || right, if layer lg + 1 exists, ||
    LE32(c[i]) for every column c of log size lg, in table order) — as tests/golden/gen_golden.py states it.  Returns the layers
    root first, layer k a uint8 array [2^k, 32]."""
    assert len(cols) == len(log_sizes)
    max_log = max(log_sizes, default=0)
    layers, prev = [None] * (max_log + 1), None
    for lg in range(max_log, -1, -1):
        n = 1 << lg
        parts = []
        if prev is not None:
            parts.append(prev.reshape(n, 64))
        here = [np.asarray(c, dtype="<u4") for c, l in zip(cols, log_sizes) if l == lg]
        assert all(c.shape == (n,) for c in here)
        if here:
            parts.append(np.ascontiguousarray(np.stack(here, axis=1)).view(np.uint8).reshape(n, 4 * len(here)))
        w = sum(p.shape[1] for p in parts)
        buf = np.ascontiguousarray(np.concatenate(parts, axis=1)).tobytes() if parts else b""
        out = b"".join(hashlib.blake2s(buf[i * w:(i + 1) * w]).digest() for i in range(n))
        prev = layers[lg] = np.frombuffer(out, dtype=np.uint8).reshape(n, 32)
    return layers


# ------------------------------------------------------------------ the host dispatch, restated
class Launch(NamedTuple):
    kind: str                       # the kernel (or arm A-D of commit_upper_levels) and, for k_merkle_layer, its launch count
    args: tuple                     # what the issue's notation shows in brackets
    stop: Optional[int] = None      # arms A-D: the log_stop of their commit_upper_levels call
    words: Optional[int] = None     # k_merkle_layer: message length W in 32-bit words

    def __str__(self):
        return f"{self.kind}({','.join(str(a) for a in self.args)})"


def _upper(log_child, stop):
    """commit_upper_levels: the four arms in source order.  A(log_child); B, C(log_child, remaining); D(log_child, levels)."""
    out = []
    while log_child > stop:
        remaining, parents_log = log_child - stop, log_child - 1
        if parents_log >= 9 and 9 <= remaining <= 16:
            out.append(Launch("A", (log_child,), stop))
            log_child -= 9
        elif parents_log <= 6:
            out.append(Launch("B", (log_child, remaining), stop))
            log_child -= remaining
        elif parents_log <= 8:
            out.append(Launch("C", (log_child, remaining), stop))
            log_child -= remaining
        else:
            levels = min(remaining, 7)
            out.append(Launch("D", (log_child, levels), stop))
            log_child -= levels
    return out


def _column_free(log_child, stop):
    """commit_column_free: s2c(log_child) writes layers log_child - 1 and log_child - 2; inner_set(log_out)."""
    out = []
    while log_child >= stop + 2 and log_child - 2 >= K_UP_LOG:
        out.append(Launch("s2c", (log_child,)))
        log_child -= 2
    if log_child > stop and log_child - 1 >= K_UP_LOG:
        log_child -= 1
        out.append(Launch("inner_set", (log_child,)))
    return out + _upper(log_child, stop)


def layer_launches(n_cols, has_prev):
    """The column split of commit_layer's generic path: columns per launch of k_merkle_layer."""
    child_words, takes, col_base = (16 if has_prev else 0), [], 0
    while True:
        take = min(n_cols - col_base, K_MAX_HASH_COLS)
        if col_base + take != n_cols:
            take -= (child_words + col_base + take) % 16
        takes.append(take)
        col_base += take
        if col_base >= n_cols:
            return takes


def _layer(log, has_prev, n_cols):
    """commit_layer."""
    if not has_prev and log <= 30 and n_cols in (16, 32, 48, 64):
        return [Launch(f"static{n_cols}", (log,))]
    if not has_prev and log <= 30 and n_cols == 4:
        return [Launch("leaf4", (log,))]
    if has_prev and n_cols == 0:
        return [Launch("inner", (log,))]
    n = len(layer_launches(n_cols, has_prev))
    return [Launch(f"layer<{'T' if has_prev else 'F'}>x{n}", (log, n_cols), None, (16 if has_prev else 0) + n_cols)]


def launches(log_sizes):
    """commit_tree (tstwo_merkle_commit): the launches of one tree, in order."""
    log_sizes = list(log_sizes)
    max_log = max(log_sizes, default=0)
    if len(log_sizes) == 4 and 1 <= max_log <= K_UP_LOG and all(l == max_log for l in log_sizes):
        whole = max_log <= 9
        first = Launch(f"leaf4_upq<{1024 if whole else 256}>", (max_log,))
        return [first] + ([] if whole else _upper(max_log - 7, 0))
    out, have_prev, lg = [], False, max_log
    while lg >= 0:
        k = log_sizes.count(lg)
        if k == 0 and have_prev:
            stop = lg
            while stop > 0 and (stop - 1) not in log_sizes:
                stop -= 1
            out += _column_free(lg + 1, stop)
            lg = stop - 1
            continue
        out += _layer(lg, have_prev, k)
        have_prev = True
        lg -= 1
    return out


def plan(log_sizes):
    """The launches tstwo_merkle_commit makes for columns of these log sizes, as strings: static64(17), leaf4(18),
    layer<T>x2(6,257) (two launches of k_merkle_layer<true> for 257 columns at log 6), s2c(20), inner_set(16), A(16), B(7,3),
    C(9,1), D(16,7) (the four arms of commit_upper_levels in source order: log_child, then remaining or levels),
    leaf4_upq<256>(12).

    This is a READING of commit_tree / commit_layer / commit_column_free / commit_upper_levels in tstwo_amd/csrc/merkle.hip, not
    a measurement: it must be updated together with them.  It is used only to account for which branches the matrix visits; no
    GPU assertion depends on it."""
    return [str(l) for l in launches(log_sizes)]


def layer_blocks(n_nodes, n_trees, n_cus, cap_per_cu=MERKLE_CAP):
    """layer_blocks of merkle.hip: (workgroups launched, workgroups the layer would need without the cap)."""
    blocks = -(-n_nodes // 256)
    cap = n_cus * cap_per_cu // n_trees
    return (blocks if blocks <= cap else cap if cap else 1), blocks


# ------------------------------------------------------------------ the shapes
def _named(pairs):
    return "+".join(f"{n}x{lg}" for n, lg in pairs), [lg for n, lg in pairs for _ in range(n)]


T_COUNTS = [1, 15, 16, 17, 47, 48, 49, 239, 240, 241, 256, 257, 272, 300, 513]       # k_merkle_layer<true>: n columns at log 6 under one at log 7
F_COUNTS = [2, 31, 33, 63, 65, 80, 128, 255, 257, 512, 513]                         # k_merkle_layer<false>: n columns at log 5

MATRIX = dict(
    # column-free runs that stop above a lower layer with columns
    [_named(p) for p in ([(3, 20), (2, 17)], [(3, 20), (2, 16)], [(3, 19), (2, 3)], [(16, 18), (3, 12)], [(4, 17), (1, 9)],
                         [(3, 16), (2, 8)], [(3, 16), (2, 7)], [(3, 14), (2, 1)], [(3, 12), (2, 0)], [(64, 17), (16, 16)])]
    + [("every_layer_6..0", [6, 5, 4, 3, 2, 1, 0])]
    # uniform trees: commit_upper_levels from every start
    + [_named([(5, lg)]) for lg in (7, 8, 9, 10, 17, 18)]
    + [_named([(4, lg)]) for lg in (9, 12, 13, 14, 15)]
    + [(f"T{n}", [7] + [6] * n) for n in T_COUNTS]
    + [(f"F{n}", [5] * n) for n in F_COUNTS]
    # the static leaf at its smallest sizes
    + [_named([(16, 0)]), _named([(32, 1)]), _named([(48, 0)]), _named([(64, 2)])]
)

# The launches the shapes above were chosen for (the issue's lists, written out in plan()'s notation: the leaf launch included,
# k_merkle_layer with its launch and column counts).
EXPECTED = {
    "3x20+2x17": ["layer<F>x1(20,3)", "s2c(20)", "layer<T>x1(17,2)", "inner_set(16)", "A(16)", "B(7,7)"],
    "3x20+2x16": ["layer<F>x1(20,3)", "s2c(20)", "inner_set(17)", "layer<T>x1(16,2)", "A(16)", "B(7,7)"],
    "3x19+2x3": ["layer<F>x1(19,3)", "s2c(19)", "inner_set(16)", "A(16)", "B(7,3)", "layer<T>x1(3,2)", "B(3,3)"],
    "16x18+3x12": ["static16(18)", "s2c(18)", "D(16,3)", "layer<T>x1(12,3)", "A(12)", "B(3,3)"],
    "4x17+1x9": ["leaf4(17)", "inner_set(16)", "D(16,6)", "layer<T>x1(9,1)", "C(9,9)"],
    "3x16+2x8": ["layer<F>x1(16,3)", "D(16,7)", "layer<T>x1(8,2)", "C(8,8)"],
    "3x16+2x7": ["layer<F>x1(16,3)", "D(16,7)", "C(9,1)", "layer<T>x1(7,2)", "B(7,7)"],
    "3x14+2x1": ["layer<F>x1(14,3)", "A(14)", "B(5,3)", "layer<T>x1(1,2)", "B(1,1)"],
    "3x12+2x0": ["layer<F>x1(12,3)", "A(12)", "B(3,2)", "layer<T>x1(0,2)"],
    "every_layer_6..0": ["layer<F>x1(6,1)"] + [f"layer<T>x1({lg},1)" for lg in (5, 4, 3, 2, 1, 0)],
    "64x17+16x16": ["static64(17)", "layer<T>x1(16,16)", "A(16)", "B(7,7)"],
}


def n_leaves(log_sizes):
    return 1 << max(log_sizes, default=0)


def first_mismatch(got_flat, ref_layers):
    """got_flat: the downloaded layers buffer as uint8 [2^(max_log+1) - 1, 32]; ref_layers: root first.  None when equal, else
    (layer, node) of the first wrong digest, from the leaf layer up — the order the launches wrote them."""
    assert got_flat.shape[0] == (1 << len(ref_layers)) - 1
    for lg in range(len(ref_layers) - 1, -1, -1):
        bad = (got_flat[(1 << lg) - 1:(2 << lg) - 1] != ref_layers[lg]).any(axis=1)
        if bad.any():
            return lg, int(np.argmax(bad))
    return None

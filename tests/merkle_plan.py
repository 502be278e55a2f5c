"""Helpers of the Merkle launch-plan tests (test_cpu_merkle_plan.py, test_gpu_merkle_plan.py); no GPU, nothing from oracle/
or tstwo_amd/.

model_layers: the tree stated directly with hashlib.blake2s (the reference of every matrix shape of at most 2^17 leaves).
steps:        the tests' own statement of the launch plan of tstwo_merkle_commit (layer_steps: of tstwo_merkle_commit_layer,
              set_steps: of tstwo_merkle_commit_many), launch by launch with grid, workgroup and kernel parameters.  The library's
              statement is tstwo_amd/csrc/merkle_plan.h; test_cpu_merkle_plan.py compiles that header and compares the two.
plan:         the same for one tree with the library's defaults, in the short notation of EXPECTED.
MATRIX:       the named shapes the GPU test commits; EXPECTED: the launches some of them were chosen for.
"""
import hashlib
from typing import NamedTuple, Optional

import numpy as np

# the constants of the dispatch; test_cpu_merkle_plan.py checks them against the compiled header
K_UP_LOG = 16             # kUpLog
K_MAX_TREES = 8           # kMaxTrees
K_MAX_HASH_COLS = 256     # kMaxHashCols
MERKLE_CAP = 32           # Knobs::merkle_cap (workgroups per CU of a one-lane-per-node launch)
MERKLE_PAIR_LOG = 19      # Knobs::merkle_pair_log (smallest leaf layer hashed together with the layer above it)

FOLD_ERROR = "fri commit: the fold was not carried by the leaf launch"


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


# ------------------------------------------------------------------ the launch plan, restated
class PlanError(Exception):
    """An input without a plan; str(): the library's error text."""


class Env(NamedTuple):
    """What the plan reads besides the input: the device's compute units and the two launch-shape parameters."""
    n_cus: int = 256
    cap: int = MERKLE_CAP
    pair_log: int = MERKLE_PAIR_LOG


class Launch(NamedTuple):
    kind: str                       # the kernel (or arm A-D of the levels below 2^kUpLog nodes) and, for k_merkle_layer, its launch count
    args: tuple                     # what the issue's notation shows in brackets
    stop: Optional[int] = None      # arms A-D: the layer their run of column-free levels stops at
    words: Optional[int] = None     # k_merkle_layer: message length W in 32-bit words
    grid: Optional[int] = None      # workgroups per tree
    wg: int = 256                   # lanes per workgroup
    trees: int = 1                  # trees the launch covers (blockIdx.y)
    tree: int = 0                   # the first of them
    levels: Optional[int] = None    # arms A-D, leaf4_upq: levels per workgroup
    cols: Optional[tuple] = None    # k_merkle_layer: (first column, columns) of this launch among the layer's columns
    lp: Optional[tuple] = None      # k_merkle_layer: total_words, w_begin, w_end, col_word0, n_cols, load_state, is_final
    fold: bool = False              # the launch first writes its 4 columns as a fold
    hook: bool = False              # the launch takes the channel step on the root

    def __str__(self):
        return f"{self.kind}({','.join(str(a) for a in self.args)})"


class Hook:
    """A channel step offered to the launches of one tree; pending until a launch takes it."""
    def __init__(self, offered):
        self.pending = bool(offered)


def layer_blocks(n_nodes, n_trees, n_cus, cap_per_cu=MERKLE_CAP):
    """Workgroups of a one-lane-per-node launch: (workgroups launched, workgroups the layer would need without the cap)."""
    blocks = -(-n_nodes // 256)
    cap = n_cus * cap_per_cu // n_trees
    return (blocks if blocks <= cap else cap if cap else 1), blocks


def _blocks(n_nodes, n_trees, env):
    return layer_blocks(n_nodes, n_trees, env.n_cus, env.cap)[0]


def _upper(log_child, stop, trees=1, tree=0, hook=None):
    """The column-free levels below 2^kUpLog nodes, 4 lanes per node: the four arms in source order.  A(log_child);
    B, C(log_child, remaining); D(log_child, levels).  A hook is taken by the launch that produces the root of a single tree."""
    root_hook = bool(hook and hook.pending and trees == 1 and stop == 0 and log_child > stop)
    if root_hook:
        hook.pending = False
    out, at = [], dict(stop=stop, trees=trees, tree=tree)
    while log_child > stop:
        remaining, parents_log = log_child - stop, log_child - 1
        if parents_log >= 9 and 9 <= remaining <= 16:
            out.append(Launch("A", (log_child,), grid=1 << (parents_log - 8), wg=1024, levels=9, **at))
            log_child -= 9
        elif parents_log <= 6:
            out.append(Launch("B", (log_child, remaining), grid=1, wg=256, levels=remaining, hook=root_hook, **at))
            log_child -= remaining
        elif parents_log <= 8:
            out.append(Launch("C", (log_child, remaining), grid=1, wg=1024, levels=remaining, hook=root_hook, **at))
            log_child -= remaining
        else:
            levels = min(remaining, 7)
            out.append(Launch("D", (log_child, levels), grid=1 << (parents_log - 6), wg=256, levels=levels, **at))
            log_child -= levels
    return out


def _column_free(log_child, stop, trees=1, tree=0, hook=None, env=Env()):
    """A run of column-free layers: s2c(log_child) writes layers log_child - 1 and log_child - 2; inner_set(log_out); then _upper."""
    out = []
    while log_child >= stop + 2 and log_child - 2 >= K_UP_LOG:
        out.append(Launch("s2c", (log_child,), grid=(1 << (log_child - 2)) // 256, trees=trees, tree=tree))
        log_child -= 2
    if log_child > stop and log_child - 1 >= K_UP_LOG:
        log_child -= 1
        out.append(Launch("inner_set", (log_child,), grid=_blocks(1 << log_child, trees, env), trees=trees, tree=tree))
    return out + _upper(log_child, stop, trees, tree, hook)


def layer_launches(n_cols, has_prev):
    """The column split of a layer's generic path: columns per launch of k_merkle_layer."""
    child_words, takes, col_base = (16 if has_prev else 0), [], 0
    while True:
        take = min(n_cols - col_base, K_MAX_HASH_COLS)
        if col_base + take != n_cols:
            take -= (child_words + col_base + take) % 16
        takes.append(take)
        col_base += take
        if col_base >= n_cols:
            return takes


def _layer(log, has_prev, n_cols, fold=False, aligned16=True, env=Env(), tree=0):
    """One layer from its children (has_prev) and its columns."""
    if log > 31:
        raise PlanError("merkle: log size out of range")
    if not aligned16:
        raise PlanError("merkle: layers must be 16-byte aligned")
    if fold and (has_prev or log > 30 or n_cols != 4):
        raise PlanError(FOLD_ERROR)
    grid = _blocks(1 << log, 1, env)
    if not has_prev and log <= 30 and n_cols in (16, 32, 48, 64):
        return [Launch(f"static{n_cols}", (log,), grid=grid, tree=tree)]
    if not has_prev and log <= 30 and n_cols == 4:
        return [Launch("leaf4", (log,), grid=grid, tree=tree, fold=fold)]
    if has_prev and n_cols == 0:
        return [Launch("inner", (log,), grid=grid, tree=tree)]
    takes = layer_launches(n_cols, has_prev)
    child_words = 16 if has_prev else 0
    words, out, col_base = child_words + n_cols, [], 0
    for i, take in enumerate(takes):
        final = i == len(takes) - 1
        lp = (words, 0 if i == 0 else child_words + col_base, (max(words, 1) + 16) if final else child_words + col_base + take,
              child_words + col_base, take, 0 if i == 0 else 1, 1 if final else 0)
        out.append(Launch(f"layer<{'T' if has_prev else 'F'}>x{len(takes)}", (log, n_cols), None, words, grid=grid, tree=tree,
                          cols=(col_base, take), lp=lp))
        col_base += take
    return out


def takes_pair(log, columns_below, aligned8, env=Env()):
    """Whether the leaf layer of a 16 / 32 / 48 / 64-column tree is hashed together with the column-free layer above it."""
    return 1 <= log <= 30 and log >= env.pair_log and not columns_below and aligned8


def steps(log_sizes, fold=False, hook=False, aligned8=True, aligned16=True, env=Env(), tree=0):
    """tstwo_merkle_commit (with fold / hook: the tree of a FRI commit layer): every launch of one tree, in order.  aligned8: the
    columns of the largest log size are 8-byte aligned; aligned16: the layers buffer is 16-byte aligned.  A hook that no launch
    could take is a trailing launch of the channel kernel."""
    log_sizes = list(log_sizes)
    if any(l > 31 for l in log_sizes):
        raise PlanError("merkle: log size out of range")
    max_log = max(log_sizes, default=0)
    hk = Hook(hook)
    if len(log_sizes) == 4 and 1 <= max_log <= K_UP_LOG and all(l == max_log for l in log_sizes):
        whole = max_log <= 9
        levels = max_log if whole else 7
        out = [Launch(f"leaf4_upq<{1024 if whole else 256}>", (max_log,), grid=1 << (max_log - levels), wg=1024 if whole else 256,
                      tree=tree, levels=levels, fold=fold, hook=whole and hook)]
        if whole:
            hk.pending = False
        else:
            out += _upper(max_log - levels, 0, 1, tree, hk)
    else:
        out, have_prev, lg = [], False, max_log
        while lg >= 0:
            k = log_sizes.count(lg)
            if k == 0 and have_prev:
                stop = lg
                while stop > 0 and (stop - 1) not in log_sizes:
                    stop -= 1
                out += _column_free(lg + 1, stop, 1, tree, hk, env)
                lg = stop - 1
                continue
            if not have_prev and not fold and k in (16, 32, 48, 64) and aligned16 and takes_pair(lg, (lg - 1) in log_sizes, aligned8, env):
                out.append(Launch(f"pair{k}", (lg,), grid=_blocks(1 << (lg - 1), 1, env), tree=tree))
                have_prev = True
                lg -= 2
                continue
            out += _layer(lg, have_prev, k, fold and not have_prev, aligned16, env, tree)
            have_prev = True
            lg -= 1
    if hk.pending:
        out.append(Launch("channel", (), grid=1, wg=64, tree=tree))
    return out


def layer_steps(log, has_prev, n_cols, aligned16=True, env=Env()):
    """tstwo_merkle_commit_layer."""
    return _layer(log, has_prev, n_cols, False, aligned16, env)


class Tree(NamedTuple):
    """One request of tstwo_merkle_commit_many."""
    logs: tuple
    aligned8: bool = True           # every column 8-byte aligned
    aligned16: bool = True          # the layers buffer 16-byte aligned
    null_arg: bool = False          # a null layers buffer, column table or log size table


def uniform_log(trees):
    """The log size of a set that tstwo_merkle_commit_many commits with shared launches: 2 to kMaxTrees trees of one shape of
    16 / 32 / 48 / 64 columns, at most kMaxHashCols columns in all, one log size in kUpLog + 1 .. 30.  None: tree by tree."""
    n = len(trees)
    uniform = 2 <= n <= K_MAX_TREES
    n_cols, lg = (len(trees[0].logs) if n else 0), 0
    for r, t in enumerate(trees):
        if not uniform:
            break
        if t.null_arg:
            raise PlanError("merkle: null argument")
        uniform = len(t.logs) == n_cols and n_cols in (16, 32, 48, 64) and n_cols * n <= K_MAX_HASH_COLS and t.aligned16
        for k, l in enumerate(t.logs):
            if not uniform:
                break
            if r == 0 and k == 0:
                lg = l
            uniform = l == lg
    return lg if uniform and K_UP_LOG + 1 <= lg <= 30 else None


def set_steps(trees, env=Env()):
    """tstwo_merkle_commit_many: a uniform set shares every launch (trees > 1); any other set is committed tree by tree."""
    lg = uniform_log(trees)
    if lg is None:
        return [l for r, t in enumerate(trees) for l in steps(t.logs, False, False, t.aligned8, t.aligned16, env, r)]
    n, n_cols = len(trees), len(trees[0].logs)
    pair = takes_pair(lg, False, all(t.aligned8 for t in trees), env)
    leaf = Launch(f"pair{n_cols}" if pair else f"static{n_cols}", (lg,), grid=_blocks(1 << (lg - 1 if pair else lg), n, env), trees=n)
    return [leaf] + _column_free(lg - 1 if pair else lg, 0, n, 0, None, env)


def launches(log_sizes):
    """steps() with the library's defaults, the launches of k_merkle_layer for one layer as one entry."""
    out = []
    for l in steps(log_sizes):
        if not (out and l.kind.startswith("layer<") and (out[-1].kind, out[-1].args) == (l.kind, l.args)):
            out.append(l)
    return out


def plan(log_sizes):
    """The launches tstwo_merkle_commit makes for columns of these log sizes, as strings: static64(17), pair32(19) (the leaf layer
    and the layer above it), leaf4(18), layer<T>x2(6,257) (two launches of k_merkle_layer<true> for 257 columns at log 6),
    s2c(20), inner_set(16), A(16), B(7,3), C(9,1), D(16,7) (the four arms of the levels below 2^kUpLog nodes in source order:
    log_child, then remaining or levels), leaf4_upq<256>(12)."""
    return [str(l) for l in launches(log_sizes)]


def render(step_list):
    """One line per plan, as tests/merkle_plan_main.cpp prints it: plan()'s notation, then [tree, grid x trees, workgroup, …]."""
    words = []
    for l in step_list:
        ext = [f"t{l.tree}", f"{l.grid}x{l.trees}", str(l.wg)]
        if l.levels is not None:
            ext.append(f"lv{l.levels}")
        if l.lp is not None:
            ext += [f"c{l.cols[0]}+{l.cols[1]}", "lp" + ":".join(str(x) for x in l.lp)]
        words.append(f"{l}[{','.join(ext)}]" + ("+fold" if l.fold else "") + ("+hook" if l.hook else ""))
    return " ".join(words)


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
    # uniform trees: the levels below 2^kUpLog nodes from every start
    + [_named([(5, lg)]) for lg in (7, 8, 9, 10, 17, 18)]
    + [_named([(4, lg)]) for lg in (9, 12, 13, 14, 15)]
    + [(f"T{n}", [7] + [6] * n) for n in T_COUNTS]
    + [(f"F{n}", [5] * n) for n in F_COUNTS]
    # the static leaf at its smallest sizes
    + [_named([(16, 0)]), _named([(32, 1)]), _named([(48, 0)]), _named([(64, 2)])]
    # the pair leaf on the shipped library, and a column-free run behind it that stops above a lower layer with columns
    + [_named([(16, 19)]), _named([(32, 19), (2, 12)])]
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


# What tests/test_gpu_merkle_pair.py commits, and under which parameters: its forced child (experiments build) and the shipped library.
PAIR_TEST = dict(pair_log=1, cap=3,                      # TSTWO_MERKLE_PAIR_LOG / TSTWO_MERKLE_CAP of the child
                 small_logs=(1, 6, 7, 8, 10),            # one pair, half a wave, exactly one wave, 2 and 8 workgroups of pairs
                 many_trees=(2, 8), many_cols=32, many_logs=(8, 17), wrap=(16, 19), shipped=(32, 19))
CAP_TEST_MANY = (5, 16, 17)                              # trees, columns, log size of test_gpu_merkle_plan.py's commit_many case (cap 3)


def gpu_test_commits():
    """(Env, trees) of every commit the two files above make besides MATRIX's: one tree = tstwo_merkle_commit, more = commit_many."""
    p, forced = PAIR_TEST, Env(cap=PAIR_TEST["cap"], pair_log=PAIR_TEST["pair_log"])
    out = [(forced, [Tree((lg,) * c)]) for c in (16, 32, 48, 64) for lg in p["small_logs"]]
    out += [(forced, [Tree((lg,) * p["many_cols"])] * n) for lg in p["many_logs"] for n in p["many_trees"]]
    out += [(forced, [Tree((p["wrap"][1],) * p["wrap"][0])])]
    out += [(Env(), [Tree((p["shipped"][1],) * p["shipped"][0])] * n) for n in (1, 2)]
    n, c, lg = CAP_TEST_MANY
    return out + [(Env(cap=3), [Tree((lg,) * c)] * n)]


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

"""The Merkle launch plan without a GPU: csrc/merkle_plan.h, compiled on its own with the address and undefined behaviour
sanitizers, against the tests' own statement (tests/merkle_plan.py) over a sweep of single trees, single layers and tree sets;
the hashlib model against the oracle; the launches the named shapes were chosen for; the coverage condition on the matrix."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rand_column
from oracle import oracle as orc

import merkle_plan as MP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "tstwo_amd", "csrc")
SMALL = [name for name, logs in MP.MATRIX.items() if MP.n_leaves(logs) <= 1 << 14]


@pytest.mark.parametrize("name", SMALL)
def test_model_layers_equals_the_oracle(name):
    """Two independent statements of the tree — hashlib over explicit messages, the oracle's C layer loop — give the same layers."""
    logs = MP.MATRIX[name]
    cols = [rand_column(9000 + i, 1 << lg) for i, lg in enumerate(logs)]
    model = MP.model_layers(cols, logs)
    olayers, oroot = orc.merkle_commit(cols, logs)
    assert len(model) == len(olayers)
    assert MP.first_mismatch(np.concatenate(model), olayers) is None
    assert model[0].tobytes() == oroot


def test_model_layers_of_small_hand_written_trees():
    import hashlib
    b2 = lambda m: hashlib.blake2s(m).digest()
    le = lambda *v: b"".join(int(x).to_bytes(4, "little") for x in v)
    assert MP.model_layers([], [])[0].tobytes() == b2(b"")
    a, b, c = np.array([1, 2], dtype=np.uint32), np.array([7], dtype=np.uint32), np.array([3, 4], dtype=np.uint32)
    layers = MP.model_layers([a, b, c], [1, 0, 1])
    l0, l1 = b2(le(1, 3)), b2(le(2, 4))
    assert layers[1].tobytes() == l0 + l1 and layers[0].tobytes() == b2(l0 + l1 + le(7))


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/merkle_plan_main.cpp — csrc/merkle_plan.h and nothing else of the library — under the address and undefined behaviour
    sanitizers."""
    out = str(tmp_path_factory.mktemp("merkle_plan") / "merkle_plan_main")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "merkle_plan_main.cpp"), "-o", out])
    return out


def _library_lines(exe, lines):
    p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _own(fn, *args):
    try:
        return MP.render(fn(*args))
    except MP.PlanError as e:
        return f"error: {e}"


def _groups(logs):
    """[19, 19, 12] -> "19*2 12*1" (a tree's columns in table order)."""
    return " ".join(f"{lg}*{len(list(g))}" for lg, g in itertools.groupby(logs))


def _env(env):
    return f"{env.n_cus} {env.cap} {env.pair_log}"


def _tree_line(logs, fold, hook, a8, a16, env):
    return f"T {_env(env)} {int(fold)} {int(hook)} {int(a8)} {int(a16)} {_groups(logs)}"


def _set_line(trees, env):
    return f"S {_env(env)} " + " ".join(f"| {int(t.null_arg)} {int(t.aligned8)} {int(t.aligned16)} {_groups(t.logs)}" for t in trees)


TOP_COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 513)
ENVS = [MP.Env(n_cus, cap, pair_log) for n_cus in (256, 64) for pair_log, cap in ((19, 32), (1, 3))]
FLAGS = list(itertools.product((False, True), repeat=4))             # fold, hook, columns 8-byte aligned, layers 16-byte aligned


def _tree_sweep():
    """Every top log 0..31 x every top column count x every second group (none, or 1 / 16 / 257 columns at any one lower log), each
    with 6 of the 64 combinations of (fold, hook, two alignments, (pair_log, cap), compute units), the choice rotating with the
    shape so that every combination meets every top log, count and second group size; and all 64 with every shape whose second
    group, if any, lies one or two layers below the top."""
    combos = [(f, e) for f in FLAGS for e in ENVS]
    i = 0
    for top in range(32):
        for n in TOP_COUNTS:
            for below, m in [(None, 0)] + [(lg, m) for lg in range(top) for m in (1, 16, 257)]:
                logs = [top] * n + ([below] * m if m else [])
                near = below is None or below >= top - 2
                for j in (range(64) if near else [(11 * i + 23 * k) % 64 for k in range(6)]):
                    yield (logs, *combos[j][0], combos[j][1])
                i += 1


def test_plan_constants_are_the_sources(exe):
    """The constants of tests/merkle_plan.py are those of the compiled header (merkle.hip asserts the header's restatements of
    common.h's at compile time)."""
    got = [int(x) for x in _library_lines(exe, ["C 0 0 0"])[0].split()]
    assert got == [MP.K_UP_LOG, MP.K_MAX_TREES, MP.K_MAX_HASH_COLS, MP.MERKLE_CAP, MP.MERKLE_PAIR_LOG], "update tests/merkle_plan.py"


def test_single_tree_plans_match_the_library(exe):
    """MP.steps is the tests' own statement of tstwo_merkle_commit's launches, written from the dispatch as it stood before
    csrc/merkle_plan.h existed; the header is the library's.  Over _tree_sweep the two give the same launches — kernel, layer,
    levels, grid, workgroup, columns, LayerParams, fold and hook — and refuse the same inputs with the same text."""
    inputs = list(_tree_sweep())
    got = _library_lines(exe, [_tree_line(*i) for i in inputs])
    refused = set()
    for i, line in zip(inputs, got):
        assert line == _own(MP.steps, *i), i
        if line.startswith("error: "):
            refused.add(line[7:])
    assert refused == {"merkle: layers must be 16-byte aligned", MP.FOLD_ERROR}
    logs = [[32], [5, 32, 5], [31] * 4 + [40]]
    assert _library_lines(exe, [_tree_line(l, False, False, True, True, MP.Env()) for l in logs]) == ["error: merkle: log size out of range"] * 3
    assert all(_own(MP.steps, l) == "error: merkle: log size out of range" for l in logs)
    # an empty tree is one launch of k_merkle_layer<false> over an empty message
    assert _library_lines(exe, [_tree_line([], False, True, True, True, MP.Env())]) == [_own(MP.steps, [], False, True)] \
        == ["layer<F>x1(0,0)[t0,1x1,256,c0+0,lp0:0:17:0:0:0:1] channel()[t0,1x1,64]"]


def test_layer_plans_match_the_library(exe):
    """tstwo_merkle_commit_layer: log 0..32 x children or none x column counts around every threshold x alignment x compute units."""
    inputs = [(log, prev, n, a16, env) for log in range(33) for prev in (False, True) for n in (0,) + TOP_COUNTS + (272, 300, 1100)
              for a16 in (False, True) for env in ENVS]
    got = _library_lines(exe, [f"L {_env(env)} {log} {int(prev)} {n} {int(a16)}" for log, prev, n, a16, env in inputs])
    for i, line in zip(inputs, got):
        assert line == _own(MP.layer_steps, *i), i
    assert {l for l in got if l.startswith("error")} == {"error: merkle: log size out of range", "error: merkle: layers must be 16-byte aligned"}


def _set_sweep():
    """1..9 trees x 16 / 32 / 48 / 64 / 80 columns x log 15..31, aligned, with one tree's columns or one tree's layers unaligned;
    then the same sets with one tree of another shape (other column count, other log size, one column of another log size), in
    the first, a middle and the last place, and with a null argument in the first or the last request."""
    for n, c, lg in itertools.product(range(1, 10), (16, 32, 48, 64, 80), range(15, 32)):
        base = [MP.Tree((lg,) * c)] * n
        yield base
        yield base[:-1] + [MP.Tree((lg,) * c, aligned8=False)]
        yield [MP.Tree((lg,) * c, aligned16=False)] + base[1:]
        for odd in (MP.Tree((lg,) * 16 if c != 16 else (lg,) * 32), MP.Tree((lg - 1,) * c), MP.Tree((lg,) * (c - 1) + (lg - 3,)),
                    MP.Tree((lg,) * c, null_arg=True)):
            for at in {0, n // 2, n - 1}:
                yield base[:at] + [odd] + base[at + 1:]


def test_tree_set_plans_match_the_library(exe):
    """tstwo_merkle_commit_many: the uniformity rule, the shared launches of a uniform set and the tree-by-tree plan of any other."""
    inputs = [(trees, env) for trees in _set_sweep() for env in ENVS]
    got = _library_lines(exe, [_set_line(*i) for i in inputs])
    shared = fallback = 0
    for i, line in zip(inputs, got):
        assert line == _own(MP.set_steps, *i), i
        shared += "x2," in line or "x8," in line
        fallback += " t1," in line.replace("[", " ")
    assert shared and fallback and {l for l in got if l.startswith("error")} == {"error: merkle: null argument",
                                                                                           "error: merkle: layers must be 16-byte aligned"}
    assert _library_lines(exe, ["S 256 32 19"]) == [""] == [_own(MP.set_steps, [])]


def test_stale_statements_are_gone():
    """What the tests' statement said before it was checked against the library: sixteen columns at log 19 take the pair kernel, and
    commit_many has a statement."""
    assert MP.plan([19] * 16)[0] == "pair16(19)" and MP.plan([18] * 16)[0] == "static16(18)"
    assert MP.plan(MP.MATRIX["32x19+2x12"]) == ["pair32(19)", "s2c(18)", "D(16,3)", "layer<T>x1(12,2)", "A(12)", "B(3,3)"]
    assert [str(l) for l in MP.set_steps([MP.Tree((22,) * 32)] * 8)] == ["pair32(22)", "s2c(21)", "s2c(19)", "inner_set(16)", "A(16)", "B(7,7)"]


@pytest.mark.parametrize("name", list(MP.EXPECTED))
def test_named_shapes_take_the_launches_they_were_chosen_for(name):
    assert MP.plan(MP.MATRIX[name]) == MP.EXPECTED[name]


def test_layer_launch_splits():
    """The column split of a layer's generic path: at most kMaxHashCols per launch, every launch but the last ends on a 64-byte block."""
    assert MP.layer_launches(256, True) == [256] and MP.layer_launches(257, True) == [256, 1]
    assert MP.layer_launches(513, True) == [256, 256, 1] and MP.layer_launches(513, False) == [256, 256, 1]
    assert MP.layer_launches(0, False) == [0] and MP.layer_launches(300, False) == [256, 44]
    for prev in (False, True):
        for n in range(0, 1100):
            takes, words = MP.layer_launches(n, prev), 16 if prev else 0
            assert sum(takes) == n and all(0 < t <= MP.K_MAX_HASH_COLS for t in takes[:-1])
            for t in takes[:-1]:
                words += t
                assert words % 16 == 0


def _kind(l):
    k = re.sub(r"x(\d+)$", lambda m: "x1" if m.group(1) == "1" else "x≥2", l.kind)
    if k in "ABCD":
        k += " stop=0" if l.stop == 0 else " stop>0"
    return k


def test_matrix_reaches_every_launch_kind():
    """The coverage condition: over the matrix, plan() names every launch kind the dispatch can make.  A condition on the
    shapes (through the plan model, which test_single_tree_plans_match_the_library ties to the library), not a measurement of
    what ran.  The pair kinds may also come from the commits of tests/test_gpu_merkle_pair.py (its child forces the pair kernel
    at small sizes); the launches a uniform commit_many shares among its trees come from that file and the grid-stride test."""
    all_launches = [l for logs in MP.MATRIX.values() for l in MP.launches(logs)]
    seen = {_kind(l) for l in all_launches}
    others = [l for env, trees in MP.gpu_test_commits() for l in MP.set_steps(trees, env)]
    seen |= {l.kind for l in others if l.kind.startswith("pair")}
    assert {l.kind for l in all_launches if l.kind.startswith("pair")} == {"pair16", "pair32"}           # on the shipped library
    shared = {re.sub(r"\d+$", "", l.kind) for l in others if l.trees > 1}
    assert shared == {"static", "pair", "s2c", "inner_set", "A", "B"}, "the launches a uniform set can share (its tail always starts at 2^16 children)"
    want = {"static16", "static32", "static48", "static64", "pair16", "pair32", "pair48", "pair64", "leaf4", "layer<F>x1", "layer<F>x≥2",
            "layer<T>x1", "layer<T>x≥2", "s2c", "inner_set", "leaf4_upq<1024>", "leaf4_upq<256>"}
    want |= {f"{arm} stop{s}" for arm in "ABC" for s in ("=0", ">0")} | {"D stop>0"}      # D with stop = 0: see the next test
    assert want - seen == set(), f"not reached: {sorted(want - seen)}"
    assert seen - want == set(), f"kinds the condition does not know: {sorted(seen - want)}"
    for t in "TF":
        aligned = [l for l in all_launches if l.kind.startswith(f"layer<{t}>") and l.words and l.words % 16 == 0]
        assert aligned, f"no layer<{t}> whose message ends on a 64-byte block"
        assert any(l.kind.endswith("x1") for l in aligned) and any(not l.kind.endswith("x1") for l in aligned), t


def test_arm_D_cannot_run_with_stop_zero():
    """Arm D (>= 512 parents, 64-quad workgroups, not the last launch) needs more than 16 levels left when log_stop is 0, and no
    caller enters those levels above 2^kUpLog children: the column-free run has peeled the layers down to it, the
    4-column path enters at log - 7 <= 9.  So "D with stop = 0" is not a launch the matrix could hold; every entry state says so."""
    for log_child in range(0, 32):                       # a column-free run down to the root, as a tree and a tree set enter it
        assert not [l for l in MP._column_free(log_child, 0) if l.kind == "D"]
    for log in range(10, MP.K_UP_LOG + 1):               # the 4-column path
        assert not [l for l in MP.launches([log] * 4) if l.kind == "D"]


def test_wrap_shapes_on_256_cus():
    """layer_blocks as the plan model states it: on 256 CUs a lane takes a second node from 2^22 nodes up; three, five, six or
    seven trees in one launch leave a partial last row."""
    assert MP.layer_blocks(1 << 21, 1, 256) == (8192, 8192) and MP.layer_blocks(1 << 22, 1, 256) == (8192, 16384)
    assert MP.layer_blocks(1 << 19, 5, 256) == (1638, 2048) and MP.layer_blocks(1 << 20, 3, 256) == (2730, 4096)
    assert MP.layer_blocks(1 << 18, 1, 256, 3) == (768, 1024) and MP.layer_blocks(1 << 17, 5, 256, 3) == (153, 512)
    assert MP.layer_blocks(1 << 16, 5, 256, 3) == (153, 256)

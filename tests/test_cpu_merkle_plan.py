"""The Merkle launch-plan matrix without a GPU: the hashlib model against the oracle, the plan model's constants against the
source, the launches the named shapes were chosen for, and the coverage condition on the matrix (tests/merkle_plan.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rand_column
from oracle import oracle as orc

import merkle_plan as MP

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


def test_plan_constants_are_the_sources():
    def const(path, pattern):
        with open(os.path.join(CSRC, path)) as f:
            m = re.findall(pattern, f.read())
        assert len(m) == 1, f"{path}: {pattern!r} found {len(m)} times: update tests/merkle_plan.py"
        return int(m[0])
    got = dict(K_UP_LOG=const("merkle.hip", r"constexpr int kUpLog = (\d+);"),
               K_MAX_TREES=const("merkle.hip", r"constexpr int kMaxTrees = (\d+);"),
               K_MAX_HASH_COLS=const("common.h", r"constexpr int kMaxHashCols = (\d+);"),
               MERKLE_CAP=const("common.h", r"int merkle_cap = (\d+);"))
    want = {k: getattr(MP, k) for k in got}
    assert got == want, "the dispatch constants changed: update tests/merkle_plan.py"


@pytest.mark.parametrize("name", list(MP.EXPECTED))
def test_named_shapes_take_the_launches_they_were_chosen_for(name):
    assert MP.plan(MP.MATRIX[name]) == MP.EXPECTED[name]


def test_layer_launch_splits():
    """commit_layer's column split: at most kMaxHashCols per launch, every launch but the last ends on a 64-byte block."""
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
    shapes (through a reading of the dispatch), not a measurement of what ran."""
    all_launches = [l for logs in MP.MATRIX.values() for l in MP.launches(logs)]
    seen = {_kind(l) for l in all_launches}
    want = {"static16", "static32", "static48", "static64", "leaf4", "layer<F>x1", "layer<F>x≥2", "layer<T>x1", "layer<T>x≥2", "s2c",
            "inner_set", "leaf4_upq<1024>", "leaf4_upq<256>"}
    want |= {f"{arm} stop{s}" for arm in "ABC" for s in ("=0", ">0")} | {"D stop>0"}      # D with stop = 0: see the next test
    assert want - seen == set(), f"not reached: {sorted(want - seen)}"
    assert seen - want == set(), f"kinds the condition does not know: {sorted(seen - want)}"
    for t in "TF":
        aligned = [l for l in all_launches if l.kind.startswith(f"layer<{t}>") and l.words and l.words % 16 == 0]
        assert aligned, f"no layer<{t}> whose message ends on a 64-byte block"
        assert any(l.kind.endswith("x1") for l in aligned) and any(not l.kind.endswith("x1") for l in aligned), t


def test_arm_D_cannot_run_with_stop_zero():
    """Arm D (>= 512 parents, 64-quad workgroups, not the last launch) needs more than 16 levels left when log_stop is 0, and no
    caller enters commit_upper_levels above 2^kUpLog children: commit_column_free has peeled the layers down to it, the
    4-column path enters at log - 7 <= 9.  So "D with stop = 0" is not a launch the matrix could hold; every entry state says so."""
    for log_child in range(0, 32):                       # commit_column_free(log_child, 0), as commit_tree and commit_many call it
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

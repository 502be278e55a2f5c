"""CPU tests of tests/arena.py (the guarded arena of test_gpu_bounds.py), so that the helper itself cannot pass silently:
the layout's alignment and guard widths, and check_image() on numpy images with single changed words."""
import numpy as np
import pytest

import arena as A


def _regions(off_a=0, off_b=0, off_c=0):
    return [A.rin("a", np.arange(5, dtype=np.uint32), off_a), A.rout("b", 1027, off_b),
            A.rinout("c", np.arange(3, dtype=np.uint32), off_c), A.Region("d", "out", nbytes=32)]


@pytest.mark.parametrize("offs", [(0, 0, 0), (4, 4, 4), (0, 4, 0), (4, 0, 0), (8, 12, 4), (12, 0, 8)])
def test_layout_alignment_and_guards(offs):
    lay = A.Layout(_regions(*offs))
    prev_end = 0
    for r, off in zip(lay.regions, list(offs) + [0]):
        s = lay.start[r.name]
        assert s % 16 == off
        assert s - prev_end >= A.GUARD
        prev_end = s + r.nbytes
    assert lay.total - prev_end >= A.GUARD and lay.total % 16 == 0
    # the guard ranges and the payloads tile the arena exactly, in order
    spans = sorted([(lo, hi) for lo, hi, _, _ in lay.guards()] + [(lay.start[r.name], lay.end(r.name)) for r in lay.regions])
    pos = 0
    for lo, hi in spans:
        assert lo == pos
        pos = hi
    assert pos == lay.total


def test_image_holds_sentinel_outside_uploaded_payloads():
    lay = A.Layout(_regions(4, 0, 4))
    img = lay.image()
    words = img[:lay.start["a"] - 4].view(np.uint32)
    assert (words == A.SENTINEL).all() and A.SENTINEL > 2**31 - 1
    s = lay.start["a"]
    assert (img[s:s + 20].view(np.uint32) == np.arange(5)).all()
    s = lay.start["b"]
    assert (img[s:s + 4 * 1027] == A.SENTINEL_BYTE).all()          # an output not uploaded
    mask = np.ones(lay.total, dtype=bool)
    for r in lay.regions:
        if r.data is not None:
            mask[lay.start[r.name]:lay.end(r.name)] = False
    assert (img[mask] == A.SENTINEL_BYTE).all()


def test_untouched_image_reports_nothing_and_returns_payloads():
    lay = A.Layout(_regions(0, 4, 0))
    before = lay.image()
    after = before.copy()
    s = lay.start["b"]
    after[s:s + 4 * 1027] = np.arange(1027, dtype=np.uint32).view(np.uint8)
    assert A.find_violations(lay, before, after) == []
    got = A.check_image(lay, before, after)
    assert sorted(got) == ["b", "c", "d"]
    assert (got["b"] == np.arange(1027)).all() and (got["c"] == np.arange(3)).all()
    assert (got["d"] == A.SENTINEL).all() and got["d"].size == 8


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("side,which", [("before", "first"), ("before", "last"), ("after", "first"), ("after", "last")])
def test_changed_guard_word_is_reported(name, side, which):
    """One changed word at the first and at the last word of either guard of every region (first, middle, last)."""
    lay = A.Layout(_regions(0, 4, 4))
    before = lay.image()
    lo, hi = next((lo, hi) for lo, hi, r, s in lay.guards() if r.name == name and s == side)
    assert hi - lo >= A.GUARD // 2
    at = lo if which == "first" else hi - 4
    after = before.copy()
    after[at:at + 4] = np.array([7], dtype=np.uint32).view(np.uint8)
    msgs = A.find_violations(lay, before, after)
    assert len(msgs) == 1
    rel = at - lay.start[name]
    assert f"guard {side} region '{name}'" in msgs[0]
    assert f"first changed byte at {rel:+d}, last at {rel + 3:+d}" in msgs[0]
    with pytest.raises(AssertionError, match=f"guard {side} region '{name}'"):
        A.check_image(lay, before, after)


def test_word_adjacent_to_a_payload_is_a_guard_word():
    """The word right after an output's last word and the word right before its first are guard, at an offset placement."""
    lay = A.Layout(_regions(0, 4, 0))
    before = lay.image()
    for at, side in ((lay.end("b"), "after"), (lay.start["b"] - 4, "before")):
        after = before.copy()
        after[at] ^= 1
        msgs = A.find_violations(lay, before, after)
        assert len(msgs) == 1 and f"guard {side} region 'b'" in msgs[0]


@pytest.mark.parametrize("word", [0, 4])
def test_changed_input_word_is_reported(word):
    lay = A.Layout(_regions(4, 0, 0))
    before = lay.image()
    after = before.copy()
    s = lay.start["a"] + 4 * word
    after[s:s + 4] = np.array([123456], dtype=np.uint32).view(np.uint8)
    msgs = A.find_violations(lay, before, after)
    assert len(msgs) == 1 and "input region 'a'" in msgs[0] and f"first changed byte at {4 * word:+d}" in msgs[0]
    with pytest.raises(AssertionError, match="input region 'a'"):
        A.check_image(lay, before, after)


def test_inout_and_out_changes_are_not_violations():
    lay = A.Layout(_regions())
    before = lay.image()
    after = before.copy()
    for name in ("b", "c", "d"):
        after[lay.start[name]:lay.end(name)] = 0
    assert A.find_violations(lay, before, after) == []


def test_region_rules():
    with pytest.raises(AssertionError):
        A.Region("x", "in", nbytes=16)                 # an input must carry data
    with pytest.raises(AssertionError):
        A.Region("x", "out", nbytes=16, offset=2)      # placements are 0, 4, 8, 12
    with pytest.raises(AssertionError):
        A.Layout([A.rout("x", 1), A.rout("x", 1)])
    lay = A.Layout([A.rout("empty", 0), A.rout("y", 1)])
    assert lay.start["y"] - lay.end("empty") >= A.GUARD

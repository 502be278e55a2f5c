"""The steered messages of tests/poseidon_steer.py on the MI355X: operands of Hades round 0 at the carry, borrow and digit edges of
csrc/felt252.cuh (one lane per hash) and csrc/felt252_coop.cuh (eight lanes per hash), through every entry that takes such a
message: hash_many, commit_layer with a caller's children, and the device channel.  tests/test_cpu_poseidon_steer.py proves on
the CPU that the cases reach those operands and holds CASE_NAMES to the steering module's list.

Every output lies inside guard bands (tests/arena.py) and is compared word for word with the integer model
(tests/poseidon_model.py); nothing here is compared with a limb model."""
import ctypes as C
import functools

import numpy as np
import pytest

import poseidon_model as M
import poseidon_steer as S
from arena import SENTINEL, Arena, rin, rinout, rout
from tstwo_amd import _lib as L

pytestmark = pytest.mark.gpu

M31_P = 2**31 - 1
CASES = list(S.CASES)
CASE_NAMES = [c.name for c in CASES]
HASH_ENTRIES = ("tstwo_poseidon252_hash_many_coop", "tstwo_poseidon252_hash_many")
LAYER_ENTRIES = ("tstwo_poseidon252_merkle_commit_layer_coop", "tstwo_poseidon252_merkle_commit_layer")
FILLER = [M.hash_many([252, 1]), M.hash_many([252, 2])]          # a message with nothing special about it


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


@functools.lru_cache(maxsize=None)
def _model_hash(msg):
    return M.hash_many(list(msg))


def _words(msgs):
    return np.array([[w for x in m for w in M.to_words(x)] for m in msgs], dtype=np.uint32).reshape(-1)


def _felts(words):
    return [M.from_words([int(w) for w in r]) for r in np.asarray(words).reshape(-1, 8)]


def _hash_many(entry, msgs):
    n, k = len(msgs), len(msgs[0])
    with Arena([rin("in", _words(msgs)), rout("out", 8 * n)]) as a:
        L.call(entry, a.ptr("in"), n, k, a.ptr("out"))
        return a.check()["out"]


def _check_hash_many(msgs, names, entries=HASH_ENTRIES):
    want = [_model_hash(tuple(m)) for m in msgs]
    outs = [_hash_many(e, msgs) for e in entries]
    for e, out in zip(entries, outs):
        bad = [names[i] for i, (g, w) in enumerate(zip(_felts(out), want)) if g != w]
        assert not bad, (e, bad)
    assert all((o == outs[0]).all() for o in outs)


# ---------------------------------------------------------------- hash_many
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hash_many_steered(k):
    """every case at k = 2, the x-only ones at k = 1 (the appended 1 is the second element), the later-absorb ones at their own k"""
    if k == 2:
        cases, msgs = CASES, [list(c.xy) for c in CASES]
    elif k == 1:
        cases = [c for c in CASES if c.kind == "msg" and c.x_only]
        msgs = [[c.msg[0]] for c in cases]
    else:
        cases = [c for c in CASES if c.kind == "msg" and len(c.msg) == k]
        msgs = [list(c.msg) for c in cases]
    assert len(cases) >= 20
    _check_hash_many(msgs, [c.name for c in cases])


def _group_local():
    return [c for c in CASES if c.group_local and c.kind == "msg" and len(c.msg) == 2]


def test_coop_wave_placement():
    """a case whose carries must stay inside its 8 lanes, at each of the 8 group slots of a wave: beside a filler with the
    neighbour case (whose same instruction carries out of limb 7) in the group below it, in the group above it, a wave of
    neighbours around it, and a whole wave of the case.  A wave is 8 consecutive messages."""
    msgs, names = [], []
    for v in _group_local():
        nb = S.BY_NAME[v.neighbour]
        waves = [[v.msg] * 8]
        for slot in range(8):
            below, above, both = [FILLER] * 8, [FILLER] * 8, [nb.msg] * 8
            below[slot] = above[slot] = both[slot] = v.msg
            if slot > 0:
                below[slot - 1] = nb.msg
            if slot < 7:
                above[slot + 1] = nb.msg
            waves += [below, above, both]
        for w, wave in enumerate(waves):
            msgs += [list(m) for m in wave]
            names += [f"{v.name} wave {w} slot {s}" for s in range(8)]
    assert len(msgs) % 8 == 0 and 1000 < len(msgs) < 5000
    _check_hash_many(msgs, names)


def test_coop_tail_groups_clamped_onto_a_case():
    """launches whose last live group is the case and whose 1 to 7 tail groups of that wave hash it again"""
    for v in _group_local():
        nb = S.BY_NAME[v.neighbour]
        for tail in range(1, 8):
            msgs = [list(nb.msg)] * (7 - tail) + [list(v.msg)]
            _check_hash_many(msgs, [f"{v.name} tail {tail} message {i}" for i in range(len(msgs))], entries=HASH_ENTRIES[:1])


# ---------------------------------------------------------------- commit_layer
def _layer(entry, log, prev_words, cols):
    n = 1 << log
    regions = [rin(f"c{i}", c) for i, c in enumerate(cols)]
    if prev_words is not None:
        regions.append(rin("prev", prev_words))
    with Arena(regions + [rout("out", 8 * n)]) as a:
        L.call(entry, log, a.ptr("prev") if prev_words is not None else C.c_void_p(0), a.ptrs([f"c{i}" for i in range(len(cols))]),
               len(cols), a.ptr("out"))
        return a.check()["out"]


@pytest.mark.parametrize("n_cols", [0, 8, 9])
def test_commit_layer_children_are_the_cases(n_cols):
    """node i's children are case i's pair; with columns the second absorb is [block, 1] or [block, block']"""
    log = 8
    n = 1 << log
    assert n >= len(CASES)
    pairs = [CASES[i % len(CASES)].xy for i in range(n)]
    prev_words = _words([[v for p in pairs for v in p]])
    rng = np.random.default_rng(5200 + n_cols)
    cols = [rng.integers(0, M31_P, size=n, dtype=np.uint32) for _ in range(n_cols)]
    want = [M.hash_node(pairs[i], [int(c[i]) for c in cols]) for i in range(n)]
    for entry in LAYER_ENTRIES:
        got = _felts(_layer(entry, log, prev_words, cols))
        bad = [CASE_NAMES[i % len(CASES)] for i in range(n) if got[i] != want[i]]
        assert not bad, (entry, bad)


def _block_patterns(n_cols):
    """per node, the values of its n_cols columns: the largest M31 value everywhere, the two alternating bit patterns, and a
    single 1 in the first or the last column of each block of 8"""
    hi, a5, aa = M31_P - 1, 0x55555555 & M31_P, 0x2AAAAAAA
    rows = [[hi] * n_cols, [a5 if c % 2 == 0 else aa for c in range(n_cols)], [aa if c % 2 == 0 else a5 for c in range(n_cols)]]
    for b in range((n_cols + 7) // 8):
        for c in sorted({8 * b, min(8 * b + 7, n_cols - 1)}):
            rows.append([1 if k == c else 0 for k in range(n_cols)])
    return rows


@pytest.mark.parametrize("n_cols", [1, 7, 8, 9, 16, 17])
def test_commit_layer_column_blocks(n_cols):
    rows = _block_patterns(n_cols)
    log = 4
    n = 1 << log
    assert len(rows) <= n
    rows += [[0] * n_cols] * (n - len(rows))
    cols = [np.array([rows[i][c] for i in range(n)], dtype=np.uint32) for c in range(n_cols)]
    want = [M.hash_node(None, rows[i]) for i in range(n)]
    for entry in LAYER_ENTRIES:
        assert _felts(_layer(entry, log, None, cols)) == want, entry


# ---------------------------------------------------------------- the device channel
N_CHALLENGES = 5


def _channel_steps(states, roots, draw):
    """one call per state, all in one arena.  states: (digest, n_sent); roots: a root per state or None.  Returns per state the
    ten channel words and the four felt words (sentinel where nothing was drawn)."""
    regions = []
    for i, (d, n_sent) in enumerate(states):
        regions.append(rinout(f"chan{i}", np.array(M.to_words(d) + [N_CHALLENGES, n_sent], dtype=np.uint32)))
        if roots is not None:
            regions.append(rin(f"root{i}", np.array(M.to_words(roots[i]), dtype=np.uint32)))
        regions.append(rout(f"felt{i}", 4))
    with Arena(regions) as a:
        for i in range(len(states)):
            L.call("tstwo_poseidon252_channel_mix_root_draw_felt", a.ptr(f"chan{i}"), a.ptr(f"root{i}") if roots is not None else C.c_void_p(0),
                   a.ptr(f"felt{i}") if draw else C.c_void_p(0))
        out = a.check()
    return [(out[f"chan{i}"].tolist(), out[f"felt{i}"].tolist()) for i in range(len(states))]


def _channel_want(state, root, draw):
    m = M.Channel()
    m.digest, m.n_challenges, m.n_sent = state[0], N_CHALLENGES, state[1]
    if root is not None:
        m.mix_root(root)
    felt = list(m.draw_felt()) if draw else [SENTINEL] * 4
    return M.to_words(m.digest) + [m.n_challenges, m.n_sent], felt


def test_channel_mix_only():
    """digest and root are a case's pair: mix_root is hash_many([digest, root])"""
    states, roots = [(c.xy[0], 3) for c in CASES], [c.xy[1] for c in CASES]
    got = _channel_steps(states, roots, draw=False)
    bad = [c.name for c, g, s, r in zip(CASES, got, states, roots) if g != _channel_want(s, r, False)]
    assert not bad, bad


def test_channel_draw_only():
    """the channel-draw cases: Hades(digest, n_sent, 2) with no sponge add"""
    cases = [c for c in CASES if c.kind == "draw"]
    assert len(cases) >= 20
    states = [(c.digest, c.n_sent) for c in cases]
    got = _channel_steps(states, None, draw=True)
    bad = [c.name for c, g, s in zip(cases, got, states) if g != _channel_want(s, None, True)]
    assert not bad, bad


def test_channel_mix_and_draw_in_one_call():
    states, roots = [(c.xy[0], 3) for c in CASES], [c.xy[1] for c in CASES]
    got = _channel_steps(states, roots, draw=True)
    bad = [c.name for c, g, s, r in zip(CASES, got, states, roots) if g != _channel_want(s, r, True)]
    assert not bad, bad

"""Poseidon252 with 8 lanes per hash on the MI355X (csrc/poseidon_coop.hip): hash_many_coop and merkle_commit_layer_coop, word for
word against the independent model (tests/poseidon_model.py) where the case is small and against the lane-per-hash entries
everywhere, with every output inside guard bands (tests/arena.py).  The sizes hit the tails of a group (8 lanes), a wave (8
groups) and a workgroup (32 groups)."""
import ctypes as C

import numpy as np
import pytest

import poseidon_model as M
from arena import Arena, rin, rout
from tstwo_amd import _lib as L

pytestmark = pytest.mark.gpu

M31_P = 2**31 - 1
R = 2**256
N_MSGS = [1, 2, 7, 8, 9, 63, 64, 65, 513]
MODEL_MAX_MSGS = 65                      # x at most 3 permutations: well inside what the model does in a second
# limb patterns of tests/test_cpu_felt_coop.py.  As message elements they are only the b operand of to_mont(x) = mul(R^2, x); from the
# first round constant on every operand is pseudo-random (tests/test_gpu_poseidon_steer.py steers the operands of round 0)
EDGE = [0, 1, 2, M.P - 1, M.P - 2, 2**251 - 1, 2**251, 2**192 * 17, 2**192 * 17 + 1, R % M.P, R * R % M.P, 2**32 - 1, 2**32, 2**224,
        2**251 + 17 * 2**192, 2**251 + 2**192 - 1, 2**224 - 1, (2**27 - 1) << 224 | (2**224 - 1), 0xFFFFFFFF << 192, 0xFFFFFFFF00000000FFFFFFFF]


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def _words(msgs):
    return np.array([[w for x in m for w in M.to_words(x)] for m in msgs], dtype=np.uint32).reshape(-1)


def _felts(words):
    return [M.from_words([int(w) for w in r]) for r in np.asarray(words).reshape(-1, 8)]


def _hash_many_both(msgs, k):
    """(coop, lane-per-hash) outputs of the two entries on the same messages, the coop one inside guard bands"""
    n = len(msgs)
    src = _words(msgs) if k else np.zeros(8, dtype=np.uint32)
    with Arena([rin("in", src), rout("out", 8 * n)]) as a:
        L.call("tstwo_poseidon252_hash_many_coop", a.ptr("in"), n, k, a.ptr("out"))
        coop = a.check()["out"]
    with Arena([rin("in", src), rout("out", 8 * n)]) as a:
        L.call("tstwo_poseidon252_hash_many", a.ptr("in"), n, k, a.ptr("out"))
        old = a.check()["out"]
    return coop, old


@pytest.mark.parametrize("k", range(1, 6))
def test_hash_many_coop(k):
    rng = np.random.default_rng(4200 + k)
    for n in N_MSGS:
        msgs = [[EDGE[(5 * i + j) % len(EDGE)] if (i + j) % 4 == 0 else int.from_bytes(rng.bytes(32), "little") % M.P for j in range(k)]
                for i in range(n)]
        coop, old = _hash_many_both(msgs, k)
        assert (coop == old).all(), (k, n)
        if n <= MODEL_MAX_MSGS:
            assert _felts(coop) == [M.hash_many(m) for m in msgs], (k, n)


def test_hash_many_coop_edge_operands():
    """every edge operand alone, and every ordered pair of them, as a message"""
    singles = [[x] for x in EDGE]
    coop, old = _hash_many_both(singles, 1)
    assert _felts(coop) == [M.hash_many(m) for m in singles] and (coop == old).all()
    pairs = [[a, b] for a in EDGE for b in EDGE]
    coop, old = _hash_many_both(pairs, 2)
    assert (coop == old).all()
    assert _felts(coop)[::7] == [M.hash_many(m) for m in pairs[::7]]


def test_hash_many_coop_empty_messages_and_arguments():
    coop, old = _hash_many_both([[]] * 3, 0)
    assert _felts(coop) == [M.hash_many([])] * 3 and (coop == old).all()
    buf = L.DeviceBuffer(256)
    L.call("tstwo_poseidon252_hash_many_coop", C.c_void_p(0), 0, 1, C.c_void_p(0))              # nothing to do
    with pytest.raises(L.TstwoError, match="null device pointer"):
        L.call("tstwo_poseidon252_hash_many_coop", C.c_void_p(0), 1, 1, C.c_void_p(buf.ptr))
    with pytest.raises(L.TstwoError, match="16-byte aligned"):
        L.call("tstwo_poseidon252_hash_many_coop", C.c_void_p(buf.ptr + 4), 1, 1, C.c_void_p(buf.ptr + 128))
    with pytest.raises(L.TstwoError, match="batch too large"):
        L.call("tstwo_poseidon252_hash_many_coop", C.c_void_p(buf.ptr), 1, (1 << 20) + 1, C.c_void_p(buf.ptr + 128))


# ---------------------------------------------------------------- commit_layer
def _layer_both(log, prev_words, cols, offsets):
    n = 1 << log
    regions = [rin(f"c{i}", c, offset=o) for i, (c, o) in enumerate(zip(cols, offsets))]
    if prev_words is not None:
        regions.append(rin("prev", prev_words))
    out = []
    for entry in ("tstwo_poseidon252_merkle_commit_layer_coop", "tstwo_poseidon252_merkle_commit_layer"):
        with Arena(regions + [rout("out", 8 * n)]) as a:
            L.call(entry, log, a.ptr("prev") if prev_words is not None else C.c_void_p(0), a.ptrs([f"c{i}" for i in range(len(cols))]),
                   len(cols), a.ptr("out"))
            out.append(a.check()["out"])
    return out


@pytest.mark.parametrize("log", [0, 1, 2, 3, 6, 10])
def test_commit_layer_coop(log):
    rng = np.random.default_rng(4300 + log)
    n = 1 << log
    prev_felts = [int.from_bytes(rng.bytes(32), "little") % M.P for _ in range(2 * n)]
    prev_felts[0], prev_felts[-1] = M.P - 1, 0
    prev_words = _words([prev_felts])
    for n_cols in (0, 1, 4, 8, 9, 17):
        cols = [rng.integers(0, M31_P, size=n, dtype=np.uint32) for _ in range(n_cols)]
        for c in cols[::3]:
            c[0] = c[-1] = M31_P - 1
        offsets = [(4 * i) % 16 for i in range(n_cols)]                 # column pointers unaligned by 4, 8, 12 bytes
        for has_prev in (True, False):
            if n_cols == 0 and not has_prev and log > 3:
                continue                                                # hash_many([]) at every node: covered at the small sizes
            coop, old = _layer_both(log, prev_words if has_prev else None, cols, offsets)
            assert (coop == old).all(), (log, n_cols, has_prev)
            if log <= 6:
                want = [M.hash_node((prev_felts[2 * i], prev_felts[2 * i + 1]) if has_prev else None, [int(c[i]) for c in cols])
                        for i in range(n)]
                assert _felts(coop) == want, (log, n_cols, has_prev)


def test_commit_layer_coop_many_columns_and_arguments():
    """more columns than travel in the kernel argument (the device pointer table), and the argument checks of the old entry"""
    rng = np.random.default_rng(4400)
    cols = [rng.integers(0, M31_P, size=4, dtype=np.uint32) for _ in range(70)]
    coop, old = _layer_both(2, None, cols, [0] * 70)
    assert (coop == old).all()
    assert _felts(coop) == [M.hash_node(None, [int(c[i]) for c in cols]) for i in range(4)]
    buf = L.DeviceBuffer(256)
    with pytest.raises(L.TstwoError, match="null output layer"):
        L.call("tstwo_poseidon252_merkle_commit_layer_coop", 0, C.c_void_p(0), L.ptr_array([]), 0, C.c_void_p(0))
    with pytest.raises(L.TstwoError, match="16-byte aligned"):
        L.call("tstwo_poseidon252_merkle_commit_layer_coop", 0, C.c_void_p(0), L.ptr_array([]), 0, C.c_void_p(buf.ptr + 8))
    with pytest.raises(L.TstwoError, match="log size out of range"):
        L.call("tstwo_poseidon252_merkle_commit_layer_coop", 31, C.c_void_p(0), L.ptr_array([]), 0, C.c_void_p(buf.ptr))
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        L.call("tstwo_poseidon252_merkle_commit_layer_coop", 0, C.c_void_p(0), L.ptr_array([0]), 1, C.c_void_p(buf.ptr))

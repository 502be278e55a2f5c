"""Poseidon252Channel on the MI355X (tstwo_poseidon252_channel_mix_root_draw_felt, DevicePoseidon252Channel): the state words and
the drawn felts exactly, against the independent model (tests/poseidon_model.py: Channel) and the host Poseidon252Channel."""
import ctypes as C

import numpy as np
import pytest

import poseidon_model as M
import tstwo_amd as T
from tstwo_amd import _lib as L
from tstwo_amd.poseidon import DevicePoseidon252Channel, FieldElement252, Poseidon252Channel, Poseidon252MerkleProver

pytestmark = pytest.mark.gpu

M31_P = 2**31 - 1
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def _host(digest=0, n_challenges=0, n_sent=0):
    return Poseidon252Channel(FieldElement252(digest), n_challenges, n_sent)


def _model(digest=0, n_challenges=0, n_sent=0):
    m = M.Channel()
    m.digest, m.n_challenges, m.n_sent = digest, n_challenges, n_sent
    return m


def _state(m):
    return M.to_words(m.digest) + [m.n_challenges, m.n_sent]


class Rig:
    """a device channel, a root buffer and felt slots, all filled with a sentinel where nothing was uploaded"""

    def __init__(self, host, roots):
        self.dch = DevicePoseidon252Channel(host)
        self.roots = L.DeviceBuffer(32 * max(len(roots), 1))
        if roots:
            self.roots.upload(np.array([w for r in roots for w in M.to_words(r)], dtype=np.uint32))
        self.felts = L.DeviceBuffer(16 * 8)
        self.felts.upload(np.full(32, SENTINEL, dtype=np.uint32))

    def step(self, root_index, felt_slot):
        self.dch.mix_root_draw_felt(None if root_index is None else self.roots.ptr + 32 * root_index,
                                    None if felt_slot is None else self.felts.ptr + 16 * felt_slot)

    def state(self):
        return self.dch.buf.download(count=10).tolist()

    def felt(self, slot):
        return tuple(self.felts.download(count=32)[4 * slot:4 * slot + 4].tolist())


START = dict(digest=M.hash_many([3, 4]), n_challenges=5, n_sent=3)
ROOTS = [M.hash_many([7]), M.P - 1, 0, 1, M.hash_many([9, 9, 9])]


def test_mix_only():
    rig, m, h = Rig(_host(**START), ROOTS), _model(**START), _host(**START)
    rig.step(1, None)
    m.mix_root(ROOTS[1])
    h.mix_root(FieldElement252(ROOTS[1]))
    assert rig.state() == _state(m) == h.digest().to_words() + [h.n_challenges, h.n_sent]
    assert rig.felt(0) == (SENTINEL,) * 4                      # nothing drawn, nothing written


def test_draw_only_and_two_draws_without_a_mix():
    rig, m, h = Rig(_host(**START), []), _model(**START), _host(**START)
    for k in range(2):                                         # n_sent 3 -> 4 -> 5
        rig.step(None, k)
        want = m.draw_felt()
        assert rig.felt(k) == want == h.draw_felt().tup()
        assert rig.state() == _state(m)
    fresh, mf = Rig(_host(), []), _model()                     # the all-zero channel: n_sent 0 -> 1 -> 2
    for k in range(2):
        fresh.step(None, k)
        assert fresh.felt(k) == mf.draw_felt()
    assert fresh.state() == _state(mf) and mf.n_sent == 2


def test_mix_and_draw_chain_of_five():
    rig, m, h = Rig(_host(), ROOTS), _model(), _host()
    for k, r in enumerate(ROOTS):
        rig.step(k, k)
        m.mix_root(r)
        h.mix_root(FieldElement252(r))
        want = m.draw_felt()
        assert h.draw_felt().tup() == want
        assert rig.felt(k) == want, k
        assert all(w < M31_P for w in want)
    assert rig.state() == _state(m) and m.n_challenges == 5 and m.n_sent == 1
    assert rig.dch.sync_to_host().digest().toBigInt() == m.digest


def test_root_from_byte_0_of_a_tree():
    rng = np.random.default_rng(4500)
    cols = [rng.integers(0, M31_P, size=1 << 4, dtype=np.uint32) for _ in range(5)]
    tree = Poseidon252MerkleProver.commit([T.HipColumn(c) for c in cols])
    root = M.commit([c.tolist() for c in cols])[0][0]
    assert tree.root().toBigInt() == root
    rig, m = Rig(_host(**START), []), _model(**START)
    rig.dch.mix_root_draw_felt(tree.root_ptr(), rig.felts.ptr)
    m.mix_root(root)
    assert rig.felt(0) == m.draw_felt() and rig.state() == _state(m)


def test_load_and_sync_to_host():
    host = _host(digest=M.P - 1, n_challenges=0xFFFFFFFE, n_sent=7)
    dch = DevicePoseidon252Channel(host)
    assert dch.buf.download(count=10).tolist() == M.to_words(M.P - 1) + [0xFFFFFFFE, 7]
    felt = L.DeviceBuffer(16)
    dch.mix_root_draw_felt(None, felt.ptr)
    m = _model(digest=M.P - 1, n_challenges=0xFFFFFFFE, n_sent=7)
    want = m.draw_felt()
    assert tuple(felt.download(count=4).tolist()) == want
    back = dch.sync_to_host()
    assert back is host and (host.digest().toBigInt(), host.n_challenges, host.n_sent) == (M.P - 1, 0xFFFFFFFE, 8)
    other = _host(digest=5, n_challenges=1, n_sent=0)
    big = DevicePoseidon252Channel(host, buf=L.DeviceBuffer(128))        # the owner of a larger buffer keeps words behind the state
    big.load(other, tail=[11, 12])
    got = big.buf.download(count=18).tolist()
    assert got[:10] == M.to_words(5) + [1, 0] and got[16:] == [11, 12]
    with pytest.raises(TypeError):
        DevicePoseidon252Channel(T.Blake2sChannel())


def test_arguments():
    chan = L.DeviceBuffer(64)
    chan.upload(np.arange(16, dtype=np.uint32))
    call = lambda c, r, f: L.call("tstwo_poseidon252_channel_mix_root_draw_felt", C.c_void_p(c), C.c_void_p(r), C.c_void_p(f))
    with pytest.raises(L.TstwoError, match="null device pointer"):
        call(0, chan.ptr + 64 - 32, 0)
    with pytest.raises(L.TstwoError, match="unaligned pointer"):
        call(chan.ptr, chan.ptr + 2, 0)
    with pytest.raises(L.TstwoError, match="unaligned pointer"):
        call(chan.ptr, 0, chan.ptr + 41)
    assert chan.download(count=16).tolist() == list(range(16))           # a refused call wrote nothing

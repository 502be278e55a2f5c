"""FriProver.commit over Poseidon252 in one library call (tstwo_fri_commit_layers_poseidon252, the Poseidon device channel) against
the host-transcript commit (device_channel=False) on the same inputs: every tree, evaluation, alpha, the channel state, the last
layer's polynomial and the decommitted proof are identical, and FriVerifier accepts.  Shapes: tests/fri_poseidon_shapes.py."""
import ctypes as C
import os

import numpy as np
import pytest

import poseidon_model as M
import sequence as Q
import tstwo_amd as T
from fri_poseidon_shapes import LOG_BLOWUP, MODEL_SHAPES, SHAPES, last_log
from tstwo_amd import _lib as L
from tstwo_amd.poseidon import DevicePoseidon252Channel, Poseidon252Channel

pytestmark = pytest.mark.gpu

M31_P = 2**31 - 1
PMC = T.Poseidon252MerkleChannel
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


_cache = {}


def _inputs(col_logs):
    """low-degree circle evaluations of the given log sizes over one twiddle tree; computed once per shape and left unchanged"""
    key = tuple(col_logs)
    if key not in _cache:
        tw = T.precompute_twiddles(T.CanonicCoset(col_logs[0]).circleDomain().halfCoset)
        cols = []
        for c in col_logs:
            domain = T.CanonicCoset(c).circleDomain()
            rng = np.random.default_rng(4600 + c)
            polys = [T.HipCirclePoly(T.HipColumn(rng.integers(0, M31_P, size=1 << (c - LOG_BLOWUP), dtype=np.uint32))) for _ in range(4)]
            evs = T.evaluate_polynomials(polys, domain, tw)
            cols.append(T.SecureEvaluation(domain, T.SecureColumnByCoords([e.values for e in evs])))
        _cache[key] = (cols, tw)
    return _cache[key]


def _start_channel():
    ch = Poseidon252Channel()
    ch.mix_u64(0x1234)
    ch.draw_felt()                                  # nonzero n_challenges and n_sent at the start
    return ch


def _tree_words(tree):
    return np.concatenate([tree.layers[k].to_numpy().reshape(-1) for k in range(len(tree.layers))])


def _state(ch):
    return (ch.digest().toBigInt(), ch.n_challenges, ch.n_sent)


@pytest.mark.parametrize("col_logs,bound", SHAPES, ids=lambda v: str(v))
def test_one_call_commit_matches_host_transcript(col_logs, bound):
    cols, tw = _inputs(col_logs)
    cfg = T.FriConfig(bound, LOG_BLOWUP, 6)
    ch_d, ch_h = _start_channel(), _start_channel()
    d = T.FriProver.commit(ch_d, cfg, cols, tw, device_channel=True, merkle_channel=PMC)
    h = T.FriProver.commit(ch_h, cfg, cols, tw, device_channel=False, merkle_channel=PMC)
    assert type(d.first_layer.merkle_tree) is type(h.first_layer.merkle_tree) is T.Poseidon252MerkleProver
    assert (_tree_words(d.first_layer.merkle_tree) == _tree_words(h.first_layer.merkle_tree)).all()
    assert len(d.inner_layers) == len(h.inner_layers) == col_logs[0] - 1 - last_log(bound)
    for ld, lh in zip(d.inner_layers, h.inner_layers):
        assert ld.evaluation.domain().logSize() == lh.evaluation.domain().logSize()
        for cd, chh in zip(ld.evaluation.values.to_numpy(), lh.evaluation.values.to_numpy()):
            assert (cd == chh).all()
        assert (_tree_words(ld.merkle_tree) == _tree_words(lh.merkle_tree)).all()
    assert [c.tup() for c in d.last_layer_poly.coeffs] == [c.tup() for c in h.last_layer_poly.coeffs]
    assert _state(ch_d) == _state(ch_h)
    if (col_logs, bound) in MODEL_SHAPES:
        first_cols = [cc.to_numpy().tolist() for c in cols for cc in c.values.columns]
        assert d.first_layer.merkle_tree.root().toBigInt() == M.commit(first_cols)[0][0]
        for layer in d.inner_layers:
            lc = [c.to_numpy().tolist() for c in layer.evaluation.values.columns]
            assert layer.merkle_tree.root().toBigInt() == M.commit(lc)[0][0]
    proof_d, pos_d = d.decommit(ch_d)
    proof_h, pos_h = h.decommit(ch_h)
    assert pos_d == pos_h and _state(ch_d) == _state(ch_h)
    for a, b in zip([proof_d.first_layer] + list(proof_d.inner_layers), [proof_h.first_layer] + list(proof_h.inner_layers)):
        assert a.commitment == b.commitment
        assert [x.tup() for x in a.fri_witness] == [x.tup() for x in b.fri_witness]
        assert list(a.decommitment.hashWitness) == list(b.decommitment.hashWitness)
        assert [v.value for v in a.decommitment.columnWitness] == [v.value for v in b.decommitment.columnWitness]
    assert [c.tup() for c in proof_d.last_layer_poly.coeffs] == [c.tup() for c in proof_h.last_layer_poly.coeffs]
    vch = _start_channel()
    v = T.FriVerifier.commit(vch, cfg, proof_d, [T.CirclePolyDegreeBound(c - LOG_BLOWUP) for c in col_logs], merkle_channel=PMC)
    assert v.sample_query_positions(vch) == pos_d
    v.decommit([c.values.gather(pos_d[c.domain.logSize()]) for c in cols])
    assert _state(vch) == _state(ch_d)


def test_default_is_the_measured_one_and_both_paths_are_reachable():
    """device_channel=None takes fri_prover.POSEIDON252_DEVICE_TRANSCRIPT; True and False give the same commit either way"""
    from tstwo_amd import fri_prover
    cols, tw = _inputs([5])
    cfg = T.FriConfig(0, LOG_BLOWUP, 3)
    states = []
    for dc in (None, True, False):
        ch = _start_channel()
        T.FriProver.commit(ch, cfg, cols, tw, device_channel=dc, merkle_channel=PMC)
        states.append(_state(ch))
    assert states[0] == states[1] == states[2]
    assert isinstance(fri_prover.POSEIDON252_DEVICE_TRANSCRIPT, bool)


# ---------------------------------------------------------------- the C entry itself
class Raw:
    """one raw call: the arguments of tstwo_fri_commit_layers_poseidon252 for a shape, over a given channel and alpha buffer"""

    def __init__(self, col_logs, bound, chan_ptr, alphas_ptr, alphas_cap):
        self.col_logs, self.last = col_logs, last_log(bound)
        self.cols, self.tw = _inputs(col_logs)
        self.cap = col_logs[0] - 1 - self.last + 1
        self.outs, self.n_out, self.first = (L.FriLayerOut * max(self.cap, 1))(), C.c_size_t(0), L.vp()
        self.chan_ptr, self.alphas_ptr, self.alphas_cap = chan_ptr, alphas_ptr, alphas_cap

    def call(self):
        L.call("tstwo_fri_commit_layers_poseidon252", L.ptr_array([cc.ptr for c in self.cols for cc in c.values.columns]), L.u32x(self.col_logs),
               len(self.col_logs), C.c_void_p(self.tw.itwiddles.ptr), self.tw.log_size, self.last, C.c_void_p(self.chan_ptr),
               C.c_void_p(self.alphas_ptr), self.alphas_cap, C.byref(self.first), self.outs, self.cap, C.byref(self.n_out))

    def adopt(self):
        """ownership of every returned block, as FriProver does: [(buffer, words)] in a fixed order"""
        bufs = [(L.DeviceBuffer.adopt(self.first.value, 32 * ((2 << self.col_logs[0]) - 1)), 8 * ((2 << self.col_logs[0]) - 1))]
        for i in range(self.n_out.value):
            o = self.outs[i]
            bufs += [(L.DeviceBuffer.adopt(o.cols[k], 4 << o.log_size), 1 << o.log_size) for k in range(4)]
            if o.layers:
                bufs.append((L.DeviceBuffer.adopt(o.layers, 32 * ((2 << o.log_size) - 1)), 8 * ((2 << o.log_size) - 1)))
        return bufs


def _host_reference(col_logs, bound, ch):
    """the same commit through the host transcript: (the words of every returned block in Raw.adopt's order, the alphas)"""
    cols, tw = _inputs(col_logs)
    replay = ch.clone()
    h = T.FriProver.commit(ch, T.FriConfig(bound, LOG_BLOWUP, 3), cols, tw, device_channel=False, merkle_channel=PMC)
    words = [_tree_words(h.first_layer.merkle_tree).view("<u4")]
    alphas = []
    trees = [h.first_layer.merkle_tree] + [layer.merkle_tree for layer in h.inner_layers]
    for t in trees:
        replay.mix_root(t.root())
        alphas.append(replay.draw_felt().tup())
    evals = [layer.evaluation for layer in h.inner_layers]
    for ev, layer in zip(evals, h.inner_layers):
        words += [c for c in ev.values.to_numpy()] + [_tree_words(layer.merkle_tree).view("<u4")]
    return words, alphas, replay


def test_raw_entry_alphas_and_state():
    col_logs, bound = [10, 8, 6], 1
    ch = _start_channel()
    dch = DevicePoseidon252Channel(ch)
    n_alpha = col_logs[0] - 1 - last_log(bound) + 1
    alphas = L.DeviceBuffer(16 * (n_alpha + 3))
    alphas.upload(np.full(4 * (n_alpha + 3), SENTINEL, dtype=np.uint32))
    raw = Raw(col_logs, bound, dch.buf.ptr, alphas.ptr, n_alpha + 3)
    raw.call()
    bufs = raw.adopt()
    want_words, want_alphas, replay = _host_reference(col_logs, bound, _start_channel())
    got_alphas = alphas.download(count=4 * (n_alpha + 3)).reshape(-1, 4)
    assert len(want_alphas) == n_alpha                                             # one per tree: the first layer's and every inner one
    assert [tuple(r) for r in got_alphas[:n_alpha].tolist()] == want_alphas
    assert (got_alphas[len(want_alphas):] == SENTINEL).all()                       # nothing written past the count
    assert dch.buf.download(count=10).tolist() == M.to_words(replay.digest().toBigInt()) + [replay.n_challenges, replay.n_sent]
    # (the blocks behind the host reference's list are the last layer's evaluation, which the host objects do not keep: its
    # polynomial is compared in test_one_call_commit_matches_host_transcript)
    assert len(bufs) == len(want_words) + 4
    for (b, n), w in zip(bufs, want_words):
        assert (b.download(np.uint32, n) == w).all()


def _probe(sizes):
    """one cached block per size class: allocate, free, and say which addresses the pool now hands out first"""
    blocks = [L.DeviceBuffer(s) for s in sizes]
    ptrs = [b.ptr for b in blocks]
    for b in reversed(blocks):
        b.free()
    return ptrs


def test_error_paths_leave_channel_alphas_and_allocator_alone():
    """every check runs before the first allocation: after a refused call the channel words and the alphas are what they were, no
    block is returned, and the allocator hands out the very blocks it had cached for the sizes the call would have taken first"""
    cols, tw = _inputs([5])
    ptrs8 = L.ptr_array([c.ptr for c in cols[0].values.columns] * 2)
    chan, alphas = L.DeviceBuffer(64), L.DeviceBuffer(16 * 16)
    chan_img = np.arange(100, 116, dtype=np.uint32)
    alpha_img = np.full(64, SENTINEL, dtype=np.uint32)
    chan.upload(chan_img)
    alphas.upload(alpha_img)
    outs, n_out, first = (L.FriLayerOut * 16)(), C.c_size_t(7), L.vp(1)
    sizes = [32 * ((2 << 5) - 1), 4 << 4, 32 * ((2 << 4) - 1)]
    args = lambda logs, n, last, cap, acap=16, tw_log=tw.log_size: (ptrs8, L.u32x(logs), n, C.c_void_p(tw.itwiddles.ptr), tw_log, last,
                                                                   C.c_void_p(chan.ptr), C.c_void_p(alphas.ptr), acap, C.byref(first), outs, cap,
                                                                   C.byref(n_out))
    cases = [("no columns", args([5], 0, 1, 16)), ("column sizes not decreasing", args([5, 5], 2, 1, 16)),
             ("column sizes not decreasing", args([4, 5], 2, 1, 16)), ("capacity too small", args([5], 1, 1, 2)),
             ("capacity too small", args([5], 1, 1, 16, acap=2)), ("Not enough twiddles!", args([5], 1, 1, 16, tw_log=3)),
             ("last layer larger than the first line layer", args([5], 1, 5, 16)), ("log size 3..31", args([2], 1, 0, 16)),
             ("not all columns were consumed", args([5, 3], 2, 3, 16))]
    pool = os.environ.get("TSTWO_ALLOC", "pool") in ("", "pool")         # the probe reads the caching allocator's free lists
    for why, a in cases:
        before = _probe(sizes)
        with pytest.raises(L.TstwoError, match=why):
            L.call("tstwo_fri_commit_layers_poseidon252", *a)
        assert n_out.value == 0 and not first.value, why
        assert not pool or _probe(sizes) == before, why
        assert (chan.download(count=16) == chan_img).all() and (alphas.download(count=64) == alpha_img).all(), why
    with pytest.raises(L.TstwoError, match="null argument"):
        L.call("tstwo_fri_commit_layers_poseidon252", None, L.u32x([5]), 1, C.c_void_p(tw.itwiddles.ptr), tw.log_size, 1, C.c_void_p(chan.ptr),
               C.c_void_p(alphas.ptr), 16, C.byref(first), outs, 16, C.byref(n_out))
    with pytest.raises(L.TstwoError, match="alpha must be 16-byte aligned"):
        L.call("tstwo_fri_commit_layers_poseidon252", ptrs8, L.u32x([5]), 1, C.c_void_p(tw.itwiddles.ptr), tw.log_size, 1, C.c_void_p(chan.ptr),
               C.c_void_p(alphas.ptr + 4), 16, C.byref(first), outs, 16, C.byref(n_out))
    assert (chan.download(count=16) == chan_img).all()


def test_two_commits_back_to_back_behind_a_plug():
    """two commits of different shapes on ONE device channel, enqueued behind a plug that keeps the stream busy while the host runs
    ahead, one comparison at the end: the second commit's transcript continues the first's"""
    shapes = [([10, 8, 6], 1), ([5], 0)]
    ch = _start_channel()
    want = []
    for col_logs, bound in shapes:                                # the host channel carries over from one commit to the next
        words, alphas, ch = _host_reference(col_logs, bound, ch)
        want.append((words, alphas))
    end_state = M.to_words(ch.digest().toBigInt()) + [ch.n_challenges, ch.n_sent]
    dch = DevicePoseidon252Channel(_start_channel())
    alphas = L.DeviceBuffer(16 * 32)

    def enqueue():
        raws = [Raw(col_logs, bound, dch.buf.ptr, alphas.ptr + 16 * 16 * i, 16) for i, (col_logs, bound) in enumerate(shapes)]
        for r in raws:
            r.call()
        return raws

    for r in enqueue():                                           # once eagerly: the pool now holds every block the run below takes
        for b, _ in r.adopt():
            b.free()
    dch.load(_start_channel())
    L.sync()
    plug = Q.Plug()
    try:
        plug.enqueue()
        raws = enqueue()
        plug.host_done()
        bufs = [r.adopt() for r in raws]
        state = dch.buf.download(count=10).tolist()
        plug.check()
    finally:
        plug.free()
    assert state == end_state
    got_alphas = alphas.download(count=4 * 32).reshape(-1, 4)
    for i, ((words, al), bl) in enumerate(zip(want, bufs)):
        assert [tuple(r) for r in got_alphas[16 * i:16 * i + len(al)].tolist()] == al, i
        for (b, n), w in zip(bl, words):
            assert (b.download(np.uint32, n) == w).all(), i

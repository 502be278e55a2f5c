"""The sum-check rounds of prove_batch on the device: tstwo_gkr_round_finish word for word against the round model
(tests/gkr_round_model.py), the entries that read their challenge from device memory against their by-value twins, and
prove_batch(device_rounds=True) against the integer model and the host loop — same proof, artifact and channel state, with one
read-back per layer.  Everything is exact M31 / QM31 arithmetic: every comparison is equality."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import gkr_model as M
import gkr_round_model as R
import poseidon_model as PM
import sequence as SQ
from arena import Arena, rin, rinout, rout
from tstwo_amd import _lib as L
from tstwo_amd import gkr as G
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import QM31
from tstwo_amd.gkr_verifier import Gate, partially_verify_batch

pytestmark = pytest.mark.gpu

P = M.P
KINDS = [M.GP, M.GENERIC, M.MULT, M.SINGLES]
PM1 = (P - 1, P - 1, P - 1, P - 1)
BAD_ARG = 7          # TSTWO_ERR_BAD_ARG (include/tstwo_hip.h)


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


def secure(a):
    return G.Mle.secure([a[k].astype(np.uint32) for k in range(4)])


def base(a):
    return G.Mle.base(a.astype(np.uint32))


def host(m):
    return m.to_numpy().astype(np.uint64)


def dev_layer(lay):
    den = secure(lay["den"])
    if lay["kind"] == M.GP:
        return G.Layer.grand_product(den)
    if lay["kind"] == M.GENERIC:
        return G.Layer.logup_generic(secure(lay["num"]), den)
    if lay["kind"] == M.MULT:
        return G.Layer.logup_multiplicities(base(lay["num"]), den)
    return G.Layer.logup_singles(den)


def make_layer(rng, kind, n_vars):
    n = 1 << n_vars
    num = {M.GENERIC: M.random_secure(rng, n), M.MULT: M.random_base(rng, n)}.get(kind)
    return {"kind": kind, "num": num, "den": M.random_secure(rng, n)}


def to_model(proof, artifact):
    t = lambda x: x.tup()       # noqa: E731
    p = {"sumcheck_proofs": [[[t(c) for c in rp.coeffs] for rp in sp.round_polys] for sp in proof.sumcheck_proofs],
         "masks": [[[(t(a), t(b)) for a, b in m.columns()] for m in ms] for ms in proof.layer_masks_by_instance],
         "output_claims": [[t(c) for c in cs] for cs in proof.output_claims_by_instance]}
    a = {"ood_point": [t(x) for x in artifact.ood_point],
         "claims_to_verify": [[t(c) for c in cs] for cs in artifact.claims_to_verify_by_instance],
         "n_variables": list(artifact.n_variables_by_instance)}
    return p, a


class ReadbackCounter:
    """Counts the library's synchronous read-backs at the C ABI: every call that hands device results to the host."""

    SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_gkr_sum_poly", "tstwo_gather_words"}

    def __init__(self, monkeypatch):
        self.n = 0
        orig_call = L.call

        def call(name, *a):
            if name in self.SYNC_CALLS:
                self.n += 1
            return orig_call(name, *a)
        monkeypatch.setattr(L, "call", call)


# ------------------------------------------------------------------ 1. tstwo_gkr_round_finish against the round model
def words_of(felts):
    return np.array([w for f in felts for w in f], dtype=np.uint32)


def model_channel(digest_words, n_sent):
    ch = M.Channel()
    ch.digest, ch.n_sent = np.asarray(digest_words, dtype="<u4").tobytes(), int(n_sent)
    return ch


def chan_words(ch, n_chal):
    return [int(w) for w in np.frombuffer(ch.digest, dtype="<u4")] + [n_chal, ch.n_sent]


class Finish:
    """One device block for a chain of tstwo_gkr_round_finish calls: chan (16 words) | state (8 n) | per round: sums (8 n),
    poly (20), challenge (4).  Everything that is not uploaded holds the sentinel."""

    def __init__(self, n, chan, claims, corrs, rounds):
        self.n, self.rounds = n, rounds
        self.per = 8 * n + 24
        self.words = 16 + 8 * n + self.per * len(rounds)
        img = np.full(self.words, SQ.SENTINEL, dtype=np.uint32)
        img[:10] = chan
        img[16:16 + 8 * n] = words_of([w for c, k in zip(claims, corrs) for w in (c, k)])
        for r, rd in enumerate(rounds):
            o = self.off(r)
            for i, (s, act) in enumerate(zip(rd["sums"], rd["active"])):
                if act:                                        # the slots of inactive instances stay sentinel: they are not read
                    img[o + 8 * i:o + 8 * i + 8] = words_of(s)
        self.image = img
        self.buf = L.DeviceBuffer(4 * self.words)
        self.buf.upload(img)

    def off(self, r):
        return 16 + 8 * self.n + self.per * r

    def call(self, r, n_instances=None, mask=None):
        rd = self.rounds[r]
        o = self.off(r)
        p = lambda w: C.c_void_p(self.buf.ptr + 4 * w)        # noqa: E731
        if mask is None:
            mask = sum(1 << i for i, a in enumerate(rd["active"]) if a)
        L.call("tstwo_gkr_round_finish", p(0), p(o), p(16), self.n if n_instances is None else n_instances, C.c_uint64(mask),
               L.u32x(rd["y"]), L.u32x(rd["a"]), L.u32x(rd["alpha"]), p(o + 8 * self.n), p(o + 8 * self.n + 20))

    def download(self):
        w = self.buf.download(np.uint32, self.words)
        self.buf.free()
        return w


def check_chain(n, chan, claims, corrs, rounds):
    """Enqueue every round back to back, read everything once, compare every word with the chained model."""
    f = Finish(n, chan, claims, corrs, rounds)
    for r in range(len(rounds)):
        f.call(r)
    got = f.download()
    mch = model_channel(chan[:8], chan[9])
    n_chal = int(chan[8])
    for r, rd in enumerate(rounds):
        coeffs, ch, claims, corrs = R.round_finish_at(mch, rd["sums"], claims, corrs, rd["active"], rd["y"], rd["a"], rd["alpha"])
        n_chal = (n_chal + 1) & 0xFFFFFFFF
        o = f.off(r) + 8 * n
        want_poly = [len(coeffs), 0, 0, 0] + [w for c in coeffs + [M.ZERO] * (4 - len(coeffs)) for w in c]
        assert [int(w) for w in got[o:o + 20]] == want_poly, (r, "round polynomial")
        assert tuple(int(w) for w in got[o + 20:o + 24]) == ch, (r, "challenge")
        assert (got[f.off(r):o] == f.image[f.off(r):o]).all(), (r, "sums are inputs")
    assert [int(w) for w in got[:10]] == chan_words(mch, n_chal)
    assert (got[10:16] == SQ.SENTINEL).all()
    assert [int(w) for w in got[16:16 + 8 * n]] == [int(w) for w in words_of([w for c, k in zip(claims, corrs) for w in (c, k)])]
    return got


def random_round(rng, n, active):
    return {"sums": [(M.random_felt(rng), M.random_felt(rng)) for _ in range(n)], "active": list(active),
            "y": M.random_felt(rng), "a": M.random_felt(rng), "alpha": M.random_felt(rng)}


def random_chan(rng, n_chal=3, n_sent=0):
    return [int(w) for w in rng.integers(0, 2**32, size=8, dtype=np.uint64)] + [n_chal, n_sent]


def masks_for(n):
    out = {"all": [True] * n, "first_inactive": [False] + [True] * (n - 1), "last_inactive": [True] * (n - 1) + [False]}
    if n == 64:
        out["single"] = [i == 37 for i in range(64)]
    return out


@pytest.mark.parametrize("n,mask", [(n, m) for n in (1, 2, 5, 64) for m in masks_for(n)])
def test_round_finish_matches_the_round_model(n, mask):
    rng = np.random.default_rng(100 * n + len(mask))
    claims = [M.random_felt(rng) for _ in range(n)]
    corrs = [M.random_felt(rng) for _ in range(n)]
    check_chain(n, random_chan(rng), claims, corrs, [random_round(rng, n, masks_for(n)[mask])])


def test_round_finish_all_zero_hashes_the_digest_alone():
    rng = np.random.default_rng(1)
    rd = random_round(rng, 2, [True, False])
    rd["sums"] = [(M.ZERO, M.ZERO), (M.ZERO, M.ZERO)]
    got = check_chain(2, random_chan(rng), [M.ZERO, M.ZERO], [M.random_felt(rng), M.ONE], [rd])
    assert int(got[16 + 16 + 16]) == 0                         # n_coeffs


def test_round_finish_vanishing_cubic_term_mixes_three_coefficients():
    rng = np.random.default_rng(2)
    rd = random_round(rng, 1, [True])
    f0, claim, corr = M.random_felt(rng), M.random_felt(rng), M.random_felt(rng)
    b = M.qdiv(M.qsub(M.ONE, rd["y"]), M.qsub(M.ONE, M.qdouble(rd["y"])))
    r0 = M.qmul(M.qmul(M.qmul(f0, corr), M.qsub(M.ONE, rd["y"])), rd["a"])
    w01 = M.qadd(M.qdiv(r0, M.qneg(M.qdouble(b))), M.qdiv(M.qneg(M.qsub(claim, r0)), M.qsub(M.ONE, b)))
    r2 = M.qmul(M.qneg(w01), M.qdouble(M.qsub(M.qm(2), b)))       # the Lagrange weights of 0, 1, 2 then sum to zero
    f2 = M.qdiv(r2, M.qmul(M.qmul(corr, M.qsub(M.qmul(M.qm(3), rd["y"]), M.ONE)), rd["a"]))
    rd["sums"] = [(f0, f2)]
    got = check_chain(1, random_chan(rng), [claim], [corr], [rd])
    assert int(got[16 + 8 + 8]) == 3


def test_round_finish_zero_claim_on_an_inactive_instance():
    rng = np.random.default_rng(3)
    rd = random_round(rng, 3, [True, False, True])
    check_chain(3, random_chan(rng), [M.random_felt(rng), M.ZERO, M.random_felt(rng)], [M.random_felt(rng) for _ in range(3)], [rd])


def test_round_finish_largest_coordinates():
    rng = np.random.default_rng(4)
    for active in ([True, True, True], [True, False, True]):
        rd = {"sums": [(PM1, PM1)] * 3, "active": active, "y": PM1, "a": PM1, "alpha": PM1}
        check_chain(3, random_chan(rng), [PM1] * 3, [PM1] * 3, [rd])


@pytest.mark.parametrize("alpha", [M.ZERO, M.ONE])
def test_round_finish_alpha_zero_and_one(alpha):
    rng = np.random.default_rng(5)
    rd = random_round(rng, 5, [True, True, False, True, True])
    rd["alpha"] = alpha
    check_chain(5, random_chan(rng), [M.random_felt(rng) for _ in range(5)], [M.random_felt(rng) for _ in range(5)], [rd])


def test_round_finish_channel_counters():
    rng = np.random.default_rng(6)
    rd = random_round(rng, 2, [True, True])
    check_chain(2, random_chan(rng, n_chal=0xFFFFFFFE, n_sent=7), [M.random_felt(rng)] * 2, [M.random_felt(rng)] * 2, [rd])


def test_round_finish_three_rounds_back_to_back_carry_the_state():
    rng = np.random.default_rng(7)
    n = 5
    rounds = [random_round(rng, n, [True, False, False, True, False]), random_round(rng, n, [True, True, False, True, False]),
              random_round(rng, n, [True, True, False, True, True])]
    check_chain(n, random_chan(rng), [M.random_felt(rng) for _ in range(n)], [M.ONE] * n, rounds)


@pytest.mark.parametrize("y", R.DEGENERATE_Y)
def test_round_finish_degenerate_eq_point_is_an_error_and_writes_nothing(y):
    rng = np.random.default_rng(8)
    rd = random_round(rng, 2, [True, True])
    rd["y"] = y
    f = Finish(2, random_chan(rng), [M.random_felt(rng)] * 2, [M.ONE] * 2, [rd])
    with pytest.raises(L.TstwoError) as ex:
        f.call(0)
    assert ex.value.code == BAD_ARG and str(ex.value) == "sum-check: degenerate eq point"
    with pytest.raises(ZeroDivisionError, match="0 has no inverse"):
        G.round_finish(f.buf.ptr, f.buf.ptr + 4 * f.off(0), f.buf.ptr + 64, 2, 3, y, rd["a"], rd["alpha"], f.buf.ptr + 4 * (f.off(0) + 16),
                       f.buf.ptr + 4 * (f.off(0) + 36))
    assert (f.download() == f.image).all()


def test_round_finish_refuses_bad_arguments():
    rng = np.random.default_rng(9)
    f = Finish(2, random_chan(rng), [M.random_felt(rng)] * 2, [M.ONE] * 2, [random_round(rng, 2, [True, True])])
    for n in (0, 65):
        with pytest.raises(L.TstwoError) as ex:
            f.call(0, n_instances=n)
        assert ex.value.code == BAD_ARG
    rd, o = f.rounds[0], f.off(0)
    good = [f.buf.ptr, f.buf.ptr + 4 * o, f.buf.ptr + 64, f.buf.ptr + 4 * (o + 16), f.buf.ptr + 4 * (o + 36)]
    for k in range(5):
        for bad in (0, good[k] + (2 if k == 0 else 4)):           # null; chan off a word boundary, the others off 16 bytes
            a = list(good)
            a[k] = bad
            with pytest.raises(L.TstwoError) as ex:
                L.call("tstwo_gkr_round_finish", C.c_void_p(a[0]), C.c_void_p(a[1]), C.c_void_p(a[2]), 2, C.c_uint64(3), L.u32x(rd["y"]),
                       L.u32x(rd["a"]), L.u32x(rd["alpha"]), C.c_void_p(a[3]), C.c_void_p(a[4]))
            assert ex.value.code == BAD_ARG
    assert (f.download() == f.image).all()


# ------------------------------------------------------------------ 2. challenges read from device memory
def upload_felt(r):
    b = L.DeviceBuffer(16)
    b.upload(np.array(r, dtype=np.uint32))
    return b


def null4():
    return L.p4([0] * 4)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n_vars", [1, 2, 5, 13])
@pytest.mark.parametrize("kind", KINDS)
def test_gkr_round_dev_is_gkr_round(kind, n_vars, in_place):
    """The slot and the folded columns, bit for bit; 13 variables = several blocks, so the ticket hand-off runs."""
    rng = np.random.default_rng(5000 + 100 * kind + n_vars)
    lay = make_layer(rng, kind, n_vars + 2)
    e = secure(M.random_secure(rng, 1 << (n_vars - 1)))
    lam, r = M.random_felt(rng), M.random_felt(rng)
    r_dev = upload_felt(r)
    half = 1 << (n_vars + 1)
    res = []
    for entry in ("tstwo_gkr_round", "tstwo_gkr_round_dev"):
        d = dev_layer(lay)
        if in_place:
            oden = d.den
            onum = G.Mle.uninitialized_secure(half) if kind == M.MULT else d.num       # base numerators never fold in place
        else:
            oden = G.Mle.uninitialized_secure(half)
            onum = G.Mle.uninitialized_secure(half) if d.num is not None else None
        slot = L.DeviceBuffer(32)
        r_arg = L.u32x(r) if entry == "tstwo_gkr_round" else C.c_void_p(r_dev.ptr)
        L.call(entry, kind, e.ptrs(), d.num.ptrs() if d.num else null4(), d.den.ptrs(), onum.ptrs() if onum else null4(), oden.ptrs(),
               n_vars, r_arg, L.u32x(lam), C.c_void_p(slot.ptr))
        res.append((slot.download(np.uint32, 8), host(oden)[:, :half], host(onum)[:, :half] if onum is not None else None,
                    host(d.den), host(d.num) if d.num is not None else None))
    (s0, od0, on0, den0, num0), (s1, od1, on1, den1, num1) = res
    assert (s0 == s1).all() and (od0 == od1).all() and (den0 == den1).all()
    if on0 is not None:
        assert (on0 == on1).all() and (num0 == num1).all()
    folded = {"kind": M.GENERIC if kind == M.MULT else kind, "num": M.fix_first_variable(lay["num"], r) if lay["num"] is not None else None,
              "den": M.fix_first_variable(lay["den"], r)}
    f0, f2 = M.sum_f0_f2(folded, host(e), n_vars, lam)
    assert tuple(int(w) for w in s1) == f0 + f2 and (od1 == folded["den"]).all()


def test_gkr_round_dev_refusals():
    rng = np.random.default_rng(11)
    lay = make_layer(rng, M.MULT, 4)
    d, e = dev_layer(lay), secure(M.random_secure(rng, 2))
    r_dev, slot = upload_felt(M.random_felt(rng)), L.DeviceBuffer(32)
    lam = L.u32x(M.random_felt(rng))
    oden = G.Mle.uninitialized_secure(8)
    in_place = L.p4([d.num.col.ptr] * 4)
    with pytest.raises(L.TstwoError, match="base numerators cannot be folded in place"):
        L.call("tstwo_gkr_round_dev", M.MULT, e.ptrs(), d.num.ptrs(), d.den.ptrs(), in_place, oden.ptrs(), 2, C.c_void_p(r_dev.ptr), lam,
               C.c_void_p(slot.ptr))
    onum = G.Mle.uninitialized_secure(8)
    for bad in (0, r_dev.ptr + 4):
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_round_dev", M.MULT, e.ptrs(), d.num.ptrs(), d.den.ptrs(), onum.ptrs(), oden.ptrs(), 2, C.c_void_p(bad), lam,
                   C.c_void_p(slot.ptr))
        assert ex.value.code == BAD_ARG
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_mle_fix_first_variable_secure_dev", d.den.ptrs(), 4, C.c_void_p(bad), oden.ptrs())
        assert ex.value.code == BAD_ARG
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_mle_fix_first_variable_base_dev", C.c_void_p(d.num.col.ptr), 4, C.c_void_p(bad), oden.ptrs())
        assert ex.value.code == BAD_ARG
    assert (host(d.den) == lay["den"]).all() and (host(d.num) == lay["num"]).all()


@pytest.mark.parametrize("form", ["secure", "secure_in_place", "base"])
@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_mle_fix_first_variable_dev_is_the_by_value_fold(n, form):
    rng = np.random.default_rng(2000 + n)
    col = M.random_base(rng, 1 << n) if form == "base" else M.random_secure(rng, 1 << n)
    r = M.random_felt(rng)
    r_dev = upload_felt(r)
    outs = []
    for dev in (False, True):
        m = base(col) if form == "base" else secure(col)
        out = m if form == "secure_in_place" else G.Mle.uninitialized_secure(1 << (n - 1))
        G.HipMleOps.fix_first_variable_into(m, r_dev.ptr if dev else q(r), out)
        outs.append((host(out), host(m)))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()
    assert (outs[1][0][:, :1 << (n - 1)] == M.fix_first_variable(col, r)).all()


# ------------------------------------------------------------------ 3. prove_batch on the device path
@functools.lru_cache(maxsize=None)
def case_layers(name):
    if name == "mixed":
        rng = np.random.default_rng(20)
        return tuple(make_layer(rng, k, n) for k, n in [(M.GENERIC, 13), (M.GP, 1), (M.SINGLES, 7), (M.MULT, 4), (M.GP, 10)])
    if name == "64":
        rng = np.random.default_rng(21)
        return tuple(make_layer(rng, KINDS[i % 4], 2 + (i % 3 == 0)) for i in range(64))
    if name == "65":
        rng = np.random.default_rng(22)
        return tuple(make_layer(rng, KINDS[i % 4], 3) for i in range(65))
    if name == "small":
        rng = np.random.default_rng(23)
        return tuple(make_layer(rng, k, n) for k, n in [(M.GENERIC, 4), (M.GP, 2), (M.SINGLES, 3)])
    kind, n = name
    return (make_layer(np.random.default_rng(7000 + 100 * kind + n), kind, n),)


@functools.lru_cache(maxsize=None)
def model_proof(name):
    """The integer model's proof, artifact and channel, computed once per case."""
    ch = M.Channel()
    proof, artifact = M.prove_batch(ch, list(case_layers(name)))
    return proof, artifact, ch.digest, ch.n_sent


def prove(name, channel, counter=None, **kw):
    dev = [dev_layer(lay) for lay in case_layers(name)]
    before = counter.n if counter else 0
    proof, artifact = G.prove_batch(channel, dev, **kw)
    n_readbacks = counter.n - before if counter else None
    for d, lay in zip(dev, case_layers(name)):                    # the caller's input layers are left as they were
        assert (host(d.den) == lay["den"]).all()
        if d.num is not None:
            assert (host(d.num) == lay["num"]).all()
        d.free()
    return proof, artifact, n_readbacks


def check_device_path(name, monkeypatch):
    mproof, martifact, mdigest, mn_sent = model_proof(name)
    counter = ReadbackCounter(monkeypatch)
    ch = Blake2sChannel()
    proof, artifact, n_readbacks = prove(name, ch, counter, device_rounds=True)
    monkeypatch.undo()
    p, a = to_model(proof, artifact)
    assert p == mproof and a == martifact
    assert (ch.digest(), ch.n_sent) == (mdigest, mn_sent)
    n_layers = max(a["n_variables"])
    assert n_readbacks <= n_layers + 1, (n_readbacks, n_layers)
    hch = Blake2sChannel()
    hp, ha = to_model(*prove(name, hch, device_rounds=False)[:2])
    assert hp == p and ha == a
    assert (hch.digest(), hch.n_challenges, hch.n_sent) == (ch.digest(), ch.n_challenges, ch.n_sent)
    gates = [Gate.GrandProduct if lay["kind"] == M.GP else Gate.LogUp for lay in case_layers(name)]
    art = partially_verify_batch(gates, proof, Blake2sChannel())
    assert to_model(proof, art)[1] == a


@pytest.mark.parametrize("n", [1, 2, 3, 6, 13])
@pytest.mark.parametrize("kind", KINDS)
def test_prove_batch_device_rounds_one_instance(kind, n, monkeypatch):
    if kind == M.MULT and n == 1:
        # the reference has no mask for a LogUpMultiplicities layer (tryIntoMask): the model and both paths refuse alike
        layers = list(case_layers((kind, n)))
        with pytest.raises(NotImplementedError, match="should never reach tryIntoMask"):
            M.prove_batch(M.Channel(), layers)
        for path in (True, False):
            with pytest.raises(NotImplementedError, match="should never reach tryIntoMask"):
                G.prove_batch(Blake2sChannel(), [dev_layer(layers[0])], device_rounds=path)
        return
    check_device_path((kind, n), monkeypatch)


@pytest.mark.parametrize("name", ["mixed", "64"])
def test_prove_batch_device_rounds_batches(name, monkeypatch):
    check_device_path(name, monkeypatch)


def test_prove_batch_default_is_the_device_path(monkeypatch):
    counter = ReadbackCounter(monkeypatch)
    ch = Blake2sChannel()
    proof, artifact, n_readbacks = prove("small", ch, counter)
    monkeypatch.undo()
    assert to_model(proof, artifact) == model_proof("small")[:2]
    assert n_readbacks <= max(artifact.n_variables_by_instance) + 1


# ------------------------------------------------------------------ 4. path selection
class TsCompatModelChannel(M.Channel):
    """gkr_model.Channel with the TS port's draw_felt: the 4 base felts a draw leaves over stay queued across later mixes."""

    def __init__(self):
        super().__init__()
        self.queue = []

    def draw_base_felts(self):
        """The 8 base felts of one accepted draw (gkr_model.Channel.draw_felt keeps the first 4 only)."""
        while True:
            b = hashlib.blake2s(self.digest + self.n_sent.to_bytes(4, "little") + bytes(28)).digest()
            self.n_sent += 1
            u = [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(8)]
            if all(x < 2 * P for x in u):
                return [x % P for x in u]

    def draw_felt(self):
        while len(self.queue) < 4:
            self.queue += self.draw_base_felts()
        out, self.queue = tuple(self.queue[:4]), self.queue[4:]
        return out


def host_path_cases():
    from tstwo_amd.poseidon import Poseidon252Channel
    return {"65 instances": ("65", Blake2sChannel, M.Channel),
            "ts_compat": ("small", lambda: Blake2sChannel(ts_compat=True), TsCompatModelChannel),
            "poseidon": ("small", Poseidon252Channel, PM.Channel)}


@pytest.mark.parametrize("case", ["65 instances", "ts_compat", "poseidon"])
def test_prove_batch_takes_the_host_path_where_the_device_path_cannot_run(case, monkeypatch):
    name, make_channel, make_model = host_path_cases()[case]
    mch = make_model()
    mproof, martifact = M.prove_batch(mch, list(case_layers(name)))
    counter = ReadbackCounter(monkeypatch)
    proof, artifact, n_readbacks = prove(name, make_channel(), counter)
    monkeypatch.undo()
    assert to_model(proof, artifact) == (mproof, martifact)
    n_rounds = sum(len(sp) for sp in mproof["sumcheck_proofs"])
    n_layers = max(martifact["n_variables"])
    assert n_readbacks == 1 + n_rounds + (n_layers - 1), "one read-back per round: the host loop"
    with pytest.raises(ValueError, match="device_rounds"):
        prove(name, make_channel(), device_rounds=True)


# ------------------------------------------------------------------ 5. guard bands and call sequences
def test_round_finish_between_guard_bands():
    rng = np.random.default_rng(30)
    n = 5
    active = [True, False, True, True, False]
    rd = random_round(rng, n, active)
    claims, corrs = [M.random_felt(rng) for _ in range(n)], [M.random_felt(rng) for _ in range(n)]
    chan = random_chan(rng)
    sums = np.full(8 * n, SQ.SENTINEL, dtype=np.uint32)
    for i, (s, act) in enumerate(zip(rd["sums"], active)):
        if act:
            sums[8 * i:8 * i + 8] = words_of(s)
    regs = [rinout("chan", np.array(chan, dtype=np.uint32), 4), rin("sums", sums),
            rinout("state", words_of([w for c, k in zip(claims, corrs) for w in (c, k)])), rout("poly", 20), rout("challenge", 4)]
    with Arena(regs) as A:
        L.call("tstwo_gkr_round_finish", A.ptr("chan"), A.ptr("sums"), A.ptr("state"), n, C.c_uint64(0b01101), L.u32x(rd["y"]), L.u32x(rd["a"]),
               L.u32x(rd["alpha"]), A.ptr("poly"), A.ptr("challenge"))
        got = A.check()
    mch = model_channel(chan[:8], chan[9])
    coeffs, ch, claims, corrs = R.round_finish_at(mch, rd["sums"], claims, corrs, active, rd["y"], rd["a"], rd["alpha"])
    assert [int(w) for w in got["poly"]] == [len(coeffs), 0, 0, 0] + [w for c in coeffs + [M.ZERO] * (4 - len(coeffs)) for w in c]
    assert tuple(int(w) for w in got["challenge"]) == ch
    assert [int(w) for w in got["chan"]] == chan_words(mch, chan[8] + 1)
    assert [int(w) for w in got["state"]] == [int(w) for w in words_of([w for c, k in zip(claims, corrs) for w in (c, k)])]


def cols_regs(prefix, a, role):
    a = np.asarray(a)
    cols = [a] if a.ndim == 1 else list(a)
    names = [f"{prefix}{k}" for k in range(len(cols))]
    return names, [(rin if role == "in" else rinout)(x, c.astype(np.uint32)) for x, c in zip(names, cols)]


def out_regs(prefix, n_words):
    names = [f"{prefix}{k}" for k in range(4)]
    return names, [rout(x, n_words) for x in names]


@pytest.mark.parametrize("n_vars", [1, 2, 11])
@pytest.mark.parametrize("kind", KINDS)
def test_gkr_round_dev_between_guard_bands(kind, n_vars):
    rng = np.random.default_rng(6000 + 100 * kind + n_vars)
    lay = make_layer(rng, kind, n_vars + 2)
    eq_cols = M.random_secure(rng, 1 << (n_vars - 1))
    lam, r = M.random_felt(rng), M.random_felt(rng)
    half = 1 << (n_vars + 1)
    e_, regs = cols_regs("eq", eq_cols, "in")
    d_, rr = cols_regs("den", lay["den"], "in")
    regs += rr
    n_, on_ = [], []
    if lay["num"] is not None:
        n_, rr = cols_regs("num", lay["num"], "in")
        regs += rr
        on_, rr = out_regs("onum", half)
        regs += rr
    od_, rr = out_regs("oden", half)
    regs += rr + [rin("r", np.array(r, dtype=np.uint32)), rout("result", 8)]
    with Arena(regs) as A:
        num = A.p4(n_ * (4 // len(n_))) if n_ else null4()
        L.call("tstwo_gkr_round_dev", kind, A.p4(e_), num, A.p4(d_), A.p4(on_) if on_ else null4(), A.p4(od_), n_vars, A.ptr("r"),
               L.u32x(lam), A.ptr("result"))
        got = A.check()
    folded = {"kind": M.GENERIC if kind == M.MULT else kind, "num": M.fix_first_variable(lay["num"], r) if lay["num"] is not None else None,
              "den": M.fix_first_variable(lay["den"], r)}
    f0, f2 = M.sum_f0_f2(folded, eq_cols, n_vars, lam)
    assert tuple(int(w) for w in got["result"]) == f0 + f2
    assert (np.stack([got[x] for x in od_]) == folded["den"]).all()
    if on_:
        assert (np.stack([got[x] for x in on_]) == folded["num"]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 11])
@pytest.mark.parametrize("is_base", [False, True])
def test_mle_fix_first_variable_dev_between_guard_bands(is_base, n):
    rng = np.random.default_rng(6500 + 100 * is_base + n)
    col = M.random_base(rng, 1 << n) if is_base else M.random_secure(rng, 1 << n)
    r = M.random_felt(rng)
    i_, regs = cols_regs("in", col, "in")
    o_, rr = out_regs("out", 1 << (n - 1))
    regs += rr + [rin("r", np.array(r, dtype=np.uint32))]
    with Arena(regs) as A:
        if is_base:
            L.call("tstwo_mle_fix_first_variable_base_dev", A.ptr(i_[0]), n, A.ptr("r"), A.p4(o_))
        else:
            L.call("tstwo_mle_fix_first_variable_secure_dev", A.p4(i_), n, A.ptr("r"), A.p4(o_))
        got = A.check()
    assert (np.stack([got[x] for x in o_]) == M.fix_first_variable(col, r)).all()


def _low_degree_eval(T, log_deg, log_blowup, seed):
    domain = T.CanonicCoset(log_deg + log_blowup).circleDomain()
    tw = T.precompute_twiddles(domain.halfCoset)
    rng = np.random.default_rng(seed)
    polys = [T.HipCirclePoly(T.HipColumn(rng.integers(0, P, size=1 << log_deg, dtype=np.uint32))) for _ in range(4)]
    evs = T.evaluate_polynomials(polys, domain, tw)
    return T.SecureEvaluation(domain, T.SecureColumnByCoords([e.values for e in evs])), tw


def test_prove_batch_twice_around_a_fri_commit():
    """Two device-path proofs and a FRI commit share the library's scratch block (the sums' ticket and slab), its upload ring and
    the device-channel kernels; the first proof's launches are enqueued while the stream is still busy (sequence.Plug).  Every
    result against its reference: the integer model for the proofs, the per-layer host loop for the commit."""
    import tstwo_amd as T
    cfg = T.FriConfig(2, 2, 5)
    col, tw = _low_degree_eval(T, 9, 2, 8100)
    ref_ch = T.Blake2sChannel()
    ref = T.FriProver.commit(ref_ch, cfg, [col], tw, per_layer_calls=True)
    plug = SQ.Plug(pairs=8)
    try:
        plug.enqueue()
        ch1, ch2, fch = Blake2sChannel(), Blake2sChannel(), T.Blake2sChannel()
        p1 = prove("mixed", ch1, device_rounds=True)
        fri = T.FriProver.commit(fch, cfg, [col], tw)
        p2 = prove("small", ch2, device_rounds=True)
    finally:
        L.sync()
        plug.free()
    for name, (proof, artifact, _), ch in (("mixed", p1, ch1), ("small", p2, ch2)):
        mproof, martifact, mdigest, mn_sent = model_proof(name)
        assert to_model(proof, artifact) == (mproof, martifact)
        assert (ch.digest(), ch.n_sent) == (mdigest, mn_sent)
    assert fch.digest() == ref_ch.digest()
    assert fri.first_layer.merkle_tree.root() == ref.first_layer.merkle_tree.root()
    assert len(fri.inner_layers) == len(ref.inner_layers) > 0
    for la, lb in zip(fri.inner_layers, ref.inner_layers):
        assert la.merkle_tree.root() == lb.merkle_tree.root()
        for ca, cb in zip(la.evaluation.values.to_numpy(), lb.evaluation.values.to_numpy()):
            assert (ca == cb).all()
    assert [c.tup() for c in fri.last_layer_poly.coeffs] == [c.tup() for c in ref.last_layer_poly.coeffs]

"""prove_batch in one library call: the entries that read their scalars from device memory against their by-value twins, word
for word; tstwo_gkr_layer_begin / tstwo_gkr_layer_end against the layer model (tests/gkr_layer_model.py);
prove_batch(one_call=True) against the integer model and the other two paths; the refusals; guard bands around every device
argument; and a call sequence that shares the library's scratch.  Everything is exact M31 / QM31 arithmetic: every comparison is
equality."""
import ctypes as C

import numpy as np
import pytest

import gkr_layer_model as LM
import gkr_model as M
import gkr_plan as GP
import gkr_round_model as R
import sequence as SQ
import test_gpu_gkr_rounds as TR
from arena import Arena, rin, rinout, rout
from tstwo_amd import _lib as L
from tstwo_amd import gkr as G
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.gkr_verifier import Gate, partially_verify_batch

pytestmark = pytest.mark.gpu

P = M.P
KINDS = TR.KINDS
BAD_ARG = TR.BAD_ARG
DEGENERATE = 1           # TSTWO_GKR_STATUS_DEGENERATE


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def felt_words(f):
    return np.array(f, dtype=np.uint32)


def words_of(felts):
    return np.array([w for f in felts for w in f], dtype=np.uint32)


def tup(words):
    return tuple(int(w) for w in words)


def null4():
    return L.p4([0] * 4)


# ------------------------------------------------------------------ 1. the _dev entries against their by-value twins
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("n_y", [0, 1, 2, 3, 5, 13])
def test_gen_eq_evals_dev_is_gen_eq_evals(n_y, offset):
    """n_y < 4: the low table has fewer than 4 entries (one output per lane); an output off a 16-byte boundary takes that path too."""
    rng = np.random.default_rng(300 + n_y)
    y, v = [M.random_felt(rng) for _ in range(n_y)], M.random_felt(rng)
    n = 1 << n_y
    twin = G.Mle.uninitialized_secure(n)
    L.call("tstwo_gkr_gen_eq_evals", L.u32x([w for f in y for w in f]), n_y, L.u32x(v), twin.ptrs())
    want = TR.host(twin)
    outs = [f"out{k}" for k in range(4)]
    regs = [rin("y", words_of(y + [M.ZERO])), rin("v", felt_words(v))] + [rout(x, n, offset) for x in outs]
    with Arena(regs) as A:
        L.call("tstwo_gkr_gen_eq_evals_dev", A.ptr("y"), n_y, A.ptr("v"), A.p4(outs))
        got = A.check()
    assert (np.stack([got[x] for x in outs]) == want).all()
    assert (want == M.gen_eq_evals(y, v)).all()


def test_gen_eq_evals_dev_refusals():
    out = G.Mle.uninitialized_secure(4)
    b = L.DeviceBuffer(64)
    for y, v in ((0, b.ptr), (b.ptr + 4, b.ptr), (b.ptr, 0), (b.ptr, b.ptr + 8)):
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_gen_eq_evals_dev", C.c_void_p(y), 2, C.c_void_p(v), out.ptrs())
        assert ex.value.code == BAD_ARG
    with pytest.raises(L.TstwoError) as ex:
        L.call("tstwo_gkr_gen_eq_evals_dev", C.c_void_p(b.ptr), 29, C.c_void_p(b.ptr), out.ptrs())
    assert ex.value.code == BAD_ARG


@pytest.mark.parametrize("n_vars", [1, 2, 5, 11])
@pytest.mark.parametrize("kind", KINDS)
def test_lambda_from_device_sum_and_round(kind, n_vars):
    """tstwo_gkr_sum_poly_async_ldev and tstwo_gkr_round_dev_ldev between guard bands give the slot and the folded columns of the
    entries that take lambda by value; 11 variables = several blocks, so the ticket hand-off runs."""
    rng = np.random.default_rng(8000 + 100 * kind + n_vars)
    lay = TR.make_layer(rng, kind, n_vars + 2)
    eq_cols = M.random_secure(rng, 1 << n_vars)
    lam, r = M.random_felt(rng), M.random_felt(rng)
    half = 1 << (n_vars + 1)
    # the by-value twins
    e, d = TR.secure(eq_cols), TR.dev_layer(lay)
    oden = G.Mle.uninitialized_secure(half)
    onum = G.Mle.uninitialized_secure(half) if d.num is not None else None
    slots = L.DeviceBuffer(64)
    num_p = d.num.ptrs() if d.num else null4()
    L.call("tstwo_gkr_sum_poly_async", kind, e.ptrs(), num_p, d.den.ptrs(), n_vars + 1, L.u32x(lam), C.c_void_p(slots.ptr))
    r_dev = TR.upload_felt(r)
    L.call("tstwo_gkr_round_dev", kind, e.ptrs(), num_p, d.den.ptrs(), onum.ptrs() if onum else null4(), oden.ptrs(), n_vars,
           C.c_void_p(r_dev.ptr), L.u32x(lam), C.c_void_p(slots.ptr + 32))
    want_slots = slots.download(np.uint32, 16)
    want_den, want_num = TR.host(oden)[:, :half], TR.host(onum)[:, :half] if onum is not None else None
    # the same with lambda in device memory
    e_, regs = TR.cols_regs("eq", eq_cols, "in")
    d_, rr = TR.cols_regs("den", lay["den"], "in")
    regs += rr
    n_, on_ = [], []
    if lay["num"] is not None:
        n_, rr = TR.cols_regs("num", lay["num"], "in")
        regs += rr
        on_, rr = TR.out_regs("onum", half)
        regs += rr
    od_, rr = TR.out_regs("oden", half)
    regs += rr + [rin("r", felt_words(r)), rin("lambda", felt_words(lam)), rout("sum", 8), rout("round", 8)]
    with Arena(regs) as A:
        num = A.p4(n_ * (4 // len(n_))) if n_ else null4()
        L.call("tstwo_gkr_sum_poly_async_ldev", kind, A.p4(e_), num, A.p4(d_), n_vars + 1, A.ptr("lambda"), A.ptr("sum"))
        L.call("tstwo_gkr_round_dev_ldev", kind, A.p4(e_), num, A.p4(d_), A.p4(on_) if on_ else null4(), A.p4(od_), n_vars, A.ptr("r"),
               A.ptr("lambda"), A.ptr("round"))
        got = A.check()
    assert (got["sum"] == want_slots[:8]).all() and (got["round"] == want_slots[8:]).all()
    assert (np.stack([got[x] for x in od_]) == want_den).all()
    if on_:
        assert (np.stack([got[x] for x in on_]) == want_num).all()
    assert tup(got["sum"]) == sum(M.sum_f0_f2(lay, eq_cols, n_vars + 1, lam), ())


def test_lambda_from_device_refusals():
    rng = np.random.default_rng(12)
    lay = TR.make_layer(rng, M.GENERIC, 4)
    d, e = TR.dev_layer(lay), TR.secure(M.random_secure(rng, 4))
    onum, oden = G.Mle.uninitialized_secure(8), G.Mle.uninitialized_secure(8)
    b, slot = L.DeviceBuffer(64), L.DeviceBuffer(32)
    for bad in (0, b.ptr + 4):
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_sum_poly_async_ldev", M.GENERIC, e.ptrs(), d.num.ptrs(), d.den.ptrs(), 3, C.c_void_p(bad), C.c_void_p(slot.ptr))
        assert ex.value.code == BAD_ARG
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_round_dev_ldev", M.GENERIC, e.ptrs(), d.num.ptrs(), d.den.ptrs(), onum.ptrs(), oden.ptrs(), 2, C.c_void_p(b.ptr),
                   C.c_void_p(bad), C.c_void_p(slot.ptr))
        assert ex.value.code == BAD_ARG
    assert (TR.host(d.den) == lay["den"]).all() and (TR.host(d.num) == lay["num"]).all()


def finish_dev_regions(n, chan, claims, corrs, rd, status=0):
    sums = np.full(8 * n, SQ.SENTINEL, dtype=np.uint32)
    for i, (s, act) in enumerate(zip(rd["sums"], rd["active"])):
        if act:
            sums[8 * i:8 * i + 8] = words_of(s)
    return [rinout("chan", np.array(chan, dtype=np.uint32), 4), rin("sums", sums),
            rinout("state", words_of([w for c, k in zip(claims, corrs) for w in (c, k)])), rin("y", felt_words(rd["y"])),
            rin("a", felt_words(rd["a"])), rin("alpha", felt_words(rd["alpha"])), rout("poly", 20), rout("challenge", 4),
            rinout("status", np.array([status], dtype=np.uint32), 4)]


def call_finish_dev(A, n, mask):
    L.call("tstwo_gkr_round_finish_dev", A.ptr("chan"), A.ptr("sums"), A.ptr("state"), n, C.c_uint64(mask), A.ptr("y"), A.ptr("a"), A.ptr("alpha"),
           A.ptr("poly"), A.ptr("challenge"), A.ptr("status"))


@pytest.mark.parametrize("n,mask", [(n, m) for n in (1, 2, 5, 64) for m in TR.masks_for(n)])
def test_round_finish_dev_is_round_finish(n, mask):
    rng = np.random.default_rng(100 * n + len(mask))
    active = TR.masks_for(n)[mask]
    claims, corrs = [M.random_felt(rng) for _ in range(n)], [M.random_felt(rng) for _ in range(n)]
    chan, rd = TR.random_chan(rng), TR.random_round(rng, n, active)
    f = TR.Finish(n, chan, claims, corrs, [rd])
    f.call(0)
    want = f.download()
    bits = sum(1 << i for i, a in enumerate(active) if a)
    with Arena(finish_dev_regions(n, chan, claims, corrs, rd, status=6)) as A:
        call_finish_dev(A, n, bits)
        got = A.check()
    o = f.off(0) + 8 * n
    assert (got["chan"] == want[:10]).all() and (got["state"] == want[16:16 + 8 * n]).all()
    assert (got["poly"] == want[o:o + 20]).all() and (got["challenge"] == want[o + 20:o + 24]).all()
    assert int(got["status"][0]) == 6                          # bits are ORed in, never cleared; none is set here


@pytest.mark.parametrize("y", R.DEGENERATE_Y)
def test_round_finish_dev_reports_a_degenerate_eq_point(y):
    """A device y_k cannot be refused before the launch: the status bit is set, the call returns, nothing outside the outputs is
    written (their contents are unspecified)."""
    rng = np.random.default_rng(8)
    rd = TR.random_round(rng, 3, [True, False, True])
    rd["y"] = y
    with Arena(finish_dev_regions(3, TR.random_chan(rng), [M.random_felt(rng)] * 3, [M.ONE] * 3, rd, status=2)) as A:
        call_finish_dev(A, 3, 0b101)
        got = A.check()
    assert int(got["status"][0]) == 2 | DEGENERATE


def test_round_finish_dev_refuses_bad_arguments():
    rng = np.random.default_rng(9)
    rd = TR.random_round(rng, 2, [True, True])
    with Arena(finish_dev_regions(2, TR.random_chan(rng), [M.random_felt(rng)] * 2, [M.ONE] * 2, rd)) as A:
        names = ["chan", "sums", "state", "y", "a", "alpha", "poly", "challenge", "status"]
        for k, name in enumerate(names):
            for bad in (0, A.addr(name) + (2 if name in ("chan", "status") else 4)):
                a = [A.addr(x) for x in names]
                a[k] = bad
                v = [C.c_void_p(x) for x in a]
                with pytest.raises(L.TstwoError) as ex:
                    L.call("tstwo_gkr_round_finish_dev", v[0], v[1], v[2], 2, C.c_uint64(3), v[3], v[4], v[5], v[6], v[7], v[8])
                assert ex.value.code == BAD_ARG
        for n in (0, 65):
            with pytest.raises(L.TstwoError) as ex:
                call_finish_dev(A, n, 3)
            assert ex.value.code == BAD_ARG
        A.check()


# ------------------------------------------------------------------ 2. the transcript kernels against the layer model
LANE_KINDS = (M.GP, M.GENERIC, M.SINGLES)
SHIFTS = (0, 1, 12)
N_Y = {1: 0, 2: 1, 5: 5, 64: 27}


class Lanes:
    """n lanes over random 2-word columns at odd word offsets inside one input region; lane j belongs to instance 2 j + 1 of 2 n + 2,
    so that a lane index taken for an instance index shows."""

    def __init__(self, rng, n, enter=None):
        self.n = n
        self.kinds = [LANE_KINDS[j % 3] for j in range(n)]
        self.enter = [j % 2 == 0 for j in range(n)] if enter is None else enter
        self.insts = [2 * j + 1 for j in range(n)]
        self.shifts = [SHIFTS[j % 3] for j in range(n)]
        self.cols = rng.integers(0, P, size=(n, 16, 3), dtype=np.uint64)         # per lane: 8 src + 8 out_src columns of 3 words (2 read)
        self.lanes = [{"inst": i, "kind": k, "shift": s, "enter": e} for i, k, s, e in zip(self.insts, self.kinds, self.shifts, self.enter)]

    def region(self):
        return rin("cols", self.cols.astype(np.uint32))

    def table(self, A):
        t = (L.GkrLane * self.n)()
        for j, rec in enumerate(t):
            base = A.addr("cols") + 4 * 48 * j
            rec.src = (L.vp * 8)(*[base + 12 * c for c in range(8)])
            rec.out_src = (L.vp * 8)(*[base + 12 * (8 + c) for c in range(8)])
            rec.inst, rec.kind, rec.shift, rec.enter = self.insts[j], self.kinds[j], self.shifts[j], int(self.enter[j])
        return np.frombuffer(bytes(t), dtype=np.uint8)

    def value(self, j, first_col, word):
        return tuple(int(self.cols[j, first_col + c, word]) for c in range(4))

    def outputs(self):
        out = {}
        for j, (i, k) in enumerate(zip(self.insts, self.kinds)):
            den = self.value(j, 12, 0)
            out[i] = [den] if k == M.GP else [self.value(j, 8, 0), den]
        return out

    def masks(self):
        return [LM.mask_of(k, (self.value(j, 0, 0), self.value(j, 0, 1)), (self.value(j, 4, 0), self.value(j, 4, 1)))
                for j, k in enumerate(self.kinds)]


def claim_words(claims, n_inst):
    w = np.full(8 * n_inst, SQ.SENTINEL, dtype=np.uint32)
    for i, c in claims.items():
        w[8 * i:8 * i + 8] = words_of(list(c) + [M.ZERO] * (2 - len(c)))
    return w


def run_begin(rng, ln, y, status=0):
    n, n_inst = ln.n, 2 * ln.n + 2
    chan = TR.random_chan(rng, n_chal=5, n_sent=2)
    claims = {i: [M.random_felt(rng)] * (1 if k == M.GP else 2) for i, k, e in zip(ln.insts, ln.kinds, ln.enter) if not e}
    with Arena([ln.region(), rinout("chan", np.array(chan, dtype=np.uint32), 4), rin("claims", claim_words(claims, n_inst)),
                rout("out_claims", 8 * n_inst), rout("state", 8 * n), rout("scalars", 12), rin("y", words_of(y + [M.ZERO])),
                rout("inv", 4 * max(len(y), 1)), rinout("status", np.array([status], dtype=np.uint32), 4),
                rinout("table", np.zeros(36 * n, dtype=np.uint32))]) as A:
        table = ln.table(A)
        A.buf.upload(table, A.layout.start["table"])
        L.call("tstwo_gkr_layer_begin", A.ptr("chan"), A.ptr("table"), n, A.ptr("claims"), A.ptr("out_claims"), A.ptr("state"), A.ptr("scalars"),
               A.ptr("y"), len(y), A.ptr("inv"), A.ptr("status"))
        got = A.check()
    assert (got["table"].view(np.uint8) == table).all()
    return chan, claims, got


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_layer_begin_matches_the_model(n):
    """Every kind, entering lanes beside continuing ones, claims doubled 0, 1 and 12 times; the point has 0, 1, 5 and 27 coordinates."""
    rng = np.random.default_rng(400 + n)
    ln = Lanes(rng, n)
    y = [M.random_felt(rng) for _ in range(N_Y[n])]
    chan, claims, got = run_begin(rng, ln, y)
    mch = TR.model_channel(chan[:8], chan[9])
    mclaims = [None] * (2 * n + 2)
    for i, c in claims.items():
        mclaims[i] = list(c)
    outputs = ln.outputs()
    alpha, lam, state, inv, v, bad = LM.layer_begin(mch, ln.lanes, mclaims, outputs, y)
    assert not bad and int(got["status"][0]) == 0
    assert [int(w) for w in got["chan"]] == TR.chan_words(mch, chan[8] + n)
    assert tup(got["scalars"][:4]) == alpha and tup(got["scalars"][4:8]) == lam
    assert tup(got["scalars"][8:12]) == (v if y else (SQ.SENTINEL,) * 4)
    assert [int(w) for w in got["state"]] == [int(w) for w in words_of([w for s in state for w in s])]
    assert [int(w) for w in got["inv"][:4 * len(y)]] == [int(w) for w in words_of(inv)]
    want_out = claim_words({i: outputs[i] for i, e in zip(ln.insts, ln.enter) if e}, 2 * n + 2)
    assert (got["out_claims"] == want_out).all()


@pytest.mark.parametrize("where", [0, 3])
@pytest.mark.parametrize("bad_y", R.DEGENERATE_Y)
def test_layer_begin_reports_a_degenerate_point(bad_y, where):
    rng = np.random.default_rng(41)
    y = [M.random_felt(rng) for _ in range(5)]
    y[where] = bad_y
    _, _, got = run_begin(rng, Lanes(rng, 2), y, status=4)
    assert int(got["status"][0]) == 4 | DEGENERATE


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_layer_end_matches_the_model(n):
    rng = np.random.default_rng(500 + n)
    ln = Lanes(rng, n)
    n_inst = 2 * n + 2
    chan = TR.random_chan(rng, n_chal=9, n_sent=1)
    with Arena([ln.region(), rinout("chan", np.array(chan, dtype=np.uint32), 4), rout("masks", 16 * n), rout("claims", 8 * n_inst),
                rout("challenge", 4), rinout("table", np.zeros(36 * n, dtype=np.uint32))]) as A:
        table = ln.table(A)
        A.buf.upload(table, A.layout.start["table"])
        L.call("tstwo_gkr_layer_end", A.ptr("chan"), A.ptr("table"), n, A.ptr("masks"), A.ptr("claims"), A.ptr("challenge"))
        got = A.check()
    assert (got["table"].view(np.uint8) == table).all()
    mch = TR.model_channel(chan[:8], chan[9])
    masks, mclaims = ln.masks(), [None] * n_inst
    ch = LM.layer_end(mch, ln.lanes, masks, mclaims)
    assert [int(w) for w in got["chan"]] == TR.chan_words(mch, chan[8] + n)
    assert tup(got["challenge"]) == ch
    assert [int(w) for w in got["masks"]] == [w for m in masks for w in LM.mask_words(m)]
    assert (got["claims"] == claim_words({i: mclaims[i] for i in ln.insts}, n_inst)).all()


def test_transcript_kernels_refuse_bad_arguments():
    b = L.DeviceBuffer(4096)
    p = C.c_void_p(b.ptr)
    for n in (0, 65):
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_layer_begin", p, p, n, p, p, p, p, p, 1, p, p)
        assert ex.value.code == BAD_ARG
        with pytest.raises(L.TstwoError) as ex:
            L.call("tstwo_gkr_layer_end", p, p, n, p, p, p)
        assert ex.value.code == BAD_ARG
    for k in range(9):                                       # chan, lanes, claims, out_claims, state, scalars, y, inv, status
        for bad in (0, b.ptr + (2 if k in (0, 8) else 4)):   # null; the channel and the status word off a word boundary
            a = [C.c_void_p(b.ptr)] * 9
            a[k] = C.c_void_p(bad)
            with pytest.raises(L.TstwoError) as ex:
                L.call("tstwo_gkr_layer_begin", a[0], a[1], 2, a[2], a[3], a[4], a[5], a[6], 3, a[7], a[8])
            assert ex.value.code == BAD_ARG
    for k in range(5):
        for bad in (0, b.ptr + (2 if k == 0 else 4)):
            a = [C.c_void_p(b.ptr)] * 5
            a[k] = C.c_void_p(bad)
            with pytest.raises(L.TstwoError) as ex:
                L.call("tstwo_gkr_layer_end", a[0], a[1], 2, a[2], a[3], a[4])
            assert ex.value.code == BAD_ARG
    with pytest.raises(L.TstwoError) as ex:
        L.call("tstwo_gkr_layer_begin", p, p, 2, p, p, p, p, p, 29, p, p)
    assert ex.value.code == BAD_ARG


# ------------------------------------------------------------------ 3. prove_batch(one_call=True)
class OneCallCounter(TR.ReadbackCounter):
    SYNC_CALLS = TR.ReadbackCounter.SYNC_CALLS | {"tstwo_gkr_prove_batch"}


def check_one_call(name, monkeypatch):
    mproof, martifact, mdigest, mn_sent = TR.model_proof(name)
    counter = OneCallCounter(monkeypatch)
    ch = Blake2sChannel()
    proof, artifact, n_readbacks = TR.prove(name, ch, counter, one_call=True)       # (prove checks the inputs are unchanged)
    monkeypatch.undo()
    assert n_readbacks == 1, "one library call hands results to the host"
    p, a = TR.to_model(proof, artifact)
    assert p == mproof and a == martifact
    assert (ch.digest(), ch.n_sent) == (mdigest, mn_sent)
    for path in (True, False):
        och = Blake2sChannel()
        op, oa = TR.to_model(*TR.prove(name, och, device_rounds=path)[:2])
        assert op == p and oa == a
        assert (och.digest(), och.n_challenges, och.n_sent) == (ch.digest(), ch.n_challenges, ch.n_sent)
    gates = [Gate.GrandProduct if lay["kind"] == M.GP else Gate.LogUp for lay in TR.case_layers(name)]
    art = partially_verify_batch(gates, proof, Blake2sChannel())
    assert TR.to_model(proof, art)[1] == a
    dev = [TR.dev_layer(lay) for lay in TR.case_layers(name)]
    G.verify_input_claims(artifact, dev)
    for d in dev:
        d.free()


# The batches come from tests/gkr_plan.py: test_cpu_gkr_plan.py holds exactly these to every branch of the plan.
SINGLES_CASES = sorted(b[0] for name, b in GP.gpu_batches().items() if name not in ("mixed", "64", "small"))
NAMED_CASES = [name for name in GP.gpu_batches() if name in ("mixed", "64", "small")]


def test_the_cases_are_the_plan_s_batches():
    """The layers proved here (test_gpu_gkr_rounds.case_layers) have the shapes tests/gkr_plan.py states."""
    assert SINGLES_CASES == sorted((k, n) for k in KINDS for n in (1, 2, 3, 6, 13) if (k, n) != (M.MULT, 1)) and len(NAMED_CASES) == 3
    for name in NAMED_CASES + SINGLES_CASES + ["65"]:
        assert [(lay["kind"], M.n_vars_of(lay)) for lay in TR.case_layers(name)] == GP.named_batch(name), name


@pytest.mark.parametrize("kind,n", SINGLES_CASES)
def test_prove_batch_one_call_one_instance(kind, n, monkeypatch):
    check_one_call((kind, n), monkeypatch)


def test_prove_batch_one_call_refuses_multiplicities_of_one_variable():
    with pytest.raises(NotImplementedError, match="should never reach tryIntoMask"):
        G.prove_batch(Blake2sChannel(), [TR.dev_layer(TR.case_layers((M.MULT, 1))[0])], one_call=True)


@pytest.mark.parametrize("name", NAMED_CASES)
def test_prove_batch_one_call_batches(name, monkeypatch):
    check_one_call(name, monkeypatch)


def test_prove_batch_one_call_continues_a_used_channel():
    """A channel that has mixed and drawn (n_sent != 0) goes on from where it stands, on all three paths alike."""
    res = []
    for kw in ({"one_call": True}, {"device_rounds": True}, {"device_rounds": False}):
        ch = Blake2sChannel()
        ch.mix_felts([TR.q((1, 2, 3, 4))])
        ch.draw_felt()
        ch.draw_felt()
        assert ch.n_sent == 2
        proof, artifact, _ = TR.prove("small", ch, **kw)
        res.append((TR.to_model(proof, artifact), ch.digest(), ch.n_challenges, ch.n_sent))
    assert res[0] == res[1] == res[2]
    mch = M.Channel()
    mch.mix_felts([(1, 2, 3, 4)])
    mch.draw_felt()
    mch.draw_felt()
    assert res[0][0] == M.prove_batch(mch, list(TR.case_layers("small"))) and res[0][1] == mch.digest


# ------------------------------------------------------------------ 4. refusals
def instances(layers):
    inst = (L.GkrInstance * max(len(layers), 1))()
    for rec, lay in zip(inst, layers):
        rec.kind, rec.log_n = lay.kind, lay.n_variables()
        num = lay.num.ptr_list() if lay.num is not None else []
        rec.num = (L.vp * 4)(*(num + [None] * (4 - len(num))))
        rec.den = (L.vp * 4)(*lay.den.ptr_list())
    return inst


def test_prove_batch_one_call_refusals():
    """Every refusal comes before anything is enqueued: the host block keeps its sentinel and two identical calls afterwards give
    the model's proof.  That no allocation is left behind is NOT checked here: the library has no allocator statistic to assert
    on; it follows from the code (the refusals return before the first tstwo_malloc; later exits free through ProveBuffers)."""
    from tstwo_amd.poseidon import Poseidon252Channel
    small = [TR.dev_layer(lay) for lay in TR.case_layers("small")]
    many = [TR.dev_layer(lay) for lay in TR.case_layers("65")]
    for channel, layers in ((Blake2sChannel(), many), (Poseidon252Channel(), small), (Blake2sChannel(ts_compat=True), small)):
        with pytest.raises(ValueError, match="one_call needs"):
            G.prove_batch(channel, layers, one_call=True)
    with pytest.raises(ValueError, match="no instances"):
        G.prove_batch(Blake2sChannel(), [], one_call=True)
    zero = TR.dev_layer(TR.make_layer(np.random.default_rng(1), M.GP, 0))
    with pytest.raises(ValueError, match="Some output claims were not set"):
        G.prove_batch(Blake2sChannel(), small + [zero], one_call=True)
    # the library's own refusals, before anything is enqueued
    chan = L.u32x([0] * 10)
    block = np.full(1 << 16, SQ.SENTINEL, dtype=np.uint32)
    bp = block.ctypes.data_as(L.u32p)
    words = C.c_size_t(0)
    mult1 = TR.dev_layer({"kind": M.MULT, "num": np.zeros(2, dtype=np.uint64), "den": np.ones((4, 2), dtype=np.uint64)})
    huge = instances(small)
    huge[0].log_n = 29
    null_den = instances(small)
    null_den[1].den[2] = None
    odd = instances(small)
    odd[0].num[1] = odd[0].num[1] + 2
    for inst, n, why in ((instances(many), 65, "1 to 64 instances"), (instances([]), 0, "no instances"), (instances(small + [zero]), 4, "output claims"),
                         (huge, 3, "too large"), (instances(small + [mult1]), 4, "tryIntoMask"), (null_den, 3, "null device pointer"),
                         (odd, 3, "misaligned")):
        with pytest.raises(L.TstwoError, match=why) as ex:
            L.call("tstwo_gkr_prove_batch", chan, inst, n, bp, block.size)
        assert ex.value.code == BAD_ARG
        if why not in ("null device pointer", "misaligned"):
            with pytest.raises(L.TstwoError, match=why):
                L.call("tstwo_gkr_prove_batch_words", inst, n, C.byref(words))
    L.call("tstwo_gkr_prove_batch_words", instances(small), 3, C.byref(words))
    assert words.value == GP.Plan(GP.named_batch("small")).block_words == G.one_call_layout([4, 2, 3])["words"]
    with pytest.raises(L.TstwoError, match="too small") as ex:
        L.call("tstwo_gkr_prove_batch", chan, instances(small), 3, bp, words.value - 1)
    assert ex.value.code == BAD_ARG
    # during graph capture
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="graph capture") as ex:
            G.prove_batch(Blake2sChannel(), small, one_call=True)
        assert ex.value.code == BAD_ARG
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)
    assert (block == SQ.SENTINEL).all()
    # two identical calls afterwards give identical proofs, the model's
    for _ in range(2):
        ch = Blake2sChannel()
        proof, artifact = G.prove_batch(ch, small, one_call=True)
        assert TR.to_model(proof, artifact) == TR.model_proof("small")[:2] and ch.digest() == TR.model_proof("small")[2]
    for d, lay in zip(small, TR.case_layers("small")):
        assert (TR.host(d.den) == lay["den"]).all()


# ------------------------------------------------------------------ 5. guard bands and call sequences
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("name", ["small", (M.MULT, 3), (M.SINGLES, 1)])
def test_prove_batch_one_call_inputs_between_guard_bands(name, offset):
    """The caller's layers, at any 4-byte alignment, are read and never written; the block is the model's proof."""
    layers = TR.case_layers(name)
    regs, names = [], []
    for i, lay in enumerate(layers):
        d_ = [f"den{i}_{k}" for k in range(4)]
        regs += [rin(x, lay["den"][k].astype(np.uint32), offset) for k, x in enumerate(d_)]
        n_ = []
        if lay["num"] is not None:
            cols = [lay["num"]] if lay["num"].ndim == 1 else list(lay["num"])
            n_ = [f"num{i}_{k}" for k in range(len(cols))]
            regs += [rin(x, c.astype(np.uint32), offset) for x, c in zip(n_, cols)]
        names.append((n_, d_))
    n_vars = [M.n_vars_of(lay) for lay in layers]
    lay_out = G.one_call_layout(n_vars)
    block = np.zeros(lay_out["words"], dtype=np.uint32)
    with Arena(regs) as A:
        inst = (L.GkrInstance * len(layers))()
        for rec, lay, (n_, d_) in zip(inst, layers, names):
            rec.kind, rec.log_n = lay["kind"], M.n_vars_of(lay)
            rec.num = (L.vp * 4)(*([A.addr(x) for x in n_] + [None] * (4 - len(n_))))
            rec.den = (L.vp * 4)(*[A.addr(x) for x in d_])
        L.call("tstwo_gkr_prove_batch", L.u32x([0] * 10), inst, len(layers), block.ctypes.data_as(L.u32p), block.size)
        A.check()
    mproof, martifact, mdigest, mn_sent = TR.model_proof(name)
    assert block[:8].astype("<u4").tobytes() == mdigest and int(block[9]) == mn_sent and int(block[lay_out["status"]]) == 0
    n_layers = max(n_vars)
    assert [tup(block[lay_out["ood"] + 4 * k:][:4]) for k in range(n_layers)] == martifact["ood_point"]
    for i, want in enumerate(martifact["claims_to_verify"]):
        assert [tup(block[lay_out["claims"] + 8 * i + 4 * k:][:4]) for k in range(len(want))] == want
    for L_, polys in enumerate(mproof["sumcheck_proofs"]):
        for rnd, coeffs in enumerate(polys):
            o = lay_out["polys"][L_] + 20 * rnd
            assert [int(w) for w in block[o:o + 20]] == [len(coeffs), 0, 0, 0] + [w for c in coeffs + [M.ZERO] * (4 - len(coeffs)) for w in c]
        for j, i in enumerate(lay_out["active"][L_]):
            m = mproof["masks"][i][L_ - (n_layers - n_vars[i])]
            o = lay_out["masks"][L_] + 16 * j
            assert [int(w) for w in block[o:o + 16]] == LM.mask_words(m)


def test_one_call_proofs_around_a_fri_commit_and_an_evaluate():
    """Two one-call proofs of different batches back to back behind a plug (the first one's launches are enqueued while the stream
    is busy), then a FRI commit and an evaluate: they share the library's scratch block (the sums' ticket and slab, the eq tables)
    and the pointer-table cache.  Every result against its reference."""
    import tstwo_amd as T
    cfg = T.FriConfig(2, 2, 5)
    col, tw = TR._low_degree_eval(T, 9, 2, 8200)
    ref_ch = T.Blake2sChannel()
    ref = T.FriProver.commit(ref_ch, cfg, [col], tw, per_layer_calls=True)
    rng = np.random.default_rng(8300)
    domain = T.CanonicCoset(10).circleDomain()
    tw10 = T.precompute_twiddles(domain.halfCoset)
    coeffs = [rng.integers(0, P, size=1 << 10, dtype=np.uint32) for _ in range(3)]
    ref_evals = [e.values.to_numpy() for e in T.evaluate_polynomials([T.HipCirclePoly(T.HipColumn(c)) for c in coeffs], domain, tw10)]
    plug = SQ.Plug(pairs=8)
    try:
        plug.enqueue()
        ch1, ch2, fch = Blake2sChannel(), Blake2sChannel(), T.Blake2sChannel()
        p1 = TR.prove("mixed", ch1, one_call=True)
        p2 = TR.prove("small", ch2, one_call=True)
        fri = T.FriProver.commit(fch, cfg, [col], tw)
        evals = T.evaluate_polynomials([T.HipCirclePoly(T.HipColumn(c)) for c in coeffs], domain, tw10)
        p3 = TR.prove("small", Blake2sChannel(), one_call=True)
    finally:
        L.sync()
        plug.free()
    for name, (proof, artifact, _), ch in (("mixed", p1, ch1), ("small", p2, ch2), ("small", p3, None)):
        mproof, martifact, mdigest, mn_sent = TR.model_proof(name)
        assert TR.to_model(proof, artifact) == (mproof, martifact)
        if ch is not None:
            assert (ch.digest(), ch.n_sent) == (mdigest, mn_sent)
    assert fch.digest() == ref_ch.digest()
    assert fri.first_layer.merkle_tree.root() == ref.first_layer.merkle_tree.root()
    for la, lb in zip(fri.inner_layers, ref.inner_layers):
        assert la.merkle_tree.root() == lb.merkle_tree.root()
    for e, want in zip(evals, ref_evals):
        assert (e.values.to_numpy() == want).all()

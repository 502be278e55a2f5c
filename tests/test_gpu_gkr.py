"""LogUp-GKR on the MI355X: every new C-ABI entry bit-exact against the integer model (tests/gkr_model.py), and the device
prove_batch identical to the model's prover, accepted by the host verifier, with at most rounds + layers read-backs."""
import ctypes as C

import numpy as np
import pytest

import gkr_model as M
from tstwo_amd import _lib as L
from tstwo_amd import gkr as G
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import QM31
from tstwo_amd.gkr_verifier import Gate, partially_verify_batch

pytestmark = pytest.mark.gpu

SMALL = list(range(0, 13))


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


# ------------------------------------------------------------------ eq table
@pytest.mark.parametrize("n", SMALL + [20, 24])
def test_gen_eq_evals(n):
    rng = np.random.default_rng(100 + n)
    y = [M.random_felt(rng) for _ in range(n)]
    v = M.random_felt(rng)
    out = G.HipGkrOps.genEqEvals([q(t) for t in y], q(v))
    want = M.gen_eq_evals_loop(y, v) if n <= 8 else M.gen_eq_evals(y, v)
    assert (host(out) == want).all()
    out.free()


def test_eq_evals_generate_rust_behaviour():
    rng = np.random.default_rng(7)
    assert G.EqEvals.generate([]).evals.to_numpy().tolist() == [[1], [0], [0], [0]]
    y = [M.random_felt(rng) for _ in range(6)]
    e = G.EqEvals.generate([q(t) for t in y])
    assert e.len() == 32 and (host(e.evals) == M.eq_evals_generate(y)).all()


# ------------------------------------------------------------------ next_layer
@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
@pytest.mark.parametrize("n", SMALL[1:] + [20, 24])
def test_next_layer(kind, n):
    rng = np.random.default_rng(1000 * kind + n)
    lay = make_layer(rng, kind, n)
    if n <= 12:                               # zero denominators are legal: nothing is inverted
        lay["den"][:, 0] = 0
    d = dev_layer(lay)
    nxt = G.HipGkrOps.nextLayer(d)
    want = M.next_layer(lay)
    assert nxt.kind == (M.GP if kind == M.GP else M.GENERIC)
    assert (host(nxt.den) == want["den"]).all()
    if kind != M.GP:
        assert (host(nxt.num) == want["num"]).all()
    nxt.free()
    d.free()


def test_next_layer_of_an_output_layer_is_none():
    d = dev_layer(make_layer(np.random.default_rng(0), M.GP, 0))
    assert G.HipGkrOps.nextLayer(d) is None


# ------------------------------------------------------------------ fix_first_variable
@pytest.mark.parametrize("is_base", [False, True])
@pytest.mark.parametrize("n", SMALL[1:] + [20, 24])
def test_fix_first_variable(is_base, n):
    rng = np.random.default_rng(2000 + 100 * is_base + n)
    col = M.random_base(rng, 1 << n) if is_base else M.random_secure(rng, 1 << n)
    r = M.random_felt(rng)
    m = base(col) if is_base else secure(col)
    out = G.HipMleOps.fixFirstVariable(m, q(r))
    assert out.n_variables() == n - 1
    assert (host(out) == M.fix_first_variable(col, r)).all()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 12, 20])
def test_fix_first_variable_secure_in_place(n):
    rng = np.random.default_rng(3000 + n)
    col = M.random_secure(rng, 1 << n)
    r = M.random_felt(rng)
    m = secure(col)
    G.HipMleOps.fix_first_variable_into(m, q(r), m)
    got = host(m)
    half = 1 << (n - 1)
    assert (got[:, :half] == M.fix_first_variable(col, r)).all()
    assert (got[:, half:] == col[:, half:]).all()             # the upper half is read, never written


# ------------------------------------------------------------------ sums
def dev_sum(kind, eq_dev, d, n_vars, lam, async_=False):
    num = d.num.ptrs() if d.num else L.p4([0] * 4)
    if not async_:
        out = np.zeros(8, dtype=np.uint32)
        L.call("tstwo_gkr_sum_poly", kind, eq_dev.ptrs(), num, d.den.ptrs(), n_vars, L.u32x(lam), out.ctypes.data_as(L.u32p))
        return tuple(map(int, out[:4])), tuple(map(int, out[4:]))
    slot = L.DeviceBuffer(64)
    L.call("tstwo_gkr_sum_poly_async", kind, eq_dev.ptrs(), num, d.den.ptrs(), n_vars, L.u32x(lam), C.c_void_p(slot.ptr + 32))
    w = slot.download(np.uint32, 16)
    return tuple(map(int, w[8:12])), tuple(map(int, w[12:16]))


@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
@pytest.mark.parametrize("n_vars", list(range(1, 12)) + [21])
def test_sum_poly(kind, n_vars):
    rng = np.random.default_rng(4000 + 100 * kind + n_vars)
    lay = make_layer(rng, kind, n_vars + 1)
    eq_cols = M.random_secure(rng, 1 << (n_vars - 1))
    lam = M.random_felt(rng)
    d, e = dev_layer(lay), secure(eq_cols)
    want = M.sum_f0_f2(lay, eq_cols, n_vars, lam)
    assert dev_sum(kind, e, d, n_vars, lam) == want
    assert dev_sum(kind, e, d, n_vars, lam, async_=True) == want


def test_sum_poly_zero_variables_is_the_reference_error():
    rng = np.random.default_rng(9)
    d, e = dev_layer(make_layer(rng, M.GP, 1)), secure(M.random_secure(rng, 1))
    with pytest.raises(L.TstwoError) as ex:
        dev_sum(M.GP, e, d, 0, M.ONE)
    assert ex.value.code == 10 and str(ex.value) == "Number of variables must not be zero"
    with pytest.raises(L.TstwoError, match="Number of variables must not be zero"):
        G.HipGkrOps.sumAsPolyInFirstVariable(d.into_multivariate_poly(q(M.ONE), G.EqEvals.generate([])), q(M.ONE))


@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
@pytest.mark.parametrize("n_vars", [1, 2, 5, 11, 20])
def test_fused_round(kind, n_vars):
    """tstwo_gkr_round: fold the (n_vars + 2)-variable layer by r, then sum the folded layer."""
    rng = np.random.default_rng(5000 + 100 * kind + n_vars)
    lay = make_layer(rng, kind, n_vars + 2)
    eq_cols = M.random_secure(rng, 1 << (n_vars - 1))
    lam, r = M.random_felt(rng), M.random_felt(rng)
    d, e = dev_layer(lay), secure(eq_cols)
    folded = {"kind": M.GENERIC if kind == M.MULT else kind,
              "num": M.fix_first_variable(lay["num"], r) if lay["num"] is not None else None,
              "den": M.fix_first_variable(lay["den"], r)}
    want = M.sum_f0_f2(folded, eq_cols, n_vars, lam)
    onum = G.Mle.uninitialized_secure(1 << (n_vars + 1)) if kind == M.MULT else d.num
    slot = L.DeviceBuffer(32)
    L.call("tstwo_gkr_round", kind, e.ptrs(), d.num.ptrs() if d.num else L.p4([0] * 4), d.den.ptrs(),
           onum.ptrs() if onum else L.p4([0] * 4), d.den.ptrs(), n_vars, L.u32x(r), L.u32x(lam), C.c_void_p(slot.ptr))
    w = slot.download(np.uint32, 8)
    assert (tuple(map(int, w[:4])), tuple(map(int, w[4:]))) == want
    half = 1 << (n_vars + 1)
    assert (host(d.den)[:, :half] == folded["den"]).all()
    if onum is not None:
        assert (host(onum)[:, :half] == folded["num"]).all()


# ------------------------------------------------------------------ prove_batch
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
    """Counts the library's synchronous read-backs at the C ABI: every call that hands device results to the host (the ctypes
    helpers download / download_many go through these too)."""

    SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_gkr_sum_poly", "tstwo_gather_words"}

    def __init__(self, monkeypatch):
        self.n = 0
        orig_call = L.call

        def call(name, *a):
            if name in self.SYNC_CALLS:
                self.n += 1
            return orig_call(name, *a)
        monkeypatch.setattr(L, "call", call)


def check_claims(layers, artifact):
    n = max(artifact["n_variables"])
    for lay, nv, claims in zip(layers, artifact["n_variables"], artifact["claims_to_verify"]):
        cols = [lay["den"]] if lay["kind"] in (M.GP, M.SINGLES) else [lay["num"], lay["den"]]
        assert [M.eval_mle_at(c, artifact["ood_point"][n - nv:]) for c in cols] == claims[-len(cols):]


def test_prove_batch_mixed_matches_model_and_verifies(monkeypatch):
    rng = np.random.default_rng(20)
    layers = [make_layer(rng, M.GENERIC, 13), make_layer(rng, M.GP, 1), make_layer(rng, M.SINGLES, 7), make_layer(rng, M.MULT, 4),
              make_layer(rng, M.GP, 10)]
    mch = M.Channel()
    mproof, martifact = M.prove_batch(mch, layers)
    dev = [dev_layer(lay) for lay in layers]
    inputs_before = [host(d.den) for d in dev]
    ch = Blake2sChannel()
    counter = ReadbackCounter(monkeypatch)
    proof, artifact = G.prove_batch(ch, dev)
    n_readbacks = counter.n
    monkeypatch.undo()
    p, a = to_model(proof, artifact)
    assert p == mproof
    assert a == martifact
    assert ch.digest() == mch.digest
    n_layers = max(a["n_variables"])
    n_rounds = sum(len(sp) for sp in p["sumcheck_proofs"])
    assert n_readbacks <= n_rounds + n_layers, (n_readbacks, n_rounds, n_layers)
    for d, before in zip(dev, inputs_before):            # the caller's input layers are left as they were
        assert (host(d.den) == before).all()
    vch = Blake2sChannel()
    art = partially_verify_batch([Gate.GrandProduct if l["kind"] == M.GP else Gate.LogUp for l in layers], proof, vch)
    assert to_model(proof, art)[1] == a
    check_claims(layers, a)
    for lay, out in zip(layers, p["output_claims"]):
        assert out == M.direct_output(lay)


def test_prove_batch_logup_generic_2_22():
    rng = np.random.default_rng(22)
    lay = make_layer(rng, M.GENERIC, 22)
    proof, artifact = G.prove_batch(Blake2sChannel(), [dev_layer(lay)])
    art = partially_verify_batch([Gate.LogUp], proof, Blake2sChannel())
    _, a = to_model(proof, artifact)
    assert to_model(proof, art)[1] == a
    check_claims([lay], a)


def test_sumcheck_over_the_oracle_matches_model():
    """The generic path: sumcheck.prove_batch over a GkrMultivariatePolyOracle (one synchronous sum per round, fix_first_variable
    into new buffers, try_into_mask) gives the model's round polynomials, challenges and mask."""
    from tstwo_amd import sumcheck as S
    for kind in (M.GP, M.GENERIC, M.MULT, M.SINGLES):
        rng = np.random.default_rng(6000 + kind)
        n = 6
        lay = make_layer(rng, kind, n + 1)
        y = [M.random_felt(rng) for _ in range(n)]
        lam, alpha, claim = M.random_felt(rng), M.random_felt(rng), M.random_felt(rng)
        m_polys, m_assign, m_oracles, _ = M.sumcheck_prove_batch([claim], [M.Oracle(M.eq_evals_generate(y), y, lay, M.ONE, lam)],
                                                                 alpha, M.Channel())
        oracle = dev_layer(lay).into_multivariate_poly(q(lam), G.EqEvals.generate([q(t) for t in y]))
        proof, assign, oracles, claims = S.prove_batch([q(claim)], [oracle], q(alpha), Blake2sChannel())
        assert [[c.tup() for c in rp.coeffs] for rp in proof.round_polys] == m_polys
        assert [c.tup() for c in assign] == m_assign
        assert [(a.tup(), b.tup()) for a, b in oracles[0].try_into_mask().columns()] == m_oracles[0].mask()

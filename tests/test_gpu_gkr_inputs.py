"""-m gpu: the way into LogUp-GKR and the way out.  tstwo_gkr_logup_denominators bit for bit against numpy, the Python mirror
(logup_input_layer, Layer.eval_at_point, verify_input_claims, check_logup_sum), and a range check that goes trace columns ->
input layers -> prove_batch -> partially_verify_batch -> the claims on the input layers."""
import numpy as np
import pytest

import gkr_model as M
from arena import Arena, rin, rout
from test_gpu_gkr import dev_layer, make_layer, to_model
from tstwo_amd import _lib as L
from tstwo_amd import gkr as G
from tstwo_amd import gkr_lookup as GL
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import QM31
from tstwo_amd.gkr_verifier import Gate, partially_verify_batch
from tstwo_amd.logup import LinearForm, LookupElements, lookup_multiplicities
from tstwo_amd.prover import InvalidLogupSum

pytestmark = pytest.mark.gpu

P = M.P
BAD_ARG = 7                     # TSTWO_ERR_BAD_ARG


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


def qcol(t):
    return np.array(t, dtype=np.uint64)[:, None]


def model_denominators(cols, coeffs, constant):
    """sum_t coeffs[t] cols[t][r] + constant as a (4, n) column."""
    acc = np.zeros((4, len(cols[0])), dtype=np.uint64)
    for c, k in zip(cols, coeffs):
        acc = M.vadd(acc, M.vmul_base(qcol(k), c))
    return M.vadd(acc, qcol(constant))


def run_denominators(cols, coeffs, constant, log_n, offset=0):
    """Through the C ABI, between guard bands: the inputs stay as they were and nothing is stored outside the 4 outputs."""
    names = [f"c{k}" for k in range(len(cols))]
    outs = [f"o{k}" for k in range(4)]
    regs = [rin(nm, c.astype(np.uint32), offset) for nm, c in zip(names, cols)] + [rout(o, 1 << log_n, offset) for o in outs]
    with Arena(regs) as A:
        L.call("tstwo_gkr_logup_denominators", A.ptrs(names), L.u32x([w for k in coeffs for w in k]), len(cols), L.u32x(constant), log_n,
               A.p4(outs))
        got = A.check()
    return np.stack([got[o] for o in outs])


# ------------------------------------------------------------------ tstwo_gkr_logup_denominators
@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 12, 20])
@pytest.mark.parametrize("n_terms", [1, 2, 16])
def test_logup_denominators_match_numpy(n_terms, log_n):
    rng = np.random.default_rng(8000 + 100 * n_terms + log_n)
    cols = [M.random_base(rng, 1 << log_n) for _ in range(n_terms)]
    coeffs = [M.random_felt(rng) for _ in range(n_terms)]
    constant = M.random_felt(rng)
    assert (run_denominators(cols, coeffs, constant, log_n) == model_denominators(cols, coeffs, constant)).all()


@pytest.mark.parametrize("log_n,offset", [(2, 4), (5, 8), (12, 12)])
def test_logup_denominators_unaligned(log_n, offset):
    rng = np.random.default_rng(8100 + log_n)
    cols = [M.random_base(rng, 1 << log_n) for _ in range(3)]
    coeffs = [M.random_felt(rng) for _ in range(3)]
    constant = M.random_felt(rng)
    assert (run_denominators(cols, coeffs, constant, log_n, offset) == model_denominators(cols, coeffs, constant)).all()


@pytest.mark.parametrize("log_n", [1, 6])
def test_logup_denominators_saturated(log_n):
    """16 terms of (P - 1) (P - 1) in every coordinate and the constant P - 1: the largest 64-bit sums the kernel can meet between
    two folds (a folded sum below 2^33 and four products)."""
    sat = (P - 1,) * 4
    cols = [np.full(1 << log_n, P - 1, dtype=np.uint64)] * 16
    got = run_denominators(cols, [sat] * 16, sat, log_n)
    assert (got == model_denominators(cols, [sat] * 16, sat)).all()
    assert (got == (16 + P - 1) % P).all()                       # 16 (-1)(-1) + (-1) = 15


def test_logup_denominators_refusals():
    col = HipColumn(np.arange(64, dtype=np.uint32))
    out = G.Mle.uninitialized_secure(64)
    before = out.to_numpy().copy()
    ok_c, ok_k = L.u32x([1, 2, 3, 4] * 17), L.u32x([5, 6, 7, 8])
    cols = L.ptr_array([col.ptr] * 17)
    cases = {
        "1 to 16 terms": (cols, ok_c, 0, ok_k, 6, out.ptrs()), "1 to 16 terms.": (cols, ok_c, 17, ok_k, 6, out.ptrs()),
        "log_n above 28": (cols, ok_c, 1, ok_k, 29, out.ptrs()),
        "an output column is also an input": (cols, ok_c, 2, ok_k, 6, L.p4([out.col.columns[0].ptr, col.ptr, out.col.columns[2].ptr, out.col.columns[3].ptr])),
        "an output column is also an input.": (L.ptr_array([out.col.columns[1].ptr + 16]), ok_c, 1, ok_k, 6, out.ptrs()),
        "coefficient word out of range": (cols, L.u32x([1, 2, 3, 4, 1, P, 3, 4]), 2, ok_k, 6, out.ptrs()),
        "constant out of range": (cols, ok_c, 2, L.u32x([0, 0, 0, 2 ** 32 - 1]), 6, out.ptrs()),
        "null host argument": (None, ok_c, 1, ok_k, 6, out.ptrs()),
    }
    for text, args in cases.items():
        with pytest.raises(L.TstwoError, match="^logup denominators: " + text.rstrip(".")) as e:
            L.call("tstwo_gkr_logup_denominators", *args)
        assert e.value.code == BAD_ARG, text
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        L.call("tstwo_gkr_logup_denominators", L.ptr_array([col.ptr, 0]), ok_c, 2, ok_k, 6, out.ptrs())
    assert (out.to_numpy() == before).all()
    with pytest.raises(ValueError, match="1 to 16 column terms"):
        G.logup_denominators(LinearForm([], QM31.one()))
    # and the entry works on the same arguments once they are within the limits
    L.call("tstwo_gkr_logup_denominators", cols, ok_c, 16, ok_k, 6, out.ptrs())
    want = model_denominators([np.arange(64, dtype=np.uint64)] * 16, [(1, 2, 3, 4)] * 16, (5, 6, 7, 8))
    assert (out.to_numpy() == want).all()


# ------------------------------------------------------------------ the Python mirror
def test_logup_input_layer_gives_the_three_kinds():
    rng = np.random.default_rng(8200)
    n = 64
    a, b = M.random_base(rng, n), M.random_base(rng, n)
    ca, cb = HipColumn(a.astype(np.uint32)), HipColumn(b.astype(np.uint32))
    el = LookupElements(q(M.random_felt(rng)), q(M.random_felt(rng)), 3)
    # relation.combine_columns: a + alpha b + alpha^2 7 - z
    want = model_denominators([a, b], [M.ONE, el.alpha.tup()], M.qsub(M.qmul(M.qm(7), el.alpha_powers[2].tup()), el.z.tup()))
    singles = G.logup_input_layer(el, [ca, cb, 7])
    assert singles.kind == G.LOGUP_SINGLES and singles.num is None and (singles.den.to_numpy() == want).all()
    mult = G.logup_input_layer(el, [ca, cb, 7], numerators=cb)
    assert mult.kind == G.LOGUP_MULTIPLICITIES and mult.num.is_base and (mult.num.to_numpy() == b).all()
    assert (mult.den.to_numpy() == want).all()
    assert G.logup_input_layer(el, [ca, cb, 7], numerators=G.Mle.base(cb)).kind == G.LOGUP_MULTIPLICITIES
    sec = M.random_secure(rng, n)
    gen = G.logup_input_layer(el.combine_columns([ca, cb, 7]), numerators=G.Mle.secure([c.astype(np.uint32) for c in sec]))
    assert gen.kind == G.LOGUP_GENERIC and (gen.num.to_numpy() == sec).all() and (gen.den.to_numpy() == want).all()
    with pytest.raises(ValueError):
        G.logup_input_layer(el)
    with pytest.raises(ValueError):
        G.logup_input_layer(el.combine_columns([ca]), [ca])


@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
def test_layer_eval_at_point_is_in_mask_order(kind):
    rng = np.random.default_rng(8300 + kind)
    lay = make_layer(rng, kind, 9)
    point = [M.random_felt(rng) for _ in range(9)]
    got = [v.tup() for v in dev_layer(lay).eval_at_point([q(p) for p in point])]
    den = M.eval_mle_at(lay["den"], point)
    want = {M.GP: [den], M.SINGLES: [M.ONE, den]}.get(kind) or [M.eval_mle_at(lay["num"], point), den]
    assert got == want


def _set_word(column: HipColumn, index: int, value: int) -> None:
    column.buf.upload(np.array([value], dtype=np.uint32), 4 * index)


def test_verify_input_claims_on_the_mixed_batch():
    """The batch of test_prove_batch_mixed_matches_model_and_verifies (13 / 1 / 7 / 4 / 10 variables): the artifact's claims hold
    on the input layers, and stop holding when one word of one input layer changes."""
    rng = np.random.default_rng(20)
    layers = [make_layer(rng, M.GENERIC, 13), make_layer(rng, M.GP, 1), make_layer(rng, M.SINGLES, 7), make_layer(rng, M.MULT, 4),
              make_layer(rng, M.GP, 10)]
    dev = [dev_layer(lay) for lay in layers]
    proof, artifact = G.prove_batch(Blake2sChannel(), dev)
    gates = [Gate.GrandProduct if l["kind"] == M.GP else Gate.LogUp for l in layers]
    art = partially_verify_batch(gates, proof, Blake2sChannel())
    G.verify_input_claims(art, dev)
    G.verify_input_claims(artifact, dev)
    with pytest.raises(ValueError):
        G.verify_input_claims(art, dev[:4])
    # one word of the LogUpSingles denominators (instance 2: columns [1, den])
    word = int(layers[2]["den"][2, 77])
    _set_word(dev[2].den.col.columns[2], 77, (word + 1) % P)
    with pytest.raises(G.GkrInputClaimMismatch) as e:
        G.verify_input_claims(art, dev)
    assert (e.value.instance, e.value.column) == (2, 1)
    _set_word(dev[2].den.col.columns[2], 77, word)
    G.verify_input_claims(art, dev)
    # one multiplicity (instance 3: columns [num, den])
    word = int(layers[3]["num"][5])
    _set_word(dev[3].num.col, 5, (word + P - 1) % P)
    with pytest.raises(G.GkrInputClaimMismatch) as e:
        G.verify_input_claims(art, dev)
    assert (e.value.instance, e.value.column) == (3, 0)


def test_check_logup_sum():
    rng = np.random.default_rng(8400)
    a, b, d = (q(M.random_felt(rng)) for _ in range(3))
    gates = [Gate.LogUp, Gate.GrandProduct, Gate.LogUp]
    # a / d - a / d = 0; the grand product's output is not a fraction
    G.check_logup_sum([[a, d], [b], [a.neg(), d]], gates)
    G.check_logup_sum([[a, d], [b], [a, d]], gates, claimed=a.add(a).mul(d.inverse()))
    with pytest.raises(InvalidLogupSum):
        G.check_logup_sum([[a, d], [b], [a, d]], gates)
    with pytest.raises(InvalidLogupSum):
        G.check_logup_sum([[QM31.zero(), QM31.zero()]], [Gate.LogUp])


# ------------------------------------------------------------------ a range check through GKR, end to end
def _values(rng, log_range, n_cols, log_rows):
    return [rng.integers(0, 1 << log_range, size=1 << log_rows, dtype=np.uint32) for _ in range(n_cols)]


@pytest.mark.parametrize("log_range,n_cols,log_rows", [(4, 2, 6), (10, 3, 12)])
def test_range_check_end_to_end(log_range, n_cols, log_rows):
    rng = np.random.default_rng(8500 + log_range)
    values = _values(rng, log_range, n_cols, log_rows)
    cols = [HipColumn(v) for v in values]
    proof = GL.gkr_range_check_prove(Blake2sChannel(), log_range, cols)
    GL.gkr_range_check_verify(Blake2sChannel(), log_range, proof, cols)
    for c, v in zip(cols, values):                                   # the trace columns are left as they were
        assert (c.to_numpy() == v).all()

    # one changed multiplicity: the circuits still verify, their fractions no longer cancel
    mult = lookup_multiplicities(log_range, *cols, order="natural").to_numpy()
    mult[3] = (int(mult[3]) + 1) % P
    bad = GL.gkr_range_check_prove(Blake2sChannel(), log_range, cols, multiplicities=HipColumn(mult))
    with pytest.raises(InvalidLogupSum):
        GL.gkr_range_check_verify(Blake2sChannel(), log_range, bad, cols)

    # one value changed after proving (to another value of the range): the claim on that column's input layer fails
    row = 11
    _set_word(cols[1], row, (int(values[1][row]) + 1) % (1 << log_range))
    with pytest.raises(G.GkrInputClaimMismatch) as e:
        GL.gkr_range_check_verify(Blake2sChannel(), log_range, proof, cols)
    assert (e.value.instance, e.value.column) == (1, 1)


def test_range_check_proof_equals_the_model():
    """The same layers built in numpy and proved by gkr_model.prove_batch: the same proof and the same channel."""
    log_range, rng = 6, np.random.default_rng(8600)
    values = _values(rng, log_range, 2, 8)
    ch = Blake2sChannel()
    proof = GL.gkr_range_check_prove(ch, log_range, [HipColumn(v) for v in values])
    z = LookupElements.draw(Blake2sChannel(), 1).z.tup()
    mch = M.Channel()
    mch.draw_felt()                                                   # the draw of (z, alpha): one hash
    layers = [{"kind": M.SINGLES, "num": None, "den": M.vsub(M.lift(v.astype(np.uint64)), qcol(z))} for v in values]
    mult = np.bincount(np.concatenate(values), minlength=1 << log_range).astype(np.uint64)
    layers.append({"kind": M.MULT, "num": (P - mult) % P, "den": M.vsub(M.lift(np.arange(1 << log_range, dtype=np.uint64)), qcol(z))})
    mproof, _ = M.prove_batch(mch, layers)
    p, _ = to_model(proof, G.GkrArtifact([], [], []))
    assert p == mproof
    assert ch.digest() == mch.digest
    for lay, out in zip(layers, p["output_claims"]):
        assert out == M.direct_output(lay)

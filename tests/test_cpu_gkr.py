"""LogUp-GKR without a GPU: the integer model (tests/gkr_model.py) against the reference's properties, and the host verifier
(tstwo_amd.gkr_verifier) on model proofs — accepted as made, rejected with the matching error when one value changes."""
import json
import os

import numpy as np
import pytest

import gkr_model as M
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import QM31
from tstwo_amd.gkr_verifier import Gate, GkrBatchProof, GkrError, GkrErrorType, GkrMask, partially_verify_batch
from tstwo_amd.sumcheck import SumcheckProof, UnivariatePoly

ROOT = os.path.dirname(os.path.abspath(__file__))


def q(t):
    return QM31.from_u32_unchecked(*t)


def to_proof(proof):
    """Model proof (tuples) -> tstwo_amd proof objects."""
    return GkrBatchProof([SumcheckProof([UnivariatePoly([q(c) for c in p]) for p in layer]) for layer in proof["sumcheck_proofs"]],
                         [[GkrMask([(q(a), q(b)) for a, b in m]) for m in ms] for ms in proof["masks"]],
                         [[q(c) for c in cs] for cs in proof["output_claims"]])


def gate_of(kind):
    return Gate.GrandProduct if kind == M.GP else Gate.LogUp


def make_layer(rng, kind, n_vars):
    n = 1 << n_vars
    num = {M.GENERIC: M.random_secure(rng, n), M.MULT: M.random_base(rng, n)}.get(kind)
    return {"kind": kind, "num": num, "den": M.random_secure(rng, n)}


def test_model_qm31_against_golden_vectors():
    d = json.load(open(os.path.join(ROOT, "golden", "qm31-test-vectors.json")))
    ops = {"add": M.qadd, "sub": M.qsub, "mul": M.qmul}
    n = 0
    for v in d["test_vectors"]:
        if v["operation"] in ops:
            assert ops[v["operation"]](tuple(v["inputs"]["a"]), tuple(v["inputs"]["b"])) == tuple(v["output"])
            a, b = np.array(v["inputs"]["a"], dtype=np.uint64)[:, None], np.array(v["inputs"]["b"], dtype=np.uint64)[:, None]
            vec = {"add": M.vadd, "sub": M.vsub, "mul": M.vmul}[v["operation"]](a, b)
            assert M.at(vec, 0) == tuple(v["output"])
            n += 1
        elif v["operation"] == "neg":
            assert M.qneg(tuple(v["inputs"]["value"])) == tuple(v["output"])
        elif v["operation"] == "inverse":
            x = tuple(v["inputs"]["value"] if "value" in v["inputs"] else v["inputs"]["a"])
            assert M.qinv(x) == tuple(v["output"])
    assert n >= 90


def test_gen_eq_evals_is_a_product_of_eq_terms():
    rng = np.random.default_rng(3)
    for n in range(0, 7):
        y = [M.random_felt(rng) for _ in range(n)]
        v = M.random_felt(rng)
        ev = M.gen_eq_evals_loop(y, v)
        assert (ev == M.gen_eq_evals(y, v)).all()
        for x in range(1 << n):
            bits = [M.qm((x >> (n - 1 - k)) & 1) for k in range(n)]     # first variable = most significant bit
            assert M.at(ev, x) == M.qmul(v, M.eq(bits, y))


def test_fix_first_variable_matches_fold_mle_evals():
    rng = np.random.default_rng(4)
    r = M.random_felt(rng)
    for col in (M.random_secure(rng, 16), M.random_base(rng, 16)):
        out = M.fix_first_variable(col, r)
        for i in range(8):
            assert M.at(out, i) == M.fold_mle_evals(r, M.at(col, i), M.at(col, i + 8))


@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
def test_corrected_round_polynomial_properties(kind):
    """r(0) + r(1) = claim, r(b) = 0 at the root of eq(t, y[n-k]), and the claim is the layer's eq-weighted gate sum."""
    rng = np.random.default_rng(5 + kind)
    n = 5
    y = [M.random_felt(rng) for _ in range(n)]
    lam = M.random_felt(rng)
    layer = make_layer(rng, kind, n + 1)
    eqe = M.eq_evals_generate(y)
    # claim = sum_x eq(x, y) gate(x): the next layer's values against the full eq table
    nxt = M.next_layer(layer)
    vals = [nxt["den"]] if kind == M.GP else [nxt["num"], nxt["den"]]
    full = M.gen_eq_evals(y, M.ONE)
    per = [M.vsum(M.vmul(c, full)) for c in vals]
    claim = M.random_linear_combination(per, lam)
    oracle = M.Oracle(eqe, y, layer, M.ONE, lam)
    r = oracle.sum_as_poly(claim)
    assert M.qadd(M.horner(r, M.ZERO), M.horner(r, M.ONE)) == claim
    yk = y[0]
    b = M.qdiv(M.qsub(M.ONE, yk), M.qsub(M.ONE, M.qdouble(yk)))
    assert M.horner(r, b) == M.ZERO
    assert len(r) <= 4
    # one more round: the folded oracle's polynomial sums to r(challenge)
    c = M.random_felt(rng)
    r2 = oracle.fix_first_variable(c).sum_as_poly(M.horner(r, c))
    assert M.qadd(M.horner(r2, M.ZERO), M.horner(r2, M.ONE)) == M.horner(r, c)


def test_sum_of_zero_variables_fails_with_the_reference_message():
    with pytest.raises(ValueError, match="Number of variables must not be zero"):
        M.sum_f0_f2(make_layer(np.random.default_rng(0), M.GP, 1), M.eq_evals_generate([]), 0, M.ONE)


def prove_and_verify(layers):
    proof, artifact = M.prove_batch(M.Channel(), layers)
    ch = Blake2sChannel()
    art = partially_verify_batch([gate_of(l["kind"]) for l in layers], to_proof(proof), ch)
    assert [x.tup() for x in art.ood_point] == artifact["ood_point"]
    assert [[x.tup() for x in c] for c in art.claims_to_verify_by_instance] == artifact["claims_to_verify"]
    assert art.n_variables_by_instance == artifact["n_variables"]
    return proof, artifact


@pytest.mark.parametrize("kind", [M.GP, M.GENERIC, M.MULT, M.SINGLES])
def test_verifier_accepts_model_proof_of_each_layer_kind(kind):
    rng = np.random.default_rng(10 + kind)
    layer = make_layer(rng, kind, 6)
    proof, artifact = prove_and_verify([layer])
    assert proof["output_claims"][0] == M.direct_output(layer)
    cols = [layer["den"]] if kind in (M.GP, M.SINGLES) else [layer["num"], layer["den"]]
    claims = artifact["claims_to_verify"][0][-len(cols):]
    assert [M.eval_mle_at(c, artifact["ood_point"]) for c in cols] == claims


def mixed_batch(rng):
    """4 instances whose sum-check oracles have 0 to 12 variables (input layers of 1 to 13)."""
    return [make_layer(rng, M.GENERIC, 13), make_layer(rng, M.GP, 1), make_layer(rng, M.SINGLES, 7), make_layer(rng, M.MULT, 4)]


def test_verifier_accepts_mixed_batch():
    layers = mixed_batch(np.random.default_rng(20))
    proof, artifact = prove_and_verify(layers)
    n = max(artifact["n_variables"])
    for lay, nv, claims, out in zip(layers, artifact["n_variables"], artifact["claims_to_verify"], proof["output_claims"]):
        assert out == M.direct_output(lay)
        cols = [lay["den"]] if lay["kind"] in (M.GP, M.SINGLES) else [lay["num"], lay["den"]]
        assert [M.eval_mle_at(c, artifact["ood_point"][n - nv:]) for c in cols] == claims[-len(cols):]


def _tamper(proof, where):
    p = {"sumcheck_proofs": [[list(c) for c in layer] for layer in proof["sumcheck_proofs"]],
         "masks": [[[list(col) for col in m] for m in ms] for ms in proof["masks"]],
         "output_claims": [list(c) for c in proof["output_claims"]]}
    bump = lambda t: ((t[0] + 1) % M.P,) + tuple(t[1:])      # noqa: E731
    if where == "round":
        p["sumcheck_proofs"][3][1][2] = bump(p["sumcheck_proofs"][3][1][2])
    elif where == "mask":
        p["masks"][0][4][1][0] = bump(p["masks"][0][4][1][0])
    else:
        p["output_claims"][2][1] = bump(p["output_claims"][2][1])
    return p


@pytest.mark.parametrize("where,err", [("round", GkrErrorType.InvalidSumcheck), ("mask", GkrErrorType.CircuitCheckFailure),
                                       ("output", GkrErrorType.InvalidSumcheck)])
def test_verifier_rejects_one_changed_value(where, err):
    layers = mixed_batch(np.random.default_rng(21))
    proof, _ = M.prove_batch(M.Channel(), layers)
    bad = _tamper(proof, where)
    with pytest.raises(GkrError) as e:
        partially_verify_batch([gate_of(l["kind"]) for l in layers], to_proof(bad), Blake2sChannel())
    assert e.value.type is err


def test_verifier_rejects_wrong_instance_count_and_mask_shape():
    layers = mixed_batch(np.random.default_rng(22))
    proof, _ = M.prove_batch(M.Channel(), layers)
    gates = [gate_of(l["kind"]) for l in layers]
    with pytest.raises(GkrError) as e:
        partially_verify_batch(gates[:3], to_proof(proof), Blake2sChannel())
    assert e.value.type is GkrErrorType.NumInstancesMismatch
    gates[0] = Gate.GrandProduct                       # a LogUp mask has 2 columns
    with pytest.raises(GkrError) as e:
        partially_verify_batch(gates, to_proof(proof), Blake2sChannel())
    assert e.value.type is GkrErrorType.InvalidMask

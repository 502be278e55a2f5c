"""The layer begin / end model (tests/gkr_layer_model.py) tied to gkr_model.prove_batch: chained with the round model over all
layers it gives the same proof, artifact and channel (no GPU)."""
import numpy as np
import pytest

import gkr_layer_model as LM
import gkr_model as M
import gkr_plan as GP
import gkr_round_model as R


def make_batch(name, seed):
    rng = np.random.default_rng(seed)
    out = []
    for kind, n_vars in GP.named_batch(name):
        n = 1 << n_vars
        num = {M.GENERIC: M.random_secure(rng, n), M.MULT: M.random_base(rng, n)}.get(kind)
        out.append({"kind": kind, "num": num, "den": M.random_secure(rng, n)})
    return out


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_layers_chained_are_prove_batch(name):
    layers = make_batch(name, 23 if name == "small" else 20)
    ch_model, ch_chain = M.Channel(), M.Channel()
    want = M.prove_batch(ch_model, layers)
    got = LM.prove_batch_by_layers(ch_chain, layers)
    assert got[0] == want[0] and got[1] == want[1]
    assert (ch_chain.digest, ch_chain.n_sent) == (ch_model.digest, ch_model.n_sent)


def test_lanes_are_the_plan_s_lanes():
    for name in ("small", "mixed", "64"):
        batch = GP.named_batch(name)
        p = GP.Plan(batch)
        for L, lay in enumerate(p.layers):
            lanes = LM.lanes_of([n for _, n in batch], [k for k, _ in batch], L)
            assert [ln["inst"] for ln in lanes] == lay["active"]
            assert [ln["inst"] for ln in lanes if ln["enter"]] == lay["enter"]
            assert all(ln["shift"] == p.first[ln["inst"]] for ln in lanes)


def test_layer_begin_inverse_table_and_degenerate_points():
    rng = np.random.default_rng(5)
    y = [M.random_felt(rng) for _ in range(6)]
    lanes = [{"inst": 0, "kind": M.GP, "shift": 2, "enter": True}]
    _, _, state, inv, v, bad = LM.layer_begin(M.Channel(), lanes, [None], [[M.random_felt(rng)]], y)
    assert not bad and inv == R.inv_eq0_table(y) and v == M.qsub(M.ONE, y[0]) and state[0][1] == M.ONE
    for d in R.DEGENERATE_Y:
        assert LM.layer_begin(M.Channel(), lanes, [None], [[M.ONE]], y[:3] + [d] + y[3:])[5]


def test_mask_words_and_reduce():
    a, b, c, d = [(k, k + 1, k + 2, k + 3) for k in (1, 10, 20, 30)]
    assert LM.mask_words([(a, b)]) == list(a + b) + [0] * 8
    assert LM.mask_words([(a, b), (c, d)]) == list(a + b + c + d)
    claims = [None]
    ch = LM.layer_end(M.Channel(), [{"inst": 0}], [LM.mask_of(M.SINGLES, None, (c, d))], claims)
    assert claims[0] == [M.ONE, M.fold_mle_evals(ch, c, d)]
    with pytest.raises(NotImplementedError):
        LM.mask_of(M.MULT, (a, b), (c, d))

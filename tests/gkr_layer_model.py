"""The top and the bottom of a layer of prove_batch, stated on gkr_model's tuples: what the prover does around a layer's batched
sum-check (gkr_prover.ts:452-500 and 540-575).  tstwo_gkr_layer_begin / tstwo_gkr_layer_end are checked against it word by word;
chained with the round model over all layers it is gkr_model.prove_batch (test_cpu_gkr_layers.py).

It imports nothing from the package under test.  Scalars are QM31 4-tuples; `channel` is a gkr_model.Channel (updated).  A lane is
an active instance of the layer: {"inst", "kind" (of the layer its mask comes from: GP, GENERIC or SINGLES), "shift", "enter"}."""
from __future__ import annotations

import gkr_model as M
import gkr_round_model as R


def layer_begin(channel, lanes, claims, outputs, y):
    """claims[inst] = the claims to verify (updated for entering lanes from outputs[inst]).  Returns (alpha, lambda, state, inv_eq0,
    v, degenerate): state[lane] = (claim, 1); inv_eq0[r] = 1 / prod_{j <= r} (1 - y_j); v = 1 - y_0 (None without coordinates);
    degenerate = the host path raises for this point."""
    for ln in lanes:
        if ln["enter"]:
            claims[ln["inst"]] = list(outputs[ln["inst"]])
    for ln in lanes:
        channel.mix_felts(claims[ln["inst"]])
    alpha = channel.draw_felt()
    lam = channel.draw_felt()
    state = [(M.qmul(M.random_linear_combination(claims[ln["inst"]], lam), M.qm(1 << ln["shift"])), M.ONE) for ln in lanes]
    degenerate = any(v in R.DEGENERATE_Y for v in y)
    inv = None if degenerate else R.inv_eq0_direct(y)
    return alpha, lam, state, inv, (M.qsub(M.ONE, y[0]) if y else None), degenerate


def mask_of(kind, num2, den2):
    """tryIntoMask from the two values of each column of a 2-point layer."""
    if kind == M.GP:
        return [tuple(den2)]
    if kind == M.SINGLES:
        return [(M.ONE, M.ONE), tuple(den2)]
    if kind == M.MULT:
        raise NotImplementedError("LogUpMultiplicities should never reach tryIntoMask")
    return [tuple(num2), tuple(den2)]


def layer_end(channel, lanes, masks, claims):
    """masks[lane] = its mask's columns.  Mixes them in lane order, draws the challenge, reduces: claims[inst] is updated.  Returns
    the challenge."""
    for m in masks:
        channel.mix_felts([v for col in m for v in col])
    ch = channel.draw_felt()
    for ln, m in zip(lanes, masks):
        claims[ln["inst"]] = [M.fold_mle_evals(ch, a, b) for a, b in m]
    return ch


def mask_words(m):
    """The 16 words tstwo_gkr_layer_end stores for a mask: column 0 at 0 and 1, column 1 at 0 and 1 (zero for one column)."""
    cols = list(m) + [(M.ZERO, M.ZERO)] * (2 - len(m))
    return [w for col in cols for v in col for w in v]


def lanes_of(n_vars_by_instance, kinds, layer):
    """The lanes of `layer` for a batch, as csrc/gkr_plan.h orders them."""
    n_layers = max(n_vars_by_instance)
    lanes = []
    for i, (nv, kind) in enumerate(zip(n_vars_by_instance, kinds)):
        n_v = layer - (n_layers - nv)
        if n_v < 0:
            continue
        if n_v + 1 < nv:                    # a generated layer: every LogUp kind generates LogUpGeneric
            k = M.GP if kind == M.GP else M.GENERIC
        elif n_v >= 1:                      # the input, folded: base numerators have become secure
            k = M.GENERIC if kind == M.MULT else kind
        else:                               # the input itself, of one variable
            k = kind
        lanes.append({"inst": i, "kind": k, "shift": layer - n_v, "enter": n_v == 0, "n_v": n_v})
    return lanes


def prove_batch_by_layers(channel, input_layers):
    """gkr_model.prove_batch restated as begin -> rounds (gkr_round_model.round_finish_at) -> end per layer."""
    n_vars = [M.n_vars_of(l) for l in input_layers]
    kinds = [l["kind"] for l in input_layers]
    n_layers = max(n_vars)
    stacks = [list(reversed(M.gen_layers(l))) for l in input_layers]          # [output, 1 variable, ..., input]
    outputs = [M.output_values(st[0]) for st in stacks]
    claims = [None] * len(input_layers)
    masks_by = [[] for _ in input_layers]
    sumcheck_proofs, ood = [], []
    for layer in range(n_layers):
        lanes = lanes_of(n_vars, kinds, layer)
        alpha, lam, state, inv, _, degenerate = layer_begin(channel, lanes, claims, outputs, ood)
        assert not degenerate
        eqe = M.eq_evals_generate(ood)
        cur = [stacks[ln["inst"]][ln["n_v"] + 1] for ln in lanes]
        sclaims, corrs = [s[0] for s in state], [s[1] for s in state]
        polys, assignment = [], []
        for rnd in range(layer):
            rem = layer - rnd
            active = [ln["n_v"] >= rem for ln in lanes]
            for j, ln in enumerate(lanes):                 # the challenge of the round before is applied first
                if active[j] and ln["n_v"] > rem:
                    cur[j] = fix_layer(cur[j], assignment[-1])
            sums = [M.sum_f0_f2(lay, eqe, rem, lam) if act else None for lay, act in zip(cur, active)]
            coeffs, ch, sclaims, corrs = R.round_finish_at(channel, sums, sclaims, corrs, active, ood[rnd], inv[rnd], alpha)
            polys.append(coeffs)
            assignment.append(ch)
        for j, ln in enumerate(lanes):
            if ln["n_v"] >= 1:
                cur[j] = fix_layer(cur[j], assignment[-1])
        masks = []
        for ln, lay in zip(lanes, cur):
            assert M.n_vars_of(lay) == 1
            num2 = None if lay["num"] is None else (M.at(lay["num"], 0), M.at(lay["num"], 1))
            masks.append(mask_of(lay["kind"], num2, (M.at(lay["den"], 0), M.at(lay["den"], 1))))
            assert lay["kind"] == ln["kind"]
        ch = layer_end(channel, lanes, masks, claims)
        for ln, m in zip(lanes, masks):
            masks_by[ln["inst"]].append(m)
        sumcheck_proofs.append(polys)
        ood = assignment + [ch]
    proof = {"sumcheck_proofs": sumcheck_proofs, "masks": masks_by, "output_claims": outputs}
    return proof, {"ood_point": ood, "claims_to_verify": claims, "n_variables": n_vars}


def fix_layer(lay, r):
    num = None if lay["num"] is None or lay["kind"] == M.SINGLES else M.fix_first_variable(lay["num"], r)
    return {"kind": M.GENERIC if lay["kind"] == M.MULT else lay["kind"], "num": num, "den": M.fix_first_variable(lay["den"], r)}

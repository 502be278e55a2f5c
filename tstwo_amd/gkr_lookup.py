"""A range check through LogUp-GKR, on columns that live on the device: trace columns -> input layers -> prove_batch ->
partially_verify_batch -> the claims on the input layers.

Every value column v contributes the fractions 1 / (v[r] - z) (one LogUpSingles instance per column) and the table
contributes -m[k] / (k - z), m = the multiplicities of the values (one LogUpMultiplicities instance over an iota column), so
the fractions of all instances add up to zero exactly when every value lies in [0, 2^log_range).  z is drawn from the channel
(LookupElements of one value).  Nothing is downloaded except what prove_batch and the evaluations read back.

gkr_range_check_prove / _verify have no commitment scheme under them: the verifier is given the value columns themselves and
rebuilds the input layers from them.  Inside a STARK the last step (verify_input_claims) becomes a statement about committed
columns: gkr_range_check_stark_prove / _verify below commit the columns and prove the claims with mle_eval components
(tstwo_amd/mle_eval.py); their verifier sees the proofs and the log sizes only."""
from __future__ import annotations

import numpy as np

from .backend import HipBackend, HipColumn
from .gkr import check_logup_sum, logup_input_layer, prove_batch, verify_input_claims
from .gkr_verifier import Gate, partially_verify_batch
from .logup import LookupElements, LookupGroup, lookup_multiplicities, lookup_multiplicities_keyed


def gkr_range_check_layers(elements: LookupElements, log_range: int, value_columns, multiplicities=None, enablers=None):
    """The input layers: one LogUpSingles layer per value column, then the table's LogUpMultiplicities layer (numerators: the
    negated multiplicities in natural order, `multiplicities` when given; denominators over the iota column 0 .. 2^log_range - 1).
    enablers: one 0/1 column per value column.  A value column's layer is then a LogUpMultiplicities layer whose numerators are
    its enabler, so a row with enabler 0 (padding) may hold anything, and the table's numerators are the negated weighted counts
    (logup.lookup_multiplicities_keyed, weight = the enabler)."""
    cols = [c if isinstance(c, HipColumn) else HipColumn(c) for c in value_columns]
    if enablers is None:
        layers = [logup_input_layer(elements, [c]) for c in cols]
        mult = multiplicities if multiplicities is not None else lookup_multiplicities(log_range, *cols, order="natural")
    else:
        ens = [e if isinstance(e, HipColumn) else HipColumn(e) for e in enablers]
        if len(ens) != len(cols):
            raise ValueError(f"{len(ens)} enablers for {len(cols)} value columns")
        # a layer owns its numerators (Layer.free): it gets a copy, the caller's column stays
        layers = [logup_input_layer(elements, [c], numerators=e.clone()) for c, e in zip(cols, ens)]
        mult = multiplicities if multiplicities is not None else lookup_multiplicities_keyed(
            [LookupGroup([(c, log_range)], weight=e) for c, e in zip(cols, ens)], order="natural")
    iota = HipColumn(np.arange(1 << log_range, dtype=np.uint32))
    layers.append(logup_input_layer(elements, [iota], numerators=HipBackend().neg(mult)))
    return layers


def gkr_range_check_prove(channel, log_range: int, value_columns, multiplicities=None, enablers=None):
    """Proves that every word of `value_columns` (HipColumns of 2^k rows each) lies in [0, 2^log_range).  Returns the
    GkrBatchProof.  multiplicities: a HipColumn of 2^log_range counts to use in place of the counted ones.  enablers: one 0/1
    column per value column; only the rows it enables are checked."""
    elements = LookupElements.draw(channel, 1)
    layers = gkr_range_check_layers(elements, log_range, value_columns, multiplicities, enablers)
    proof, _ = prove_batch(channel, layers)
    for lay in layers:
        lay.free()
    return proof


def gkr_range_check_verify(channel, log_range: int, proof, value_columns, enablers=None) -> None:
    """Verifies a gkr_range_check_prove proof against the value columns: the GKR circuits (GkrError), the fraction sum of their
    outputs (InvalidLogupSum) and the input layers at the out-of-domain point (GkrInputClaimMismatch)."""
    elements = LookupElements.draw(channel, 1)
    gates = [Gate.LogUp] * (len(value_columns) + 1)
    artifact = partially_verify_batch(gates, proof, channel)
    check_logup_sum(proof.output_claims_by_instance, gates)
    layers = gkr_range_check_layers(elements, log_range, value_columns, enablers=enablers)
    try:
        verify_input_claims(artifact, layers)
    finally:
        for lay in layers:
            lay.free()


# ------------------------------------------------------------------ the same range check inside a STARK
# The value columns and the multiplicities are committed, and the last step is one mle_eval component per log size
# (tstwo_amd/mle_eval.py) instead of verify_input_claims: the verifier never holds a value column.
#
# Trees.  Preprocessed: per component its 2 s + 2 selectors, then the table's iota column in storage order (word k = k: the row
# order of a column is the order of its MLE).  Main: the value columns, then the multiplicities in natural order.  Interaction:
# 8 base columns (E, S) per component.  Components: one over the value columns' log size (the first) and, when log_range differs
# from it, one over log_range; with equal sizes one component carries every claim.
# Transcript.  Commit the preprocessed and the main tree, draw z (LookupElements of one value), prove_batch / partially_verify_batch,
# draw gamma, commit the interaction tree, prove / verify.  Every claim v comes from the GKR artifact: the claims of the
# instances of one log size are batched with powers of gamma into one form at the matching suffix of the out-of-domain point.
class GkrStarkProof:
    """What gkr_range_check_stark_prove hands the verifier: the GKR batch proof and the STARK proof."""

    def __init__(self, gkr_proof, stark_proof):
        self.gkr_proof, self.stark_proof = gkr_proof, stark_proof


def _stark_layout(log_range: int, log_sizes):
    """The components' shape from public data: [(log size, value column indices, carries the table)], values first."""
    log_sizes = [int(s) for s in log_sizes]
    if not log_sizes or len(set(log_sizes)) != 1:
        raise ValueError("the value columns must share one log size")
    m = log_sizes[0]
    if m == log_range:
        return [(m, list(range(len(log_sizes))), True)]
    return [(m, list(range(len(log_sizes))), False), (log_range, [], True)]


def _stark_components(layout, log_range: int, n_values: int, z, gamma, artifact, native: bool):
    """The mle_eval components of the layout from the artifact's claims (both sides run this), in layout order."""
    from .air import TraceLocationAllocator
    from .constraint_framework import FrameworkComponent
    from .fields import QM31
    from .gkr import GkrInputClaimMismatch
    from .mle_eval import MleEvalEval, MleEvalForm, batched_form, n_selector_columns
    one, n_max = QM31.one(), max(artifact.n_variables_by_instance)
    want = [s for s, vals, _ in layout for _ in vals] + [log_range]
    if list(artifact.n_variables_by_instance) != want:
        raise ValueError(f"the artifact's instances have {list(artifact.n_variables_by_instance)} variables, the columns {want}")
    claims = artifact.claims_to_verify_by_instance
    alloc, comps, evals, pre_at = TraceLocationAllocator(), [], [], 0
    n_pre_total = sum(n_selector_columns(s) for s, _, _ in layout)            # the iota column follows every selector
    for s, vals, table in layout:
        forms, vs = [], []
        for k, i in enumerate(vals):
            if claims[i][0].tup() != one.tup():                              # a LogUpSingles layer: its numerators are the constant 1
                raise GkrInputClaimMismatch(i, 0)
            forms.append(MleEvalForm([(one, ("main", k))], z.neg()))
            vs.append(claims[i][1])
        n_main = len(vals) + (1 if table else 0)
        if table:
            forms += [MleEvalForm([(one.neg(), ("main", len(vals)))]), MleEvalForm([(one, ("pre", 0))], z.neg())]
            vs += list(claims[n_values])
        form, v = batched_form(vs, forms, gamma)
        form.n_main = n_main
        ev = MleEvalEval(s, artifact.ood_point[n_max - s:], v, form)
        pre = list(range(pre_at, pre_at + n_selector_columns(s))) + ([n_pre_total] if table else [])
        pre_at += n_selector_columns(s)
        comps.append(FrameworkComponent(ev, alloc, pre, native=native))
        evals.append(ev)
    return comps, evals


def gkr_range_check_stark_prove(channel, log_range: int, value_columns, multiplicities=None, config=None, twiddles=None,
                                merkle=None, native: bool = False):
    """Proves inside a STARK that every word of `value_columns` (HipColumns of one log size, at least 2; log_range at least 2)
    lies in [0, 2^log_range).  multiplicities: a HipColumn of 2^log_range counts in natural order to use in place of the counted
    ones.  config: a PcsConfig (default PcsConfig()); twiddles: a twiddle tree that covers the largest log size + 1 + the
    blowup; merkle: the Merkle channel of a non-Blake2s `channel`.  Returns a GkrStarkProof."""
    from .circle import CanonicCoset
    from .mle_eval import mle_eval_interaction_trace, mle_eval_selector_columns
    from .pcs import CommitmentSchemeProver, PcsConfig
    from .poly import HipCircleEvaluation, precompute_twiddles
    from .prover import prove
    cols = [c if isinstance(c, HipColumn) else HipColumn(c) for c in value_columns]
    log_sizes = [c.len().bit_length() - 1 for c in cols]
    layout = _stark_layout(log_range, log_sizes)
    config = config or PcsConfig()
    if twiddles is None:
        top = max(s for s, _, _ in layout) + 1 + config.fri_config.log_blowup_factor
        twiddles = precompute_twiddles(CanonicCoset(top).circleDomain().halfCoset)
    mult = multiplicities if multiplicities is not None else lookup_multiplicities(log_range, *cols, order="natural")
    iota = HipColumn(np.arange(1 << log_range, dtype=np.uint32))

    def evals(columns, log):
        domain = CanonicCoset(log).circleDomain()
        return [HipCircleEvaluation(domain, c) for c in columns]

    def commit(evs):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(channel)
    scheme = CommitmentSchemeProver(config, twiddles, merkle)
    commit([e for s, _, _ in layout for e in evals(mle_eval_selector_columns(s), s)] + evals([iota], log_range))
    commit(evals(cols, log_sizes[0]) + evals([mult], log_range))
    elements = LookupElements.draw(channel, 1)
    layers = gkr_range_check_layers(elements, log_range, cols, mult)
    try:
        gkr_proof, artifact = prove_batch(channel, layers)
    finally:
        for lay in layers:
            lay.free()
    gamma = channel.draw_felt()
    comps, mle_evals = _stark_components(layout, log_range, len(cols), elements.z, gamma, artifact, native)
    inter = []
    for (s, vals, table), ev in zip(layout, mle_evals):
        main = [cols[i] for i in vals] + ([mult] if table else [])
        inter += mle_eval_interaction_trace(ev.point, ev.claim, ev.form.on_columns(main, [iota]))
    commit(inter)
    return GkrStarkProof(gkr_proof, prove(comps, channel, scheme))


def gkr_range_check_stark_verify(channel, log_range: int, log_sizes, proof: GkrStarkProof, config=None, merkle=None) -> None:
    """Verifies a gkr_range_check_stark_prove proof from public data alone: log_sizes, the log size of every value column.  In
    order: the GKR circuits (GkrError), the fraction sum of their outputs (InvalidLogupSum), the forms and claims of the mle_eval
    components from the artifact (GkrInputClaimMismatch for a LogUpSingles numerator claim that is not 1, ValueError for an
    out-of-domain point with a coordinate 0 or 1), the STARK (prover.verify's errors)."""
    from .air import Components
    from .mle_eval import n_selector_columns
    from .pcs import PcsConfig
    from .pcs_verifier import CommitmentSchemeVerifier
    from .prover import InvalidStructure, verify
    log_sizes = [int(s) for s in log_sizes]
    layout = _stark_layout(log_range, log_sizes)
    config = config or PcsConfig()
    stark = proof.stark_proof
    if len(stark.commitments) != 4:
        raise InvalidStructure("4 commitments expected: preprocessed, main, interaction, composition")
    scheme = CommitmentSchemeVerifier(config, merkle)
    scheme.commit(stark.commitments[0], [s for s, _, _ in layout for _ in range(n_selector_columns(s))] + [log_range], channel)
    scheme.commit(stark.commitments[1], log_sizes + [log_range], channel)
    elements = LookupElements.draw(channel, 1)
    gates = [Gate.LogUp] * (len(log_sizes) + 1)
    artifact = partially_verify_batch(gates, proof.gkr_proof, channel)
    check_logup_sum(proof.gkr_proof.output_claims_by_instance, gates)
    gamma = channel.draw_felt()
    comps, _ = _stark_components(layout, log_range, len(log_sizes), elements.z, gamma, artifact, False)
    n_pre = sum(n_selector_columns(s) for s, _, _ in layout) + 1
    scheme.commit(stark.commitments[2], Components(comps, n_pre).column_log_sizes()[2], channel)
    verify(comps, channel, scheme, stark)

"""A range check through LogUp-GKR, on columns that live on the device: trace columns -> input layers -> prove_batch ->
partially_verify_batch -> the claims on the input layers.

Every value column v contributes the fractions 1 / (v[r] - z) (one LogUpSingles instance per column) and the table
contributes -m[k] / (k - z), m = the multiplicities of the values (one LogUpMultiplicities instance over an iota column), so
the fractions of all instances add up to zero exactly when every value lies in [0, 2^log_range).  z is drawn from the channel
(LookupElements of one value).  Nothing is downloaded except what prove_batch and the evaluations read back.

This example has no commitment scheme under it: the verifier is given the value columns themselves and rebuilds the input
layers from them.  Inside a STARK the last step (verify_input_claims) becomes a statement about committed columns."""
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

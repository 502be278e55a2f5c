"""GKR batch verifier (lookups/gkr_verifier.ts:14-200) and the proof objects the prover hands it.  Host only: per layer it
checks one sum-check transcript and evaluates each instance's gate on its 2-point mask."""
from __future__ import annotations

from enum import Enum

from .fields import M31, QM31
from .sumcheck import SumcheckError, eq, fold_mle_evals, partially_verify, random_linear_combination


class Gate(Enum):
    LogUp = "LogUp"
    GrandProduct = "GrandProduct"


class GkrMask:
    """Each input column of a layer restricted to the line through its two points: [(v0, v1), ...]."""

    def __init__(self, columns):
        self._columns = [tuple(c) for c in columns]

    def columns(self):
        return list(self._columns)

    def to_rows(self):
        return [c[0] for c in self._columns], [c[1] for c in self._columns]

    def reduce_at_point(self, x: QM31):
        return [fold_mle_evals(x, v0, v1) for v0, v1 in self._columns]

    def __eq__(self, o):
        return isinstance(o, GkrMask) and [(a.tup(), b.tup()) for a, b in self._columns] == [(a.tup(), b.tup()) for a, b in o._columns]


class GkrBatchProof:
    def __init__(self, sumcheck_proofs, layer_masks_by_instance, output_claims_by_instance):
        self.sumcheck_proofs = list(sumcheck_proofs)
        self.layer_masks_by_instance = [list(m) for m in layer_masks_by_instance]
        self.output_claims_by_instance = [list(c) for c in output_claims_by_instance]


class GkrArtifact:
    def __init__(self, ood_point, claims_to_verify_by_instance, n_variables_by_instance):
        self.ood_point = list(ood_point)
        self.claims_to_verify_by_instance = [list(c) for c in claims_to_verify_by_instance]
        self.n_variables_by_instance = list(n_variables_by_instance)


class GkrErrorType(Enum):
    MalformedProof = "MalformedProof"
    InvalidMask = "InvalidMask"
    NumInstancesMismatch = "NumInstancesMismatch"
    InvalidSumcheck = "InvalidSumcheck"
    CircuitCheckFailure = "CircuitCheckFailure"


class GkrError(Exception):
    def __init__(self, type: GkrErrorType, **details):
        self.type, self.details = type, details
        super().__init__(GkrError._message(type, details))

    @staticmethod
    def _message(t, d):
        if t is GkrErrorType.MalformedProof:
            return "proof data is invalid"
        if t is GkrErrorType.InvalidMask:
            return f"mask in layer {d.get('instance_layer')} of instance {d.get('instance')} is invalid"
        if t is GkrErrorType.NumInstancesMismatch:
            return f"provided an invalid number of instances (given {d.get('given')}, proof expects {d.get('proof')})"
        if t is GkrErrorType.InvalidSumcheck:
            return f"sum-check invalid in layer {d.get('layer')}: {d.get('source')}"
        return f"circuit check failed in layer {d.get('layer')} (calculated {d.get('output')}, claim {d.get('claim')})"


class InvalidNumMaskColumnsError(Exception):
    pass


def evaluate_gate(gate: Gate, mask: GkrMask):
    """gkr_verifier.ts:171: the gate's output values from the mask of its two inputs."""
    cols = mask.columns()
    if gate is Gate.LogUp:
        if len(cols) != 2:
            raise InvalidNumMaskColumnsError()
        (na, nb), (da, db) = cols
        return [na.mul(db).add(nb.mul(da)), da.mul(db)]
    if gate is Gate.GrandProduct:
        if len(cols) != 1:
            raise InvalidNumMaskColumnsError()
        a, b = cols[0]
        return [a.mul(b)]
    raise ValueError(f"Unknown gate type: {gate}")


def partially_verify_batch(gate_by_instance, proof: GkrBatchProof, channel) -> GkrArtifact:
    """Checks every layer's sum-check and gate evaluation; returns the claims on the input layers still to be checked
    (against the committed input columns, at artifact.ood_point)."""
    masks_by = proof.layer_masks_by_instance
    if len(masks_by) != len(proof.output_claims_by_instance):
        raise GkrError(GkrErrorType.MalformedProof)
    n_inst = len(masks_by)
    n_layers_of = [len(m) for m in masks_by]
    n_layers = max(n_layers_of) if n_layers_of else 0
    if n_layers != len(proof.sumcheck_proofs):
        raise GkrError(GkrErrorType.MalformedProof)
    if len(gate_by_instance) != n_inst:
        raise GkrError(GkrErrorType.NumInstancesMismatch, given=len(gate_by_instance), proof=n_inst)
    ood = []
    claims = [None] * n_inst
    for layer, sc_proof in enumerate(proof.sumcheck_proofs):
        rem = n_layers - layer
        for i in range(n_inst):
            if n_layers_of[i] == rem:
                claims[i] = list(proof.output_claims_by_instance[i])
        for c in claims:
            if c is not None:
                channel.mix_felts(c)
        alpha = channel.draw_felt()
        lam = channel.draw_felt()
        sc_claims, insts = [], []
        for i, c in enumerate(claims):
            if c is not None:
                unused = n_layers - n_layers_of[i]
                sc_claims.append(random_linear_combination(c, lam).mulM31(M31(1 << unused)))
                insts.append(i)
        sc_claim = random_linear_combination(sc_claims, alpha)
        try:
            sc_ood, sc_eval = partially_verify(sc_claim, sc_proof, channel)
        except SumcheckError as e:
            raise GkrError(GkrErrorType.InvalidSumcheck, layer=layer, source=e) from e
        layer_evals = []
        for i in insts:
            unused = n_layers - n_layers_of[i]
            mask = masks_by[i][layer - unused]
            try:
                out = evaluate_gate(gate_by_instance[i], mask)
            except InvalidNumMaskColumnsError:
                raise GkrError(GkrErrorType.InvalidMask, instance=i, instance_layer=layer - unused) from None
            e = eq(ood[unused:], sc_ood[unused:])
            layer_evals.append(e.mul(random_linear_combination(out, lam)))
        layer_eval = random_linear_combination(layer_evals, alpha)
        if not sc_eval.equals(layer_eval):
            raise GkrError(GkrErrorType.CircuitCheckFailure, claim=sc_eval, output=layer_eval, layer=layer)
        for i in insts:
            mask = masks_by[i][layer - (n_layers - n_layers_of[i])]
            channel.mix_felts([v for col in mask.columns() for v in col])
        ch = channel.draw_felt()
        ood = list(sc_ood) + [ch]
        for i in insts:
            claims[i] = masks_by[i][layer - (n_layers - n_layers_of[i])].reduce_at_point(ch)
    if any(c is None for c in claims):
        raise GkrError(GkrErrorType.MalformedProof)
    return GkrArtifact(ood, claims, n_layers_of)

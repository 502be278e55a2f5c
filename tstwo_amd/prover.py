"""prove / verify of a set of AIR components (Rust stwo prover/mod.rs; the reference's prover/index.ts has the shapes, but its
OODS point is QM31.zero() and its components are stubs, so nothing there produces a proof).

Default "rust" semantics only: there is no working TS prove() to be transcript-compatible with.

prove: draw alpha -> composition polynomial on the device (air.ComponentProvers) -> commit its 4 coordinate polynomials as one
tree -> draw the OODS point -> prove_values on the mask points plus the composition tree's [[oods]] * 4 -> sanity check that the
composition value from the sampled coordinates equals the one the constraints give at the OODS point.  Between drawing alpha and
the composition root, nothing is read back from the device."""
from __future__ import annotations

from dataclasses import dataclass

from .air import ComponentProvers, Components, Trace
from .circle import CirclePoint
from .fields import QM31
from .pcs import CommitmentSchemeProof
from .pcs_verifier import VerificationError

SECURE_EXTENSION_DEGREE = 4


class ConstraintsNotSatisfied(Exception):
    """ProvingError::ConstraintsNotSatisfied."""

    def __init__(self, msg: str = "Constraints not satisfied."):
        super().__init__(msg)


class InvalidStructure(VerificationError):
    """VerificationError::InvalidStructure."""

    def __init__(self, details: str = ""):
        super().__init__("Proof has invalid structure" + (f": {details}" if details else ""))


class OodsNotMatching(VerificationError):
    """VerificationError::OodsNotMatching."""

    def __init__(self):
        super().__init__("The composition polynomial OODS value does not match the trace OODS values (DEEP-ALI failure).")


class InvalidLogupSum(VerificationError):
    """The claimed LogUp sums of the components do not add up to the expected total (Rust: the sum check of a LogUp relation)."""

    def __init__(self, details: str = ""):
        super().__init__("The claimed LogUp sums do not add up" + (f": {details}" if details else ""))


class InvalidOodsSampleStructure(Exception):
    pass


@dataclass
class StarkProof:
    """StarkProof<H>: the commitment scheme's proof (the composition tree is the last one)."""
    commitment_scheme_proof: CommitmentSchemeProof

    def __getattr__(self, name):
        if name == "commitment_scheme_proof":
            raise AttributeError(name)
        return getattr(self.commitment_scheme_proof, name)

    def extract_composition_oods_eval(self) -> QM31:
        """The composition polynomial's value at the OODS point from the 4 sampled coordinate values of the last tree."""
        sv = self.commitment_scheme_proof.sampled_values
        if not sv:
            raise InvalidOodsSampleStructure()
        cols = sv[-1]
        if len(cols) != SECURE_EXTENSION_DEGREE or any(len(c) != 1 for c in cols):
            raise InvalidOodsSampleStructure()
        return QM31.from_partial_evals([c[0] for c in cols])


def _sample_points(components: Components, oods_point: CirclePoint) -> list:
    pts = components.mask_points(oods_point)
    pts.append([[oods_point] for _ in range(SECURE_EXTENSION_DEGREE)])
    return pts


def _uses_logup(components) -> bool:
    return any(getattr(c, "n_interaction_columns", 0) for c in components)


def prove(components, channel, commitment_scheme) -> StarkProof:
    """components: FrameworkComponents whose trace trees (preprocessed, main, and the interaction tree when a component uses
    LogUp: logup.py's caller protocol) are already committed in `commitment_scheme` (a CommitmentSchemeProver).  Raises
    ConstraintsNotSatisfied when the trace breaks a constraint."""
    trace = Trace.of(commitment_scheme)
    if _uses_logup(components) and len(trace.polys) != 3:
        raise ValueError(f"LogUp components need 3 committed trace trees (preprocessed, main, interaction), not {len(trace.polys)}")
    # the preprocessed tree's width from the commitment scheme (Rust prove; the reference's prover/index.ts:606)
    provers = ComponentProvers(components, len(trace.polys[0]) if trace.polys else 0)
    random_coeff = channel.draw_felt()
    # composition polynomial, committed as one tree of its 4 coordinate polynomials
    composition = provers.compute_composition_polynomial(random_coeff, trace, commitment_scheme.twiddles)
    tree_builder = commitment_scheme.tree_builder()
    tree_builder.extend_polys(composition.into_coordinate_polys())
    tree_builder.commit(channel)
    oods_point = CirclePoint.get_random_point(channel)
    comps = provers.components()
    proof = StarkProof(commitment_scheme.prove_values(_sample_points(comps, oods_point), channel))
    # sanity check: the sampled composition value against the constraints at the OODS point
    if proof.extract_composition_oods_eval() != comps.eval_composition_polynomial_at_point(oods_point, proof.sampled_values, random_coeff):
        raise ConstraintsNotSatisfied()
    return proof


def verify(components, channel, commitment_scheme_verifier, proof: StarkProof, logup_sum: QM31 = QM31.zero()) -> None:
    """components: the same component descriptions the prover used; commitment_scheme_verifier already holds the trace trees'
    commitments (as the prover's channel saw them; with LogUp the interaction tree too, after the claimed sums were mixed).
    Raises InvalidLogupSum when the LogUp components' claimed sums do not add up to logup_sum (nothing is checked without a
    LogUp component), OodsNotMatching, InvalidStructure or VerificationError."""
    claimed = [c.claimed_sum for c in components if getattr(c, "claimed_sum", None) is not None]
    if claimed:
        total = QM31.zero()
        for v in claimed:
            total = total.add(v)
        if total != logup_sum:
            raise InvalidLogupSum(f"{total} != {logup_sum}")
    sizes = commitment_scheme_verifier.column_log_sizes()
    comps = Components(components, len(sizes[0]) if sizes else 0)
    random_coeff = channel.draw_felt()
    if not proof.commitments:
        raise InvalidStructure("no composition commitment")
    commitment_scheme_verifier.commit(proof.commitments[-1], [comps.composition_log_degree_bound()] * SECURE_EXTENSION_DEGREE, channel)
    oods_point = CirclePoint.get_random_point(channel)
    sample_points = _sample_points(comps, oods_point)
    try:
        composition_oods_eval = proof.extract_composition_oods_eval()
    except InvalidOodsSampleStructure:
        raise InvalidStructure("Unexpected sampled_values structure") from None
    if len(proof.sampled_values) != len(sample_points) or any(
            len(tv) != len(tp) or any(len(cv) != len(cp) for cv, cp in zip(tv, tp)) for tv, tp in zip(proof.sampled_values, sample_points)):
        raise InvalidStructure("Unexpected sampled_values structure")
    try:
        expected = comps.eval_composition_polynomial_at_point(oods_point, proof.sampled_values, random_coeff)
    except (IndexError, ValueError):
        raise InvalidStructure("Unexpected sampled_values structure") from None
    if composition_oods_eval != expected:
        raise OodsNotMatching()
    commitment_scheme_verifier.verify_values(sample_points, proof.commitment_scheme_proof, channel)

"""prove / verify of a set of AIR components (Rust stwo prover/mod.rs; the reference's prover/index.ts has the shapes, but its
OODS point is QM31.zero() and its components are stubs, so nothing there produces a proof).

Default "rust" semantics only: there is no working TS prove() to be transcript-compatible with.

prove: draw alpha -> composition polynomial on the device (air.ComponentProvers) -> commit its 4 coordinate polynomials as one
tree -> draw the OODS point -> prove_values on the mask points plus the composition tree's [[oods]] * 4 -> sanity check that the
composition value from the sampled coordinates equals the one the constraints give at the OODS point.  Between drawing alpha and
the composition root, nothing is read back from the device."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

from .air import INTERACTION_TRACE_IDX, ORIGINAL_TRACE_IDX, PREPROCESSED_TRACE_IDX, ComponentProvers, Components, Trace
from .circle import CanonicCoset, CirclePoint
from .constraint_framework import ConstraintFailure
from .fields import QM31
from .pcs import CommitmentSchemeProof
from .pcs_verifier import VerificationError
from .poly import evaluate_polynomials

SECURE_EXTENSION_DEGREE = 4


class ConstraintsNotSatisfied(Exception):
    """ProvingError::ConstraintsNotSatisfied."""

    def __init__(self, msg: str = "Constraints not satisfied."):
        super().__init__(msg)


class ConstraintViolation(ConstraintsNotSatisfied):
    """ConstraintsNotSatisfied with the place: `component` (its index among the components proved, None from
    FrameworkComponent.assert_constraints), `constraint` (add_constraint calls in the order `evaluate` makes them), `row` (the
    first failing row in coset order: the row of the trace as it was written) and `n_rows` (on how many rows it fails) of the
    first failing constraint, and `failures`, every record (constraint_failures / diagnose)."""

    def __init__(self, component, failures, total_rows: int):
        first = failures[0]
        self.component, self.failures = component, list(failures)
        self.constraint, self.n_rows, self.row = first.constraint, first.n_rows, first.first_row
        where = "" if component is None else f"component {component}: "
        super().__init__(f"{where}constraint {self.constraint} is non-zero on {self.n_rows} of {total_rows} rows, first at row {self.row}")


# one failing constraint of a proof's components (diagnose): ConstraintFailure with the component's index in front
ComponentFailure = namedtuple("ComponentFailure", "component constraint n_rows first_row")


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


def diagnose(components, commitment_scheme) -> list:
    """Which constraint of which component the committed trace breaks, on which row: ComponentFailure(component, constraint,
    n_rows, first_row) records in component and constraint order, [] for a trace that satisfies every AIR.  For every component
    the committed polynomials it reads (all three trees) are evaluated on CanonicCoset(log_size).circle_domain(), one
    evaluate_polynomials per tree, and FrameworkComponent.constraint_failures runs one check launch over them.  Needs nothing
    that `prove` does not hold."""
    trace = Trace.of(commitment_scheme)
    out = []
    for i, comp in enumerate(components):
        domain = CanonicCoset(comp.log_size).circle_domain()
        trees = [(ORIGINAL_TRACE_IDX, list(comp._columns())), (PREPROCESSED_TRACE_IDX, list(comp.preprocessed_column_indices))]
        if comp.n_interaction_columns:
            trees.append((INTERACTION_TRACE_IDX, list(comp._columns(INTERACTION_TRACE_IDX))))
        cols = [evaluate_polynomials([trace.polys[tree][ci] for ci in indices], domain, commitment_scheme.twiddles) if indices else []
                for tree, indices in trees]
        out += [ComponentFailure(i, *f) for f in comp.constraint_failures(*cols)]
    return out


_diagnose = diagnose                    # `prove` has a flag of the same name


def prove(components, channel, commitment_scheme, diagnose: bool = False) -> StarkProof:
    """components: FrameworkComponents whose trace trees (preprocessed, main, and the interaction tree when a component uses
    LogUp: logup.py's caller protocol) are already committed in `commitment_scheme` (a CommitmentSchemeProver).  Raises
    ConstraintsNotSatisfied when the trace breaks a constraint; with diagnose=True the exception is a ConstraintViolation that
    names the first failing component, constraint and row (prover.diagnose, run only after the failure), when the check finds one."""
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
        if diagnose:
            failures = _diagnose(components, commitment_scheme)
            if failures:
                first = failures[0].component
                raise ConstraintViolation(first, [ConstraintFailure(*f[1:]) for f in failures if f.component == first],
                                          1 << components[first].log_size)
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

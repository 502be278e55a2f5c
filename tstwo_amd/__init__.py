"""tstwo_amd — MI355X (gfx950) backend for tstwo's data-parallel Circle-STARK hot path.

Host-side mirror of the reference's Backend / ColumnOps / PolyOps / FriOps / MerkleOps / QuotientOps surface
over the C ABI of libtstwo_hip.so (include/tstwo_hip.h).  The product path is GPU-only: it fails loudly when
the HIP library is missing or no GPU is present, and never touches oracle/.
"""
from . import _lib  # noqa: F401
from .backend import HipBackend, HipColumn, SecureColumnByCoords, shard_columns  # noqa: F401
from .channel import Blake2sChannel, DeviceChannel, HipGrindOps, grind  # noqa: F401
from .circle import (CanonicCoset, CircleDomain, CirclePoint, CirclePointIndex, Coset, LineDomain,  # noqa: F401
                     M31_CIRCLE_GEN, SECURE_FIELD_CIRCLE_GEN, bit_reverse_index)
from .fields import CM31, M31, P, QM31  # noqa: F401
from .fri_prover import (FriCommitPlan, FriConfig, FriLayerProof, FriProof, FriProver, LinePoly, line_interpolate,  # noqa: F401
                         compute_decommitment_positions_and_witness_evals)
from .fri_verifier import (CirclePolyDegreeBound, FriVerificationError, FriVerifier, LinePolyDegreeBound,  # noqa: F401
                           SparseEvaluation, accumulate_line, compute_decommitment_positions_and_rebuild_evals)
from .gkr import (EqEvals, GkrInputClaimMismatch, GkrMultivariatePolyOracle, HipGkrOps, HipMleOps, Layer, Mle,  # noqa: F401
                  check_logup_sum, eval_mles_at_point, logup_denominators, logup_input_layer, verify_input_claims,
                  prove_batch as gkr_prove_batch)
from .gkr_lookup import (GkrStarkProof, gkr_range_check_layers, gkr_range_check_prove, gkr_range_check_stark_prove,  # noqa: F401
                         gkr_range_check_stark_verify, gkr_range_check_verify)
from .gkr_verifier import (Gate, GkrArtifact, GkrBatchProof, GkrError, GkrErrorType, GkrMask,  # noqa: F401
                           partially_verify_batch)
from .sumcheck import SumcheckError, SumcheckProof, UnivariatePoly  # noqa: F401
from .queries import Queries, get_query_positions_by_log_size  # noqa: F401
from .fri_sharded import ShardedFriLayer, fri_commit_row_sharded  # noqa: F401
from .fri import HipFriOps, decompose, fold_circle_into_line, fold_line  # noqa: F401
from .pcs import (CommitmentSchemeProof, CommitmentSchemeProver, CommitmentTreeProver, PcsConfig, PointSample,  # noqa: F401
                  TreeBuilder, column_sample_batches, compute_fri_quotients)
from .pcs_verifier import (CommitmentSchemeVerifier, VerificationError, accumulate_row_quotients,  # noqa: F401
                           fri_answers)
from .poly import (CosetSubEvaluation, HipCircleEvaluation, HipCirclePoly, LineEvaluation, SecureCirclePoly, SecureEvaluation, TwiddleTree,
                   domain_line_twiddles_from_tree, get_twiddle_dbls,  # noqa: F401
                   evaluate_polynomials, interpolate_columns, precompute_twiddles)
from .quotients import (ColumnSampleBatch, accumulate, accumulateQuotients, generate_secure_powers,  # noqa: F401
                        quotientConstants)
from .vcs import (Blake2sMerkleChannel, Blake2sMerkleHasher, DeviceHashLayer, HipMerkleOps, MerkleDecommitment,  # noqa: F401
                  MerkleProver, MerkleVerifier)
from .poseidon import (DeviceFeltLayer, DevicePoseidon252Channel, FieldElement252, HipPoseidon252MerkleOps, Poseidon252Channel,  # noqa: F401
                       Poseidon252MerkleChannel, Poseidon252MerkleHasher, Poseidon252MerkleProver)
from .air import (ColumnAccumulator, ComponentProvers, Components, DomainEvaluationAccumulator,  # noqa: F401
                  PointEvaluationAccumulator, Trace, TraceLocationAllocator, coset_vanishing, generate_wide_fib_trace)
from .constraint_framework import (FrameworkComponent, MulAddComponent, MulAddEval, PermutationEval,  # noqa: F401
                                   RangeCheckTableEval, RangeCheckValuesEval, RelationEvaluator, StateMachineEval,
                                   WideFibonacciComponent, WideFibonacciEval, XorTableEval, XorValuesEval, compile_columns,
                                   evaluate_columns, state_machine_trace, xor_multiplicities_device, xor_table_columns)
from .logup import (INTERACTION_TRACE_IDX, LogupColGenerator, LogupTraceGenerator, LookupElements, LookupGroup,  # noqa: F401
                    RelationEntry, coset_iota, derive_interaction_trace, deriveInteractionTrace, lookup_multiplicities,
                    lookup_multiplicities_keyed)
from .prover import (ConstraintsNotSatisfied, ConstraintViolation, InvalidLogupSum, InvalidStructure, OodsNotMatching,  # noqa: F401
                     StarkProof, diagnose, prove, verify)
from .mle_eval import (MleEvalEval, MleEvalForm, batched_form, mle_eval_constants, mle_eval_interaction_trace,  # noqa: F401
                       mle_eval_selector_columns, mle_eval_terms)

__all__ = [n for n in dir() if not n.startswith("_")]
from .semantics import get_semantics, set_semantics  # noqa: F401,E402

"""AIR accumulators, component sets and the composition polynomial on the device.

Follows Rust stwo's air/accumulation.rs and air/components.rs, which the reference carries as shapes in air/accumulator.ts and
air/components.ts (their logic there is stubbed).  The components themselves are constraint_framework.FrameworkComponents (wide
Fibonacci and mul-add included); this module holds what every component shares: the point and domain accumulators, the vanishing
polynomial and the denominators, trace locations, and the verifier's and prover's views of a component set.  The domain
accumulator's finalize chains existing device entries (evaluate, accumulate, interpolate); nothing is read back to the host on the
prover side.  evaluate_constraint_quotients wraps the hand-written constraint kernel (TSTWO_AIR_*), generate_wide_fib_trace the
wide Fibonacci trace generator.  air.WideFibonacciComponent and air.MulAddComponent still resolve, to the functions of
constraint_framework."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .backend import HipColumn, SecureColumnByCoords
from .circle import CanonicCoset, CirclePoint, Coset, bit_reverse_index
from .fields import M31, QM31
from .poly import (HipCircleEvaluation, HipCirclePoly, SecureCirclePoly, TwiddleTree, evaluate_polynomials, interpolate_columns,
                   precompute_twiddles)
from .logup import INTERACTION_TRACE_IDX  # noqa: F401  (the third tree index, beside the two below)
from .quotients import generate_secure_powers

PREPROCESSED_TRACE_IDX = 0
ORIGINAL_TRACE_IDX = 1
# TSTWO_AIR_* of include/tstwo_hip.h
AIR_WIDE_FIB, AIR_MUL_ADD = 0, 1


# ------------------------------------------------------------------ vanishing polynomial (constraints.ts:34, constraints.rs)
def _lift(p: CirclePoint) -> CirclePoint:
    return CirclePoint(QM31.from_(p.x), QM31.from_(p.y))


def _double_x(x, one):
    return x.square().double().sub(one)


def coset_vanishing(coset: Coset, p: CirclePoint):
    """coset_vanishing: zero exactly on `coset`.  p may have M31 or QM31 coordinates (the result has the same field)."""
    secure = isinstance(p.x, QM31)
    init, half = coset.initial, coset.step_size.half().to_point()
    if secure:
        init, half = _lift(init), _lift(half)
    x = p.add(init.conjugate()).add(half).x
    one = QM31.one() if secure else M31.one()
    for _ in range(1, coset.log_size):
        x = _double_x(x, one)
    return x


def denominator_inverses(trace_log_size: int, eval_log_size: int) -> list:
    """The 2^log_expand M31 values 1 / coset_vanishing(trace coset, eval_domain.at(j)), bit-reversed (component.rs)."""
    trace_coset = CanonicCoset(trace_log_size).coset
    eval_domain = CanonicCoset(eval_log_size).circleDomain()
    log_expand = eval_log_size - trace_log_size
    vals = [coset_vanishing(trace_coset, eval_domain.at(j)).inverse() for j in range(1 << log_expand)]
    return [vals[bit_reverse_index(j, log_expand)] for j in range(1 << log_expand)]


# ------------------------------------------------------------------ accumulators (air/accumulation.rs)
class PointEvaluationAccumulator:
    """Horner accumulation of the constraint evaluations at one point: acc = acc * alpha + e."""

    def __init__(self, random_coeff: QM31):
        self.random_coeff, self.accumulation = random_coeff, QM31.zero()

    def accumulate(self, evaluation: QM31) -> None:
        self.accumulation = self.accumulation.mul(self.random_coeff).add(evaluation)

    def finalize(self) -> QM31:
        return self.accumulation


class ColumnAccumulator:
    """One component's share of a DomainEvaluationAccumulator: its coefficient powers (already reversed: constraint i gets
    random_coeff_powers[i]) and the sub-accumulation of its evaluation domain's size."""

    def __init__(self, random_coeff_powers: list, col: SecureColumnByCoords, log_size: int):
        self.random_coeff_powers, self.col, self.log_size = random_coeff_powers, col, log_size


class DomainEvaluationAccumulator:
    """Accumulates the constraint quotients of every component over their evaluation domains, one device SecureColumnByCoords per
    log size; finalize() combines them into the composition polynomial."""

    def __init__(self, random_coeff: QM31, max_log_size: int, total_constraints: int):
        self.random_coeff_powers = generate_secure_powers(random_coeff, total_constraints)
        self.max_log_size = max_log_size
        self.sub_accumulations = {}

    @staticmethod
    def new(random_coeff: QM31, max_log_size: int, total_constraints: int) -> "DomainEvaluationAccumulator":
        return DomainEvaluationAccumulator(random_coeff, max_log_size, total_constraints)

    def log_size(self) -> int:
        return self.max_log_size

    def columns(self, n_cols_per_size) -> list:
        """[(log_size, n_constraints)] -> one ColumnAccumulator each.  The powers are split off the top of the remaining list and
        reversed, so the first component's first constraint gets the highest power (Rust `split_off` + `reverse`)."""
        out = []
        for log_size, n in n_cols_per_size:
            if n > len(self.random_coeff_powers) or log_size > self.max_log_size:
                raise ValueError("accumulator: more constraints or a larger domain than announced")
            powers = self.random_coeff_powers[len(self.random_coeff_powers) - n:]
            del self.random_coeff_powers[len(self.random_coeff_powers) - n:]
            powers.reverse()
            if log_size not in self.sub_accumulations:
                self.sub_accumulations[log_size] = SecureColumnByCoords.zeros(1 << log_size)
            out.append(ColumnAccumulator(powers, self.sub_accumulations[log_size], log_size))
        return out

    def finalize(self, twiddles: TwiddleTree | None = None) -> SecureCirclePoly:
        """Ascending log sizes: the polynomial of the sizes below is evaluated on this size's domain and added, then the sum is
        interpolated.  Returns the composition polynomial (4 coordinate polys of the largest size)."""
        if self.random_coeff_powers:
            raise ValueError("not all random coefficients were used")
        if twiddles is None:
            twiddles = precompute_twiddles(CanonicCoset(self.max_log_size).circleDomain().halfCoset)
        cur = None
        for log_size in sorted(self.sub_accumulations):
            if log_size == 0:
                continue
            values = self.sub_accumulations[log_size]
            domain = CanonicCoset(log_size).circleDomain()
            if cur is not None:
                evs = evaluate_polynomials(cur.polys, domain, twiddles)
                L.call("tstwo_secure_accumulate", values.ptrs(), L.p4([e.values.ptr for e in evs]), values.len())
            cur = SecureCirclePoly(interpolate_columns([HipCircleEvaluation(domain, c) for c in values.columns], twiddles))
        if cur is None:
            return SecureCirclePoly([HipCirclePoly(HipColumn(np.zeros(1, dtype=np.uint32))) for _ in range(4)])
        return cur


# ------------------------------------------------------------------ trace locations and the committed trace
class TraceLocationAllocator:
    """Consecutive column ranges per tree, in allocation order, so that several components share one trace tree."""

    def __init__(self):
        self.next_tree_offsets = {}

    def next_for_structure(self, n_columns_per_tree: dict) -> dict:
        """{tree: n_columns} -> {tree: (col_start, col_end)}."""
        out = {}
        for tree, n in n_columns_per_tree.items():
            start = self.next_tree_offsets.get(tree, 0)
            self.next_tree_offsets[tree] = start + n
            out[tree] = (start, start + n)
        return out


class Trace:
    """The prover's committed trace: per tree, the polynomials and their committed evaluations (Rust air::Trace)."""

    def __init__(self, polys: list, evals: list):
        self.polys, self.evals = polys, evals

    @staticmethod
    def of(commitment_scheme) -> "Trace":
        return Trace(commitment_scheme.polynomials(), commitment_scheme.evaluations())


# ------------------------------------------------------------------ the hand-written constraint kernel, the wide Fibonacci trace
def evaluate_constraint_quotients(kind: int, cols, trace_log_size: int, log_expand: int, coeffs, denom_inv, accum: SecureColumnByCoords) -> None:
    """tstwo_air_constraint_quotients: accum[r] += sum_i coeffs[i] c_i(r) * denom_inv[r >> trace_log_size] over the trace `cols` on
    the evaluation domain of log size trace_log_size + log_expand (bit-reversed)."""
    words = (C.c_uint32 * max(4 * len(coeffs), 4))(*[w for c in coeffs for w in c.tup()])
    dinv = L.u32x([d.value if isinstance(d, M31) else int(d) for d in denom_inv])
    L.call("tstwo_air_constraint_quotients", kind, L.ptr_array([c.ptr for c in cols]), len(cols), trace_log_size, log_expand,
           words, len(coeffs), dinv, accum.ptrs())


def generate_wide_fib_trace(log_n: int, a, b, n_columns: int = 100) -> list:
    """generateTrace (examples/fibonacci.ts) on the device: columns x_0 = a, x_1 = b, x_k = x_{k-2}^2 + x_{k-1}^2, each of 2^log_n
    values (a, b: HipColumn or arrays).  Returns HipCircleEvaluations on CanonicCoset(log_n).circle_domain() (bit-reversed order)."""
    a = a if isinstance(a, HipColumn) else HipColumn(a)
    b = b if isinstance(b, HipColumn) else HipColumn(b)
    if a.len() != 1 << log_n or b.len() != 1 << log_n:
        raise ValueError("a and b must have 2^log_n values")
    cols = [HipColumn.uninitialized(1 << log_n) for _ in range(n_columns)]
    L.call("tstwo_air_wide_fib_trace", C.c_void_p(a.ptr), C.c_void_p(b.ptr), log_n, L.ptr_array([c.ptr for c in cols]), n_columns)
    domain = CanonicCoset(log_n).circleDomain()
    return [HipCircleEvaluation(domain, c) for c in cols]


def __getattr__(name):
    """air.WideFibonacciComponent / air.MulAddComponent, where callers found them before: the functions of constraint_framework
    (imported on first use, since constraint_framework imports this module)."""
    if name in ("WideFibonacciComponent", "MulAddComponent"):
        from . import constraint_framework
        return getattr(constraint_framework, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ------------------------------------------------------------------ component sets (air/components.rs)
def _concat_cols(trees_list: list) -> list:
    out = []
    for trees in trees_list:
        for t, cols in enumerate(trees):
            while len(out) <= t:
                out.append([])
            out[t] += cols
    return out


class Components:
    """The verifier's view of a set of components.  n_preprocessed_columns: the width of the preprocessed tree (tree 0).  Each of
    its columns that some component names (`preprocessed_column_indices`) is sampled once, at [point], whichever components read
    it; the others get no sample (Rust air/components.rs)."""

    def __init__(self, components, n_preprocessed_columns: int = 0):
        self.components = list(components)
        self.n_preprocessed_columns = n_preprocessed_columns
        for c in self.components:
            for idx in c.preprocessed_column_indices:
                if not 0 <= idx < n_preprocessed_columns:
                    raise ValueError(f"preprocessed column {idx} out of range (the preprocessed tree has {n_preprocessed_columns})")

    def composition_log_degree_bound(self) -> int:
        return max(c.max_constraint_log_degree_bound() for c in self.components)

    def mask_points(self, point: CirclePoint) -> list:
        """TreeVec of per-column sample points, the components' columns concatenated per tree (preprocessed tree 0 included)."""
        pts = _concat_cols([c.mask_points(point) for c in self.components])
        while len(pts) <= ORIGINAL_TRACE_IDX:
            pts.append([])
        if self.n_preprocessed_columns or any(c.preprocessed_column_indices for c in self.components):
            pre = [[] for _ in range(self.n_preprocessed_columns)]
            for c in self.components:
                for idx in c.preprocessed_column_indices:
                    pre[idx] = [point]
            pts[PREPROCESSED_TRACE_IDX] = pre
        return pts

    def column_log_sizes(self) -> list:
        sizes = _concat_cols([c.trace_log_degree_bounds() for c in self.components])
        while len(sizes) <= ORIGINAL_TRACE_IDX:
            sizes.append([])
        if self.n_preprocessed_columns or any(c.preprocessed_column_indices for c in self.components):
            pre, seen = [0] * self.n_preprocessed_columns, set()
            for c in self.components:
                for idx, lg in zip(c.preprocessed_column_indices, c.trace_log_degree_bounds()[PREPROCESSED_TRACE_IDX]):
                    if idx in seen and pre[idx] != lg:
                        raise ValueError(f"preprocessed column {idx} read with two log sizes ({pre[idx]} and {lg})")
                    pre[idx] = lg
                    seen.add(idx)
            sizes[PREPROCESSED_TRACE_IDX] = pre
        return sizes

    def eval_composition_polynomial_at_point(self, point: CirclePoint, mask_values: list, random_coeff: QM31) -> QM31:
        acc = PointEvaluationAccumulator(random_coeff)
        for c in self.components:
            c.evaluate_constraint_quotients_at_point(point, mask_values, acc)
        return acc.finalize()


class ComponentProvers:
    """The prover's view: Components plus the composition polynomial on the device."""

    def __init__(self, components, n_preprocessed_columns: int = 0):
        self.component_provers = list(components)
        self.n_preprocessed_columns = n_preprocessed_columns

    def components(self) -> Components:
        return Components(self.component_provers, self.n_preprocessed_columns)

    def compute_composition_polynomial(self, random_coeff: QM31, trace: Trace, twiddles: TwiddleTree) -> SecureCirclePoly:
        total = sum(c.n_constraints for c in self.component_provers)
        acc = DomainEvaluationAccumulator.new(random_coeff, self.components().composition_log_degree_bound(), total)
        for c in self.component_provers:
            c.evaluate_constraint_quotients_on_domain(trace, acc, twiddles)
        return acc.finalize(twiddles)

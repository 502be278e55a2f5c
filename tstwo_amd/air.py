"""AIR components and the composition polynomial on the device.

Follows Rust stwo's air/accumulation.rs, air/components.rs and constraint_framework/component.rs, which the reference carries as
shapes in air/accumulator.ts, air/components.ts and constraint_framework/index.ts (their logic there is stubbed).  Two constraint
kinds are supported, both reading only their own row (mask offset 0):
  WideFibonacciComponent  examples/fibonacci.ts WideFibonacciEval: c_i = x_{i+2} - (x_i^2 + x_{i+1}^2)
  MulAddComponent         TestEval of the Rust tutorial's example 05: c = x_0 x_1 + x_0 - x_2
The verifier side (evaluate_constraint_quotients_at_point) is host QM31 code; the prover side evaluates every row of the
evaluation domain in one tstwo_air_constraint_quotients launch per component, and the domain accumulator's finalize chains existing
device entries (evaluate, accumulate, interpolate).  Nothing is read back to the host on the prover side."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .backend import HipColumn, SecureColumnByCoords
from .circle import CanonicCoset, CirclePoint, Coset, bit_reverse_index
from .fields import M31, QM31
from .poly import (HipCircleEvaluation, HipCirclePoly, SecureCirclePoly, TwiddleTree, evaluate_polynomials, interpolate_columns,
                   precompute_twiddles)
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


# ------------------------------------------------------------------ components
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


class FrameworkComponent:
    """A component whose constraints read only their own row of `n_columns` main-trace columns of log size `log_size`, with
    constraint degree 2 (max_constraint_log_degree_bound = log_size + 1).  Subclasses give `kind` (TSTWO_AIR_*), `n_columns`,
    `n_constraints` and `constraints_at(values)` (the host form, for the verifier)."""

    kind = None
    LOG_CONSTRAINT_DEGREE = 1

    def __init__(self, location_allocator: TraceLocationAllocator | None, log_size: int, n_columns: int, n_constraints: int):
        if log_size < 1:
            raise ValueError("log_size must be at least 1")
        self.log_size, self.n_columns, self.n_constraints = log_size, n_columns, n_constraints
        alloc = location_allocator or TraceLocationAllocator()
        self.trace_locations = alloc.next_for_structure({ORIGINAL_TRACE_IDX: n_columns})

    # --- Component
    def max_constraint_log_degree_bound(self) -> int:
        return self.log_size + self.LOG_CONSTRAINT_DEGREE

    def trace_log_degree_bounds(self) -> list:
        """TreeVec of column log sizes: the (empty) preprocessed tree, then this component's main-trace columns."""
        return [[], [self.log_size] * self.n_columns]

    def mask_points(self, point: CirclePoint) -> list:
        return [[], [[point] for _ in range(self.n_columns)]]

    def _columns(self) -> range:
        start, end = self.trace_locations[ORIGINAL_TRACE_IDX]
        return range(start, end)

    def evaluate_constraint_quotients_at_point(self, point: CirclePoint, mask: list, acc: PointEvaluationAccumulator) -> None:
        """PointEvaluator: each constraint at the OODS point times 1 / coset_vanishing(trace coset, point), in constraint order."""
        denom_inv = coset_vanishing(CanonicCoset(self.log_size).coset, point).inverse()
        values = []
        for ci in self._columns():
            col = mask[ORIGINAL_TRACE_IDX][ci]
            if len(col) != 1:
                raise ValueError("one sampled value per column expected")
            values.append(col[0])
        for c in self.constraints_at(values):
            acc.accumulate(c.mul(denom_inv))

    def constraints_at(self, values: list) -> list:
        raise NotImplementedError

    # --- ComponentProver
    def trace_on_eval_domain(self, trace: Trace, twiddles: TwiddleTree) -> list:
        """This component's columns on CanonicCoset(max_constraint_log_degree_bound).circle_domain(): the committed evaluation when
        it already lives there (log blowup 1), else the polynomials evaluated there (one batched launch sequence)."""
        eval_domain = CanonicCoset(self.max_constraint_log_degree_bound()).circleDomain()
        cols, missing = [], []
        for ci in self._columns():
            ev = trace.evals[ORIGINAL_TRACE_IDX][ci]
            if ev.domain == eval_domain:
                cols.append(ev.values)
            else:
                cols.append(None)
                missing.append(len(cols) - 1)
        if missing:
            polys = [trace.polys[ORIGINAL_TRACE_IDX][self._columns()[k]] for k in missing]
            for k, ev in zip(missing, evaluate_polynomials(polys, eval_domain, twiddles)):
                cols[k] = ev.values
        return cols

    def evaluate_constraint_quotients_on_domain(self, trace: Trace, acc: DomainEvaluationAccumulator, twiddles: TwiddleTree) -> None:
        eval_log = self.max_constraint_log_degree_bound()
        cols = self.trace_on_eval_domain(trace, twiddles)
        [column_acc] = acc.columns([(eval_log, self.n_constraints)])
        evaluate_constraint_quotients(self.kind, cols, self.log_size, eval_log - self.log_size, column_acc.random_coeff_powers,
                                      denominator_inverses(self.log_size, eval_log), column_acc.col)


def evaluate_constraint_quotients(kind: int, cols, trace_log_size: int, log_expand: int, coeffs, denom_inv, accum: SecureColumnByCoords) -> None:
    """tstwo_air_constraint_quotients: accum[r] += sum_i coeffs[i] c_i(r) * denom_inv[r >> trace_log_size] over the trace `cols` on
    the evaluation domain of log size trace_log_size + log_expand (bit-reversed)."""
    words = (C.c_uint32 * max(4 * len(coeffs), 4))(*[w for c in coeffs for w in c.tup()])
    dinv = L.u32x([d.value if isinstance(d, M31) else int(d) for d in denom_inv])
    L.call("tstwo_air_constraint_quotients", kind, L.ptr_array([c.ptr for c in cols]), len(cols), trace_log_size, log_expand,
           words, len(coeffs), dinv, accum.ptrs())


class WideFibonacciComponent(FrameworkComponent):
    """WideFibonacciEval<N> (examples/fibonacci.ts): N columns, N - 2 constraints x_{i+2} = x_i^2 + x_{i+1}^2."""

    kind = AIR_WIDE_FIB

    def __init__(self, log_n_rows: int, n_columns: int = 100, location_allocator: TraceLocationAllocator | None = None):
        if n_columns < 3:
            raise ValueError("wide Fibonacci needs at least 3 columns")
        super().__init__(location_allocator, log_n_rows, n_columns, n_columns - 2)

    def constraints_at(self, v: list) -> list:
        return [v[i + 2].sub(v[i].square().add(v[i + 1].square())) for i in range(self.n_columns - 2)]


class MulAddComponent(FrameworkComponent):
    """TestEval of the Rust tutorial's example 05: 3 columns, x_0 x_1 + x_0 - x_2 = 0."""

    kind = AIR_MUL_ADD

    def __init__(self, log_n_rows: int, location_allocator: TraceLocationAllocator | None = None):
        super().__init__(location_allocator, log_n_rows, 3, 1)

    def constraints_at(self, v: list) -> list:
        return [v[0].mul(v[1]).add(v[0]).sub(v[2])]


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
            for idx in getattr(c, "preprocessed_column_indices", ()):
                if not 0 <= idx < n_preprocessed_columns:
                    raise ValueError(f"preprocessed column {idx} out of range (the preprocessed tree has {n_preprocessed_columns})")

    def composition_log_degree_bound(self) -> int:
        return max(c.max_constraint_log_degree_bound() for c in self.components)

    def mask_points(self, point: CirclePoint) -> list:
        """TreeVec of per-column sample points, the components' columns concatenated per tree (preprocessed tree 0 included)."""
        pts = _concat_cols([c.mask_points(point) for c in self.components])
        while len(pts) <= ORIGINAL_TRACE_IDX:
            pts.append([])
        if self.n_preprocessed_columns or any(getattr(c, "preprocessed_column_indices", ()) for c in self.components):
            pre = [[] for _ in range(self.n_preprocessed_columns)]
            for c in self.components:
                for idx in getattr(c, "preprocessed_column_indices", ()):
                    pre[idx] = [point]
            pts[PREPROCESSED_TRACE_IDX] = pre
        return pts

    def column_log_sizes(self) -> list:
        sizes = _concat_cols([c.trace_log_degree_bounds() for c in self.components])
        while len(sizes) <= ORIGINAL_TRACE_IDX:
            sizes.append([])
        if self.n_preprocessed_columns or any(getattr(c, "preprocessed_column_indices", ()) for c in self.components):
            pre, seen = [0] * self.n_preprocessed_columns, set()
            for c in self.components:
                for idx, lg in zip(getattr(c, "preprocessed_column_indices", ()), c.trace_log_degree_bounds()[PREPROCESSED_TRACE_IDX]):
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

"""The constraint framework: every AIR component (Rust stwo constraint_framework/: FrameworkEval, EvalAtRow, InfoEvaluator,
PointEvaluator, FrameworkComponent; the reference carries the shapes in constraint_framework/index.ts).

A component is a FrameworkComponent of an eval, an object with `log_size()`, `max_constraint_log_degree_bound()` and one
`evaluate(eval)` function.  Three evaluators drive it:
  InfoEvaluator     the mask offsets of each column, the number of constraints and the degree of each;
  ProgramEvaluator  the constraints as a straight-line program for tstwo_air_eval_program (include/tstwo_hip.h): identical loads
                    (same column and offset) and identical sub-expressions are computed once, registers are reused after their
                    last use, and the number of live registers is bounded by MAX_REGS;
  PointEvaluator    the constraints over QM31 at the out-of-domain point (the verifier, and the prover's sanity check).
A fourth, RelationEvaluator, keeps the relation entries of `evaluate` as they were added (relation, multiplicity, values) and
their batching: logup.derive_interaction_trace builds the interaction trace from them, with compile_columns / evaluate_columns
(tstwo_air_eval_columns; with native=True a kernel compiled from the columns program, compile_columns_native /
tstwo_air_eval_columns_compiled) for every multiplicity or value that is an expression of columns.
check_program (tstwo_air_check_constraints) runs a constraint program on the TRACE domain and reports, per constraint, on how many
rows it is non-zero and the first of them in coset order; FrameworkComponent.constraint_failures / assert_constraints drive it
(Rust stwo assert_constraints_on_trace), prover.diagnose does so for a committed trace.
The prover evaluates a component's constraints on the whole evaluation domain with one launch: WideFibonacciEval and MulAddEval
(exactly these types, not subclasses) run on the hand-written kernel of tstwo_air_constraint_quotients, every other eval on the
program interpreter or, for a FrameworkComponent made with native=True, on a kernel compiled from the program at construction
(compile_native, tstwo_air_program_compile).  WideFibonacciComponent and MulAddComponent are FrameworkComponents of those two evals, as in Rust.

The main trace (ORIGINAL_TRACE_IDX) is read at row offsets; preprocessed columns are read at offset 0 (as in Rust).  LogUp
(tstwo_amd/logup.py, Rust logup.rs): add_to_relation / finalize_logup_* read the interaction trace (INTERACTION_TRACE_IDX, 4 base
columns per secure column, the last one at offsets -1 and 0) and add secure-field (QM31) constraints.  The program path lowers a
secure value to its 4 base coordinates (SecureExpr): a secure constraint is 4 ACCs whose coefficients are c, c i, c u, c iu for
its random coefficient c, so the interpreter and its program encoding stay base-field.  The interaction trace itself is built on
the device by logup.LogupTraceGenerator, written by hand or derived from `evaluate` (logup.derive_interaction_trace).
"""
from __future__ import annotations

import bisect
import ctypes as C
import time
from collections import namedtuple

from . import _lib as L
from .air import (AIR_MUL_ADD, AIR_WIDE_FIB, ORIGINAL_TRACE_IDX, PREPROCESSED_TRACE_IDX, DomainEvaluationAccumulator,
                  PointEvaluationAccumulator, TraceLocationAllocator, coset_vanishing, denominator_inverses,
                  evaluate_constraint_quotients, _lift)
from .backend import SecureColumnByCoords
from .circle import CanonicCoset, CirclePoint, bit_reverse_index
from .fields import M31, QM31, P
from .logup import INTERACTION_TRACE_IDX, LogupTraceGenerator, LookupElements, RelationEntry
from .poly import evaluate_polynomials

# include/tstwo_hip.h TSTWO_AIR_OP_* and TSTWO_AIR_PROGRAM_MAX_*
OP_LOAD, OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_NEG, OP_ACC, OP_STORE = range(9)
MAX_INSTR, MAX_REGS, MAX_CONSTRAINTS, MAX_COLS, MAX_OFFSET = 1536, 32, 256, 4096, 64
MAX_OUT = 64                            # TSTWO_AIR_COLUMNS_MAX_OUT
MAX_LOG_EXPAND = 4


# ------------------------------------------------------------------ row offsets (utils.rs offset_bit_reversed_circle_domain_index)
def offset_bit_reversed_circle_domain_index(i: int, domain_log_size: int, eval_log_size: int, offset: int) -> int:
    """The bit-reversed position, on CanonicCoset(eval_log_size).circle_domain(), of the point `offset` steps of
    CanonicCoset(domain_log_size) away from the point at bit-reversed position i.  Needs eval_log_size > domain_log_size."""
    if eval_log_size <= domain_log_size:
        raise ValueError("the evaluation domain must be larger than the trace domain")
    prev = bit_reverse_index(i, eval_log_size)
    half = 1 << (eval_log_size - 1)
    step = offset * (1 << (eval_log_size - domain_log_size - 1))
    if prev < half:
        prev = (prev + step) % half
    else:
        prev = (prev - step) % half + half
    return bit_reverse_index(prev, eval_log_size)


offsetBitReversedCircleDomainIndex = offset_bit_reversed_circle_domain_index


def shifted_mask_point(point: CirclePoint, log_size: int, offset: int) -> CirclePoint:
    """point + CanonicCoset(log_size).step * offset (mask.ts shiftedMaskPoints, Rust component.rs mask_points)."""
    if offset == 0:
        return point
    return point.add(_lift(CanonicCoset(log_size).step_size().mul(offset).to_point()))


# ------------------------------------------------------------------ symbolic values (Info and Program evaluators)
class Expr:
    """A node of the constraint DAG: ('load', (column, offset)), ('const', value) or an operation on other nodes.  `column` is
    ('main', k) for the k-th main-trace mask column or ('pre', i) for the component's i-th preprocessed column."""

    __slots__ = ("op", "args", "key", "degree")

    def __init__(self, op, args, key, degree):
        self.op, self.args, self.key, self.degree = op, args, key, degree

    @staticmethod
    def load(column, offset):
        return Expr("load", (column, offset), ("load", column, offset), 1)

    @staticmethod
    def const(v: int):
        v = int(v) % P
        return Expr("const", v, ("const", v), 0)

    @staticmethod
    def _lift(o):
        if isinstance(o, Expr):
            return o
        if isinstance(o, M31):
            return Expr.const(o.value)
        if isinstance(o, int):
            return Expr.const(o)
        raise TypeError(f"constraint values mix with Python ints and M31 only, not {type(o).__name__}")

    def _bin(self, op, o, swap=False):
        a, b = (Expr._lift(o), self) if swap else (self, Expr._lift(o))
        deg = a.degree + b.degree if op == "mul" else max(a.degree, b.degree)
        return Expr(op, (a, b), (op, id(a), id(b)), deg)

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __neg__(self): return Expr("neg", (self,), ("neg", id(self)), self.degree)

    def square(self):
        return Expr("sqr", (self,), ("sqr", id(self)), 2 * self.degree)


class PointValue:
    """A QM31 value at the out-of-domain point, with the operators of Expr (PointEvaluator)."""

    __slots__ = ("v",)

    def __init__(self, v: QM31):
        self.v = v

    @staticmethod
    def _q(o):
        if isinstance(o, PointValue):
            return o.v
        if isinstance(o, QM31):
            return o
        if isinstance(o, M31):
            return QM31.from_(o)
        if isinstance(o, int):
            return QM31.from_(M31(int(o) % P))
        raise TypeError(f"constraint values mix with Python ints and M31 only, not {type(o).__name__}")

    def __add__(self, o): return PointValue(self.v.add(PointValue._q(o)))
    def __radd__(self, o): return PointValue(PointValue._q(o).add(self.v))
    def __sub__(self, o): return PointValue(self.v.sub(PointValue._q(o)))
    def __rsub__(self, o): return PointValue(PointValue._q(o).sub(self.v))
    def __mul__(self, o): return PointValue(self.v.mul(PointValue._q(o)))
    def __rmul__(self, o): return PointValue(PointValue._q(o).mul(self.v))
    def __neg__(self): return PointValue(self.v.neg())

    def square(self):
        return PointValue(self.v.square())


# ------------------------------------------------------------------ secure values of the symbolic evaluators
# A coordinate is an int (a constant) or an Expr.  These helpers fold constants 0 and 1, so that an M31 value lifted to QM31 does
# not turn into chains of x * 0; Expr itself folds nothing.
def _sadd(a, b):
    if isinstance(a, int) and isinstance(b, int):
        return (a + b) % P
    if isinstance(a, int) and a == 0:
        return b
    if isinstance(b, int) and b == 0:
        return a
    return (b + a) if isinstance(a, int) else (a + b)


def _ssub(a, b):
    if isinstance(a, int) and isinstance(b, int):
        return (a - b) % P
    if isinstance(b, int) and b == 0:
        return a
    if isinstance(a, int) and a == 0:
        return -b
    return (a - b) if isinstance(a, Expr) else (Expr.const(a) - b)


def _smul(a, b):
    if isinstance(a, int) and isinstance(b, int):
        return a * b % P
    if (isinstance(a, int) and a == 0) or (isinstance(b, int) and b == 0):
        return 0
    if isinstance(a, int) and a == 1:
        return b
    if isinstance(b, int) and b == 1:
        return a
    return (b * a) if isinstance(a, int) else (a * b)


def _sneg(a):
    return (-a) % P if isinstance(a, int) else -a


def _cmul(ar, ai, br, bi):
    """(ar + ai i)(br + bi i)."""
    return _ssub(_smul(ar, br), _smul(ai, bi)), _sadd(_smul(ar, bi), _smul(ai, br))


def _qmul(x, y):
    """QM31 product over coordinates: (x0 + x1 u)(y0 + y1 u) = x0 y0 + (2 + i) x1 y1 + (x0 y1 + x1 y0) u (u^2 = 2 + i)."""
    c0r, c0i = _cmul(x[0], x[1], y[0], y[1])
    tr, ti = _cmul(x[2], x[3], y[2], y[3])
    rr, ri = _ssub(_sadd(tr, tr), ti), _sadd(tr, _sadd(ti, ti))         # (2 + i)(tr + ti i)
    d0r, d0i = _cmul(x[0], x[1], y[2], y[3])
    d1r, d1i = _cmul(x[2], x[3], y[0], y[1])
    return (_sadd(c0r, rr), _sadd(c0i, ri), _sadd(d0r, d1r), _sadd(d0i, d1i))


class SecureExpr:
    """A secure-field (QM31) value inside the Info and Program evaluators: 4 base coordinates c (ints for constants, else Expr),
    the value c0 + c1 i + c2 u + c3 iu.  Mixes with Expr, ints, M31 and QM31 (an Expr on the left of an operator does not know
    it: write the SecureExpr first)."""

    __slots__ = ("c",)

    def __init__(self, coords):
        self.c = tuple(coords)

    @staticmethod
    def lift(o) -> "SecureExpr":
        if isinstance(o, SecureExpr):
            return o
        if isinstance(o, QM31):
            return SecureExpr(o.tup())
        if isinstance(o, M31):
            return SecureExpr((o.value, 0, 0, 0))
        if isinstance(o, int):
            return SecureExpr((int(o) % P, 0, 0, 0))
        if isinstance(o, Expr):
            return SecureExpr((o, 0, 0, 0))
        raise TypeError(f"secure constraint values mix with Expr, ints, M31 and QM31, not {type(o).__name__}")

    @property
    def degree(self) -> int:
        return max(x.degree if isinstance(x, Expr) else 0 for x in self.c)

    def coords(self) -> list:
        """The 4 coordinates as Expr nodes (constants as CONST)."""
        return [Expr.const(x) if isinstance(x, int) else x for x in self.c]

    def __add__(self, o): return SecureExpr(map(_sadd, self.c, SecureExpr.lift(o).c))
    def __radd__(self, o): return SecureExpr(map(_sadd, SecureExpr.lift(o).c, self.c))
    def __sub__(self, o): return SecureExpr(map(_ssub, self.c, SecureExpr.lift(o).c))
    def __rsub__(self, o): return SecureExpr(map(_ssub, SecureExpr.lift(o).c, self.c))
    def __mul__(self, o): return SecureExpr(_qmul(self.c, SecureExpr.lift(o).c))
    def __rmul__(self, o): return SecureExpr(_qmul(SecureExpr.lift(o).c, self.c))
    def __neg__(self): return SecureExpr(map(_sneg, self.c))

    def square(self):
        return self * self


# basis of QM31 over M31 (from_partial_evals): a secure constraint's 4 coordinates take coefficients c * (1, i, u, iu)
_BASIS = [QM31.from_u32_unchecked(*[1 if j == k else 0 for j in range(4)]) for k in range(4)]


def expand_coeffs(coeffs, secure_flags) -> list:
    """The per-ACC coefficients of a program: c for a base constraint, c * (1, i, u, iu) for a secure one."""
    out = []
    for c, secure in zip(coeffs, secure_flags):
        out += [c.mul(b) for b in _BASIS] if secure else [c]
    return out


# ------------------------------------------------------------------ EvalAtRow
def _offsets(offsets) -> list:
    offsets = [int(o) for o in offsets]
    if not offsets:
        raise ValueError("a mask needs at least one offset")
    if any(abs(o) > MAX_OFFSET for o in offsets):
        raise ValueError(f"row offsets are limited to |offset| <= {MAX_OFFSET}")
    return offsets


class EvalAtRow:
    """The surface `evaluate` sees (Rust EvalAtRow).  Subclasses produce the values.  claimed_sum and log_size give the LogUp
    shift claimed_sum / 2^log_size of finalize_logup_batched (Rust LogupAtRow)."""

    def __init__(self, claimed_sum: QM31 | None = None, log_size: int = 0):
        self.n_main = 0                 # main-trace mask columns handed out so far
        self.main_offsets = []          # offsets of each main column, in call order
        self.constraints = []
        self.n_interaction = 0          # interaction (tree 2) base columns handed out so far
        self.interaction_offsets = []   # offsets of each of them
        self.fracs = []                 # LogUp fractions (numerator, denominator) not yet finalized
        self.n_entries = 0
        self.logup_finalized = False
        claimed = claimed_sum if claimed_sum is not None else QM31.zero()
        self.cumsum_shift = claimed.mulM31(M31(1 << log_size).inverse()) if log_size else claimed

    def _value(self, column, offset):
        raise NotImplementedError

    def _secure(self, o):
        """o as this evaluator's secure value."""
        return SecureExpr.lift(o)

    def _extension_values(self, k: int, offsets) -> list:
        """The secure values of interaction columns k .. k + 3 at each offset (symbolic: the 4 loads as coordinates)."""
        return [SecureExpr([self._value(("int", k + c), o) for c in range(4)]) for o in offsets]

    def next_interaction_mask(self, interaction: int, offsets) -> list:
        if interaction == PREPROCESSED_TRACE_IDX:
            raise ValueError("preprocessed columns are read with get_preprocessed_column (offset 0 only)")
        if interaction == INTERACTION_TRACE_IDX:
            raise ValueError("the interaction trace is read with next_extension_interaction_mask (4 base columns per value)")
        if interaction != ORIGINAL_TRACE_IDX:
            raise ValueError("only the main trace (ORIGINAL_TRACE_IDX) is supported")
        offsets = _offsets(offsets)
        k = self.n_main
        self.n_main += 1
        self.main_offsets.append(offsets)
        return [self._value(("main", k), o) for o in offsets]

    def next_extension_interaction_mask(self, interaction: int, offsets) -> list:
        """One secure column of the interaction trace: 4 consecutive base columns of tree INTERACTION_TRACE_IDX read at the same
        offsets, each value QM31.from_partial_evals of the 4 (Rust next_extension_interaction_mask)."""
        if interaction != INTERACTION_TRACE_IDX:
            raise ValueError("secure columns live in the interaction trace (INTERACTION_TRACE_IDX)")
        offsets = _offsets(offsets)
        k = self.n_interaction
        self.n_interaction += 4
        self.interaction_offsets += [list(offsets) for _ in range(4)]
        return self._extension_values(k, offsets)

    def next_trace_mask(self):
        return self.next_interaction_mask(ORIGINAL_TRACE_IDX, [0])[0]

    def get_preprocessed_column(self, i: int):
        if i < 0:
            raise ValueError("negative preprocessed column index")
        return self._value(("pre", int(i)), 0)

    def add_constraint(self, expr) -> None:
        self.constraints.append(expr)

    # --- LogUp (Rust logup.rs LogupAtRow)
    def add_to_relation(self, entry: RelationEntry) -> None:
        if self.logup_finalized:
            raise ValueError("a relation entry added after finalize_logup")
        self.fracs.append((entry.multiplicity, entry.relation.combine(entry.values)))
        self.n_entries += 1

    def finalize_logup_batched(self, batching) -> None:
        """Fractions of one batch are summed (a/b + c/d = (ad + cb)/(bd), left to right) into one interaction column each.  Batch
        j before the last: column cur_j at [0], constraint (cur_j - cur_{j-1}) den_j - num_j (cur_{-1} = 0).  The last batch:
        its column at [-1, 0], constraint (cur - prev_row - cur_{last-1} + claimed_sum / 2^log_size) den - num."""
        if self.logup_finalized:
            raise ValueError("finalize_logup called twice")
        batching = [int(b) for b in batching]
        if not self.fracs:
            raise ValueError("finalize_logup without relation entries")
        if len(batching) != len(self.fracs):
            raise ValueError(f"batching names {len(batching)} entries, {len(self.fracs)} were added")
        last = max(batching)
        if sorted(set(batching)) != list(range(last + 1)):
            raise ValueError("batches must be consecutive from 0")
        self.logup_finalized = True
        sums = []
        for j in range(last + 1):
            num = den = None
            for b, (n, d) in zip(batching, self.fracs):
                if b != j:
                    continue
                n, d = self._secure(n), self._secure(d)
                if den is None:
                    num, den = n, d
                else:
                    num, den = num * d + n * den, den * d
            sums.append((num, den))
        self.fracs = []
        prev_col = self._secure(0)
        for num, den in sums[:-1]:
            [cur] = self.next_extension_interaction_mask(INTERACTION_TRACE_IDX, [0])
            self.add_constraint((cur - prev_col) * den - num)
            prev_col = cur
        num, den = sums[-1]
        prev_row, cur = self.next_extension_interaction_mask(INTERACTION_TRACE_IDX, [-1, 0])
        self.add_constraint((cur - prev_row - prev_col + self._secure(self.cumsum_shift)) * den - num)

    def finalize_logup(self) -> None:
        """One fraction per batch."""
        self.finalize_logup_batched(range(len(self.fracs)))

    def finalize_logup_in_pairs(self) -> None:
        """Batches 0, 0, 1, 1, ...: two fractions per interaction column."""
        self.finalize_logup_batched([i // 2 for i in range(len(self.fracs))])

    def check_finished(self) -> None:
        """Called after `evaluate`: relation entries must have been finalized."""
        if self.fracs and not self.logup_finalized:
            raise ValueError("evaluate added relation entries without finalize_logup")

    # camelCase aliases (the reference's names)
    nextInteractionMask = next_interaction_mask
    nextExtensionInteractionMask = next_extension_interaction_mask
    nextTraceMask = next_trace_mask
    getPreprocessedColumn = get_preprocessed_column
    addConstraint = add_constraint
    addToRelation = add_to_relation
    finalizeLogupBatched = finalize_logup_batched
    finalizeLogup = finalize_logup
    finalizeLogupInPairs = finalize_logup_in_pairs


class _SymbolicEval(EvalAtRow):
    def __init__(self, claimed_sum: QM31 | None = None, log_size: int = 0):
        super().__init__(claimed_sum, log_size)
        self.pre_used = set()

    def _value(self, column, offset):
        if column[0] == "pre":
            self.pre_used.add(column[1])
        return Expr.load(column, offset)

    def add_constraint(self, expr) -> None:
        if isinstance(expr, SecureExpr):
            self.constraints.append(SecureExpr(expr.coords()))
        else:
            self.constraints.append(Expr._lift(expr))


class InfoEvaluator(_SymbolicEval):
    """Mask offsets per column, the number of constraints and their degrees (Rust InfoEvaluator)."""

    @property
    def n_constraints(self) -> int:
        return len(self.constraints)

    def degrees(self) -> list:
        return [c.degree for c in self.constraints]

    def max_degree(self) -> int:
        return max(self.degrees(), default=0)

    def n_preprocessed(self) -> int:
        return max(self.pre_used) + 1 if self.pre_used else 0

    def secure_flags(self) -> list:
        """Per constraint: True for a secure (QM31) one, which takes 4 ACCs in the program."""
        return [isinstance(c, SecureExpr) for c in self.constraints]

    def mask_offsets(self) -> list:
        """TreeVec: per preprocessed column read, [0]; per main column, its offsets; with LogUp, per interaction column its offsets."""
        trees = [[[0] for _ in range(self.n_preprocessed())], [list(o) for o in self.main_offsets]]
        if self.n_interaction:
            trees.append([list(o) for o in self.interaction_offsets])
        return trees


def required_log_degree_bound(log_size: int, max_degree: int) -> int:
    """The smallest max_constraint_log_degree_bound that holds the quotient of a degree-d constraint: about
    (d - 1) 2^log_size + 1 coefficients, so log_size + floor(log2(d - 1)) + 1 (and at least log_size + 1)."""
    if max_degree <= 2:
        return log_size + 1
    return log_size + (max_degree - 1).bit_length() - 1 + 1


def info(eval_) -> InfoEvaluator:
    ev = InfoEvaluator()
    eval_.evaluate(ev)
    ev.check_finished()
    return ev


class ProgramEvaluator(_SymbolicEval):
    """Records the constraints, then compile() turns them into the program of tstwo_air_eval_program (a secure constraint as its 4
    coordinates, in order)."""

    def compile(self, n_main: int | None = None, n_pre: int = 0) -> "Program":
        roots = []
        for c in self.constraints:
            roots += c.coords() if isinstance(c, SecureExpr) else [c]
        return compile_program(roots, self.n_main if n_main is None else n_main, n_pre)


class RelationEvaluator(_SymbolicEval):
    """Keeps what `evaluate` says about LogUp and nothing else: per add_to_relation the raw (relation, multiplicity, values), before
    relation.combine, in `entries`; per finalize_logup_* the batch of every entry, in `batching`.  Constraints are dropped.
    Masks are handed out as every evaluator does, so an `evaluate` written for the prover runs unchanged."""

    def __init__(self):
        super().__init__()
        self.entries, self.batching = [], []

    def add_constraint(self, expr) -> None:
        pass

    def add_to_relation(self, entry: RelationEntry) -> None:
        super().add_to_relation(entry)
        self.entries.append((entry.relation, entry.multiplicity, list(entry.values)))

    def finalize_logup_batched(self, batching) -> None:
        batching = [int(b) for b in batching]
        super().finalize_logup_batched(batching)
        self.batching = batching


def relation_entries(eval_) -> RelationEvaluator:
    """`evaluate` run on a RelationEvaluator.  Raises ValueError when it adds no relation entry."""
    ev = RelationEvaluator()
    eval_.evaluate(ev)
    ev.check_finished()
    if not ev.entries:
        raise ValueError("evaluate adds no relation entries: there is no interaction trace to derive")
    return ev


class Program:
    """words: 2 per instruction (include/tstwo_hip.h); n_instr, n_regs (registers used), n_constraints (the ACCs of a constraint
    program, the STOREs of a columns program: n_out), n_loads."""

    def __init__(self, words, n_regs, n_constraints, n_loads):
        self.words, self.n_regs, self.n_constraints, self.n_loads = list(words), n_regs, n_constraints, n_loads

    @property
    def n_instr(self) -> int:
        return len(self.words) // 2

    @property
    def n_out(self) -> int:
        return self.n_constraints


def encode(op: int, dst: int = 0, x: int = 0, w1: int = 0) -> tuple:
    return (op | (dst << 8) | (x << 16), w1 & 0xffffffff)


class Canonical:
    """Structural merging of Expr nodes: canonical(e) is the one node that stands for every expression built like e (the same
    operation on the same merged operands; loads by column and offset; constants by value), so `is` on canonical nodes is
    structural equality."""

    def __init__(self):
        self.canon = {}             # structural key -> canonical node

    def __call__(self, e: Expr) -> Expr:
        canon = self.canon
        # iterative post-order: expressions can be deep chains
        stack, done = [(e, False)], {}
        while stack:
            n, expanded = stack.pop()
            if id(n) in done:
                continue
            if n.op in ("load", "const"):
                done[id(n)] = canon.setdefault(n.key, n)
                continue
            if not expanded:
                stack.append((n, True))
                stack.extend((a, False) for a in n.args if id(a) not in done)
                continue
            args = tuple(done[id(a)] for a in n.args)
            key = (n.op,) + tuple(id(a) for a in args)
            if key not in canon:
                canon[key] = Expr(n.op, args, key, n.degree)
            done[id(n)] = canon[key]
        return done[id(e)]


def compile_program(constraints: list, n_main: int, n_pre: int = 0) -> Program:
    """The program of tstwo_air_eval_program: constraint k is the k-th ACC (see _compile)."""
    program = _compile(constraints, n_main, n_pre, lambda k, r: encode(OP_ACC, 0, r))
    if program.n_constraints > MAX_CONSTRAINTS:
        raise ValueError(f"more than {MAX_CONSTRAINTS} constraints in one component")
    return program


def compile_columns(exprs: list, n_main: int, n_pre: int = 0) -> Program:
    """The program of tstwo_air_eval_columns: expression k is stored to output column k (STORE k in place of the k-th ACC)."""
    if not 1 <= len(exprs) <= MAX_OUT:
        raise ValueError(f"a columns program has 1 to {MAX_OUT} outputs")
    return _compile([Expr._lift(e) for e in exprs], n_main, n_pre, lambda k, r: encode(OP_STORE, 0, r, k))


def _compile(constraints: list, n_main: int, n_pre: int, terminal) -> Program:
    """Straight-line program of the DAG of `constraints` (the roots) over the columns main (n_main), preprocessed (n_pre),
    interaction, in that order; terminal(k, register) encodes the instruction that consumes root k (ACC or STORE).
    Nodes are merged structurally (same operation on the same merged operands;
    loads by column and offset; constants by value).  Instructions are ordered by a depth-first walk of each constraint in turn
    (the operand that needs more registers first), each value gets the lowest free register at its definition and frees it
    after its last use (an instruction may write the register its last operand read).  Raises ValueError when the program
    needs more than MAX_REGS registers or MAX_INSTR instructions."""
    canonical = Canonical()
    roots = [canonical(c) for c in constraints]
    # registers a subtree needs (Sethi-Ullman, on the tree view of the DAG): evaluate the heavier operand first
    need = {}

    def need_of(n):
        stack = [n]
        while stack:
            m = stack[-1]
            if id(m) in need:
                stack.pop()
                continue
            if m.op in ("load", "const"):
                need[id(m)] = 1
                stack.pop()
                continue
            pending = [a for a in m.args if id(a) not in need]
            if pending:
                stack.extend(pending)
                continue
            ns = sorted((need[id(a)] for a in m.args), reverse=True)
            need[id(m)] = ns[0] if len(ns) == 1 or ns[0] != ns[1] else ns[0] + 1
            stack.pop()
        return need[id(n)]

    order, seen = [], set()             # instructions: ("node", n) or ("acc", n)
    for r in roots:
        need_of(r)
        stack = [(r, False)]
        while stack:
            n, expanded = stack.pop()
            if id(n) in seen:
                continue
            if n.op in ("load", "const") or expanded:
                seen.add(id(n))
                order.append(("node", n))
                continue
            stack.append((n, True))
            args = sorted(n.args, key=lambda a: -need[id(a)])      # stable: ties keep operand order
            stack.extend((a, False) for a in reversed(args) if id(a) not in seen)
        order.append(("acc", r))
    # the instructions that read every value
    uses = {}
    for i, (kind, n) in enumerate(order):
        for a in ((n,) if kind == "acc" else () if n.op in ("load", "const") else n.args):
            uses.setdefault(id(a), []).append(i)
    if len(order) > MAX_INSTR:
        raise ValueError(f"the constraints compile to {len(order)} instructions, more than {MAX_INSTR}")
    reg, held, free, n_regs, words, n_loads, n_done = {}, {}, [], 0, [], 0, 0   # reg: value -> register, held: register -> value

    def next_use(a, i):
        u = uses[id(a)]
        k = bisect.bisect_left(u, i)
        return u[k] if k < len(u) else len(order)

    def take(i, protect):
        """The lowest free register; when all MAX_REGS hold live values, evict the load or constant (cheap to redo) whose next
        use is farthest away."""
        nonlocal n_regs
        if free:
            free.sort()
            return free.pop(0)
        if n_regs < MAX_REGS:
            n_regs += 1
            return n_regs - 1
        victims = [v for v in held.values() if v.op in ("load", "const") and id(v) not in protect]
        if not victims:
            raise ValueError(f"the constraints need more than {MAX_REGS} live registers")
        v = max(victims, key=lambda v: (next_use(v, i), -reg[id(v)]))
        r = reg.pop(id(v))
        del held[r]
        return r

    def emit_leaf(n, i, protect):
        nonlocal n_loads
        d = take(i, protect)
        if n.op == "load":
            (col, offset) = n.args
            x = col[1] if col[0] == "main" else n_main + col[1] if col[0] == "pre" else n_main + n_pre + col[1]
            if x >= MAX_COLS:
                raise ValueError(f"more than {MAX_COLS} columns")
            words.extend(encode(OP_LOAD, d, x, offset))
            n_loads += 1
        else:
            words.extend(encode(OP_CONST, d, 0, n.args))
        reg[id(n)], held[d] = d, n

    def release(ns, i):
        for a in ns:
            if id(a) in reg and next_use(a, i + 1) == len(order):
                r = reg.pop(id(a))
                del held[r]
                free.append(r)

    for i, (kind, n) in enumerate(order):
        operands = (n,) if kind == "acc" else () if n.op in ("load", "const") else n.args
        protect = {id(a) for a in operands}
        for a in operands:                        # reload what was evicted
            if id(a) not in reg:
                emit_leaf(a, i, protect)
        if kind == "acc":
            words.extend(terminal(n_done, reg[id(n)]))
            n_done += 1
            release([n], i)
            continue
        if n.op in ("load", "const"):
            emit_leaf(n, i, protect)
            continue
        srcs = [reg[id(a)] for a in n.args]
        release(n.args, i)
        d = take(i, protect)
        op = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL, "sqr": OP_SQR, "neg": OP_NEG}[n.op]
        words.extend(encode(op, d, srcs[0], srcs[1] if len(srcs) == 2 else 0))
        reg[id(n)], held[d] = d, n
    if len(words) // 2 > MAX_INSTR:
        raise ValueError(f"the constraints compile to {len(words) // 2} instructions, more than {MAX_INSTR}")
    return Program(words, n_regs, len(roots), n_loads)


class PointEvaluator(EvalAtRow):
    """Evaluates the constraints over QM31 (Rust PointEvaluator): main[k] = the values of main column k at its offsets, pre[i] =
    the value of the component's i-th preprocessed column."""

    def __init__(self, main: list, pre: list, inter: list = (), claimed_sum: QM31 | None = None, log_size: int = 0):
        super().__init__(claimed_sum, log_size)
        self.main, self.pre, self.inter = main, pre, list(inter)

    def _secure(self, o):
        return PointValue(PointValue._q(o))

    def _extension_values(self, k: int, offsets) -> list:
        # at the OODS point every base column's sample is a QM31: combine the 4 with from_partial_evals (no packing)
        if k + 4 > len(self.inter):
            raise ValueError("more interaction columns than sampled")
        if any(len(self.inter[k + c]) != len(offsets) for c in range(4)):
            raise ValueError("one sampled value per mask offset expected")
        return [PointValue(QM31.from_partial_evals([self.inter[k + c][j] for c in range(4)])) for j in range(len(offsets))]

    def next_interaction_mask(self, interaction: int, offsets) -> list:
        offsets = list(offsets)
        if interaction == ORIGINAL_TRACE_IDX:
            if self.n_main >= len(self.main):
                raise ValueError("more mask columns than sampled")
            if len(self.main[self.n_main]) != len(offsets):
                raise ValueError("one sampled value per mask offset expected")
        self._j = 0
        return super().next_interaction_mask(interaction, offsets)

    def _value(self, column, offset):
        kind, idx = column
        if kind == "pre":
            if idx >= len(self.pre):
                raise ValueError("preprocessed column out of range")
            return PointValue(self.pre[idx])
        v = self.main[idx][self._j]
        self._j += 1
        return PointValue(v)


def point_constraints(eval_, main: list, pre: list, inter: list = (), claimed_sum: QM31 | None = None, log_size: int = 0) -> list:
    """The constraints of eval_ at a point as QM31 values (no denominator): main[k] the sampled values of main column k (one per
    offset), pre[i] the component's i-th preprocessed column, inter[k] the sampled values of interaction column k; claimed_sum
    and log_size give the LogUp shift."""
    ev = PointEvaluator(main, pre, inter, claimed_sum, log_size)
    eval_.evaluate(ev)
    ev.check_finished()
    return [PointValue._q(c) for c in ev.constraints]


# ------------------------------------------------------------------ the device entry points
def evaluate_program(cols, trace_log_size: int, log_expand: int, program: Program, coeffs, denom_inv, accum: SecureColumnByCoords) -> None:
    """tstwo_air_eval_program: accum[r] += sum_k coeffs[k] e_k(r) * denom_inv[r >> trace_log_size] over the columns `cols`
    (HipColumns on the evaluation domain of log size trace_log_size + log_expand, bit-reversed)."""
    words = L.u32x(program.words)
    cw = (C.c_uint32 * max(4 * len(coeffs), 4))(*[w for c in coeffs for w in c.tup()])
    dinv = L.u32x([d.value if isinstance(d, M31) else int(d) for d in denom_inv])
    L.call("tstwo_air_eval_program", L.ptr_array([c.ptr for c in cols]), len(cols), trace_log_size, log_expand, words,
           program.n_instr, cw, len(coeffs), dinv, accum.ptrs())


class NativeKernel:
    """A program compiled to a native kernel (tstwo_air_program_compile, or tstwo_air_columns_compile for a columns program):
    `id` names it in the library's table, n_cols and n_constraints (the outputs of a columns program: n_out) are what it was
    compiled for, compile_seconds the wall time of the compilation."""

    def __init__(self, id_: int, n_cols: int, n_constraints: int, compile_seconds: float):
        self.id, self.n_cols, self.n_constraints, self.compile_seconds = id_, n_cols, n_constraints, compile_seconds

    @property
    def n_out(self) -> int:
        return self.n_constraints

    def info(self) -> dict:
        """tstwo_air_kernel_info: VGPRs, SGPRs and private-segment bytes of both widths, the code-object size, the compile time."""
        w = (C.c_uint32 * 7)()
        L.call("tstwo_air_kernel_info", self.id, w)
        width = lambda k: {"vgprs": w[3 * k], "sgprs": w[3 * k + 1], "private_bytes": w[3 * k + 2]}
        return {"w4": width(0), "w1": width(1), "code_bytes": w[6], "compile_seconds": self.compile_seconds}


_native_kernels: dict = {}              # (program words, n_cols) -> NativeKernel: one compilation per program and process


def compile_native(program: Program, n_cols: int) -> NativeKernel:
    """The native kernel of a constraint program over n_cols columns, compiled once per process: programs with the same words
    (the same eval at any size) share it.  A cached kernel the library no longer knows (tstwo_shutdown unloads every kernel,
    and so does tstwo_init on another device) is compiled again."""
    return _compile_native("tstwo_air_program_compile", program, n_cols)


def compile_columns_native(program: Program, n_cols: int) -> NativeKernel:
    """The native kernel of a compile_columns program over n_cols input columns (tstwo_air_columns_compile), cached and
    recompiled as compile_native's: the words of a columns program (its STOREs) never equal those of a constraint program."""
    return _compile_native("tstwo_air_columns_compile", program, n_cols)


def _compile_native(entry: str, program: Program, n_cols: int) -> NativeKernel:
    key = (tuple(program.words), n_cols)
    kernel = _native_kernels.get(key)
    if kernel is not None:
        try:
            kernel.info()
            return kernel
        except L.TstwoError:
            del _native_kernels[key]
    L.ensure_init()
    kid = C.c_uint64(0)
    t0 = time.perf_counter()
    L.call(entry, L.u32x(program.words), program.n_instr, n_cols, program.n_constraints, C.byref(kid))
    kernel = _native_kernels[key] = NativeKernel(kid.value, n_cols, program.n_constraints, time.perf_counter() - t0)
    return kernel


def evaluate_program_native(cols, trace_log_size: int, log_expand: int, kernel: NativeKernel, coeffs, denom_inv,
                            accum: SecureColumnByCoords) -> None:
    """tstwo_air_eval_compiled: what evaluate_program computes, bit for bit, by the kernel compile_native made of the program."""
    cw = (C.c_uint32 * max(4 * len(coeffs), 4))(*[w for c in coeffs for w in c.tup()])
    dinv = L.u32x([d.value if isinstance(d, M31) else int(d) for d in denom_inv])
    L.call("tstwo_air_eval_compiled", kernel.id, L.ptr_array([c.ptr for c in cols]), len(cols), trace_log_size, log_expand,
           cw, len(coeffs), dinv, accum.ptrs())


def evaluate_columns(cols, log_size: int, program: Program, n_out: int, *, native: bool = False) -> list:
    """tstwo_air_eval_columns: the n_out output columns (new HipColumns of 2^log_size values) of a compile_columns program over
    `cols`, HipColumns on CanonicCoset(log_size).circle_domain() in storage order (main, then preprocessed).  Asynchronous.
    native=True (opt-in): the program is compiled once per process (compile_columns_native) and
    tstwo_air_eval_columns_compiled runs that kernel instead of the interpreter, with identical results."""
    from .backend import HipColumn
    if n_out != program.n_out:
        raise ValueError(f"the program stores {program.n_out} outputs, {n_out} were asked for")
    n = 1 << log_size
    if any(c.len() != n for c in cols):
        raise ValueError("every column must hold 2^log_size values")
    out = [HipColumn.uninitialized(n) for _ in range(n_out)]
    if native:
        kernel = compile_columns_native(program, len(cols))
        L.call("tstwo_air_eval_columns_compiled", kernel.id, L.ptr_array([c.ptr for c in cols]), len(cols), log_size,
               L.ptr_array([c.ptr for c in out]), n_out)
        return out
    L.call("tstwo_air_eval_columns", L.ptr_array([c.ptr for c in cols]), len(cols), log_size, L.u32x(program.words), program.n_instr,
           L.ptr_array([c.ptr for c in out]), n_out)
    return out


NO_ROW = 0xffffffff                     # tstwo_air_check_constraints: "the constraint fails on no row"


def check_program(cols, log_size: int, program: Program, groups=None) -> list:
    """tstwo_air_check_constraints: [(n_rows, first_row | None)] per constraint of a compile_program program over `cols`,
    HipColumns on CanonicCoset(log_size).circle_domain() in storage order (main, then preprocessed, then interaction): the
    number of rows on which the constraint is non-zero and the first of them in coset order (the row of the trace as it was
    written).  groups[k] is the constraint the k-th ACC belongs to (the identity by default; a secure constraint is 4 ACCs with
    one index).  One launch, one read-back of 2 words per constraint."""
    from .backend import HipColumn
    n = 1 << log_size
    if any(c.len() != n for c in cols):
        raise ValueError("every column must hold 2^log_size values")
    words = list(program.words)
    accs = [pc for pc in range(program.n_instr) if words[2 * pc] & 0xff == OP_ACC]
    groups = list(range(len(accs))) if groups is None else [int(g) for g in groups]
    if len(groups) != len(accs):
        raise ValueError(f"groups names {len(groups)} ACCs, the program has {len(accs)}")
    if not groups:
        raise ValueError("the program has no constraints")
    for pc, g in zip(accs, groups):
        words[2 * pc + 1] = g & 0xffffffff
    n_constraints = groups[-1] + 1
    report = HipColumn.uninitialized(2 * n_constraints)
    L.call("tstwo_air_check_constraints", L.ptr_array([c.ptr for c in cols]), len(cols), log_size, L.u32x(words), program.n_instr,
           n_constraints, L.vp(report.ptr))
    r = report.to_numpy()
    return [(int(r[2 * c]), None if int(r[2 * c + 1]) == NO_ROW else int(r[2 * c + 1])) for c in range(n_constraints)]


# one failing constraint of a component: its index (add_constraint calls in the order `evaluate` makes them), the number of rows
# on which it is non-zero and the first of them in coset order
ConstraintFailure = namedtuple("ConstraintFailure", "constraint n_rows first_row")


def _trace_column(x):
    """A HipColumn of a column given as one, as an evaluation (`.values`) or as an array."""
    return _col(getattr(x, "values", x))


# ------------------------------------------------------------------ FrameworkComponent (Rust constraint_framework/component.rs)
class FrameworkComponent:
    """A component defined by a FrameworkEval (`log_size()`, `max_constraint_log_degree_bound()`, `evaluate(eval)`).  Its main
    columns are allocated in the main trace tree by `location_allocator`; `preprocessed_column_indices[i]` is the position in the
    preprocessed tree (tree 0) of the column `get_preprocessed_column(i)` reads.  `kind` is the TSTWO_AIR_* kind of the
    hand-written kernel for the eval's exact type (None: the program path, and `program` holds the compiled constraints).
    claimed_sum: the LogUp sum of the component's interaction trace (LogupTraceGenerator.finalize_last), required exactly when
    `evaluate` adds relation entries; its interaction columns are then allocated in tree INTERACTION_TRACE_IDX, 4 per batch.
    native=True (opt-in, and only on the program path): the program is compiled to a native kernel here, at construction, and
    evaluate_constraint_quotients_on_domain runs that kernel instead of the interpreter, with identical results."""

    def __init__(self, eval_, location_allocator: TraceLocationAllocator | None = None, preprocessed_column_indices=None, *,
                 claimed_sum: QM31 | None = None, native: bool = False):
        self.eval = eval_
        self.log_size = eval_.log_size()
        if self.log_size < 1:
            raise ValueError("log_size must be at least 1")
        inf = info(eval_)
        need = required_log_degree_bound(self.log_size, inf.max_degree())
        bound = eval_.max_constraint_log_degree_bound()
        if bound < need:
            raise ValueError(f"max_constraint_log_degree_bound {bound} is below {need}, which constraints of degree "
                             f"{inf.max_degree()} over 2^{self.log_size} rows need")
        if bound - self.log_size > MAX_LOG_EXPAND:
            raise ValueError(f"max_constraint_log_degree_bound exceeds log_size + {MAX_LOG_EXPAND}")
        self.info = inf
        self.mask_offsets = [list(o) for o in inf.main_offsets]
        self.n_columns = len(self.mask_offsets)
        self.n_constraints = inf.n_constraints
        self.preprocessed_column_indices = list(preprocessed_column_indices or [])
        if inf.n_preprocessed() > len(self.preprocessed_column_indices):
            raise ValueError(f"evaluate reads {inf.n_preprocessed()} preprocessed columns, {len(self.preprocessed_column_indices)} named")
        if inf.n_entries and claimed_sum is None:
            raise ValueError("evaluate adds relation entries: FrameworkComponent needs claimed_sum")
        if not inf.n_entries and claimed_sum is not None:
            raise ValueError("claimed_sum given, but evaluate adds no relation entries")
        self.claimed_sum = claimed_sum
        self.interaction_offsets = [list(o) for o in inf.interaction_offsets]
        self.n_interaction_columns = len(self.interaction_offsets)
        self.secure_flags = inf.secure_flags()
        alloc = location_allocator or TraceLocationAllocator()
        structure = {ORIGINAL_TRACE_IDX: self.n_columns}
        if self.n_interaction_columns:
            structure[INTERACTION_TRACE_IDX] = self.n_interaction_columns
        self.trace_locations = alloc.next_for_structure(structure)
        self.kind = _HAND_WRITTEN_KINDS.get(type(eval_))
        self.program = None
        self._check_program = None       # hand-written kinds: compiled by constraint_failures at its first use
        if self.kind is None:
            pe = ProgramEvaluator(claimed_sum, self.log_size)
            eval_.evaluate(pe)
            pe.check_finished()
            self.program = pe.compile(self.n_columns, len(self.preprocessed_column_indices))
        self.native = None
        if native and self.program is not None and self.n_constraints:
            self.native = compile_native(self.program, self._n_program_columns())

    def _n_program_columns(self) -> int:
        return self.n_columns + len(self.preprocessed_column_indices) + self.n_interaction_columns

    def native_info(self) -> dict | None:
        """NativeKernel.info() of the component's kernel; None for a component that does not run one."""
        return self.native.info() if self.native is not None else None

    def derive_interaction_trace(self, main, preprocessed=()):
        """logup.derive_interaction_trace of the component's eval, through native column kernels when the component runs a
        native constraint kernel (native=True)."""
        from .logup import derive_interaction_trace
        return derive_interaction_trace(self.eval, main, preprocessed, native=self.native is not None)

    # --- which constraint fails on which row (Rust assert_constraints_on_trace)
    def _constraint_program(self) -> Program:
        """The compiled constraints: `program`, or for the hand-written kinds (which prove on their own kernel) the program the
        other evals take, compiled at the first use."""
        if self.program is not None:
            return self.program
        if self._check_program is None:
            pe = ProgramEvaluator(self.claimed_sum, self.log_size)
            self.eval.evaluate(pe)
            pe.check_finished()
            self._check_program = pe.compile(self.n_columns, len(self.preprocessed_column_indices))
        return self._check_program

    def constraint_failures(self, main, preprocessed=(), interaction=()) -> list:
        """The constraints the trace breaks, as ConstraintFailure(constraint, n_rows, first_row) in constraint order; [] for a
        trace that satisfies the AIR.  main / preprocessed / interaction: the component's own columns (HipColumns, evaluations or
        arrays) on CanonicCoset(log_size).circle_domain() in storage order; preprocessed[i] is the column
        get_preprocessed_column(i) reads.  A secure (LogUp) constraint is reported once.  One launch (check_program)."""
        cols = [_trace_column(c) for c in list(main) + list(preprocessed) + list(interaction)]
        want = (self.n_columns, len(self.preprocessed_column_indices), self.n_interaction_columns)
        if (len(main), len(preprocessed), len(interaction)) != want:
            raise ValueError(f"the component reads {want[0]} main, {want[1]} preprocessed and {want[2]} interaction columns, "
                             f"not {len(main)}, {len(preprocessed)} and {len(interaction)}")
        if self.n_constraints == 0:
            return []
        groups = [c for c, secure in enumerate(self.secure_flags) for _ in range(4 if secure else 1)]
        report = check_program(cols, self.log_size, self._constraint_program(), groups)
        return [ConstraintFailure(c, n, first) for c, (n, first) in enumerate(report) if n]

    def assert_constraints(self, main, preprocessed=(), interaction=()) -> None:
        """Raises prover.ConstraintViolation (a ConstraintsNotSatisfied) naming the first failing constraint and its first row."""
        failures = self.constraint_failures(main, preprocessed, interaction)
        if failures:
            from .prover import ConstraintViolation
            raise ConstraintViolation(None, failures, 1 << self.log_size)

    # --- Component
    def max_constraint_log_degree_bound(self) -> int:
        return self.eval.max_constraint_log_degree_bound()

    def trace_log_degree_bounds(self) -> list:
        trees = [[self.log_size] * len(self.preprocessed_column_indices), [self.log_size] * self.n_columns]
        if self.n_interaction_columns:
            trees.append([self.log_size] * self.n_interaction_columns)
        return trees

    def mask_points(self, point: CirclePoint) -> list:
        """Preprocessed columns at [point]; main column k at point + step * offset for each of its offsets, in order; the same
        for the interaction columns (tree INTERACTION_TRACE_IDX) when the eval uses LogUp."""
        trees = [[[point] for _ in self.preprocessed_column_indices],
                 [[shifted_mask_point(point, self.log_size, o) for o in offs] for offs in self.mask_offsets]]
        if self.n_interaction_columns:
            trees.append([[shifted_mask_point(point, self.log_size, o) for o in offs] for offs in self.interaction_offsets])
        return trees

    def _columns(self, tree: int = ORIGINAL_TRACE_IDX) -> range:
        start, end = self.trace_locations[tree]
        return range(start, end)

    def evaluate_constraint_quotients_at_point(self, point: CirclePoint, mask: list, acc: PointEvaluationAccumulator) -> None:
        denom_inv = coset_vanishing(CanonicCoset(self.log_size).coset, point).inverse()
        main = [list(mask[ORIGINAL_TRACE_IDX][ci]) for ci in self._columns()]
        for vals, offs in zip(main, self.mask_offsets):
            if len(vals) != len(offs):
                raise ValueError("one sampled value per mask offset expected")
        pre = []
        for idx in self.preprocessed_column_indices:
            col = mask[PREPROCESSED_TRACE_IDX][idx]
            if len(col) != 1:
                raise ValueError("one sampled value per preprocessed column expected")
            pre.append(col[0])
        inter = []
        if self.n_interaction_columns:
            inter = [list(mask[INTERACTION_TRACE_IDX][ci]) for ci in self._columns(INTERACTION_TRACE_IDX)]
            for vals, offs in zip(inter, self.interaction_offsets):
                if len(vals) != len(offs):
                    raise ValueError("one sampled value per mask offset expected")
        for c in point_constraints(self.eval, main, pre, inter, self.claimed_sum, self.log_size):
            acc.accumulate(c.mul(denom_inv))

    # --- ComponentProver
    def _on_eval_domain(self, trace, tree: int, indices, twiddles) -> list:
        eval_domain = CanonicCoset(self.max_constraint_log_degree_bound()).circleDomain()
        cols, missing = [], []
        for ci in indices:
            ev = trace.evals[tree][ci]
            cols.append(ev.values if ev.domain == eval_domain else None)
            if cols[-1] is None:
                missing.append((len(cols) - 1, trace.polys[tree][ci]))
        if missing:
            for (k, _), ev in zip(missing, evaluate_polynomials([p for _, p in missing], eval_domain, twiddles)):
                cols[k] = ev.values
        return cols

    def trace_on_eval_domain(self, trace, twiddles) -> list:
        """The columns the kernels read, on CanonicCoset(max_constraint_log_degree_bound).circle_domain(): the main columns, then
        the preprocessed ones, then the interaction ones (LogUp); each the committed evaluation when it already lives there (log
        blowup 1), else its polynomial evaluated there (one batched launch sequence per tree)."""
        cols = (self._on_eval_domain(trace, ORIGINAL_TRACE_IDX, self._columns(), twiddles)
                + self._on_eval_domain(trace, PREPROCESSED_TRACE_IDX, self.preprocessed_column_indices, twiddles))
        if self.n_interaction_columns:
            cols += self._on_eval_domain(trace, INTERACTION_TRACE_IDX, self._columns(INTERACTION_TRACE_IDX), twiddles)
        return cols

    def evaluate_constraint_quotients_on_domain(self, trace, acc: DomainEvaluationAccumulator, twiddles) -> None:
        eval_log = self.max_constraint_log_degree_bound()
        cols = self.trace_on_eval_domain(trace, twiddles)
        [column_acc] = acc.columns([(eval_log, self.n_constraints)])
        if self.n_constraints == 0:
            return
        coeffs, denom_inv = column_acc.random_coeff_powers, denominator_inverses(self.log_size, eval_log)
        if self.kind is not None:
            evaluate_constraint_quotients(self.kind, cols, self.log_size, eval_log - self.log_size, coeffs, denom_inv, column_acc.col)
        else:
            if any(self.secure_flags):
                coeffs = expand_coeffs(coeffs, self.secure_flags)
            if self.native is None:
                evaluate_program(cols, self.log_size, eval_log - self.log_size, self.program, coeffs, denom_inv, column_acc.col)
                return
            try:
                evaluate_program_native(cols, self.log_size, eval_log - self.log_size, self.native, coeffs, denom_inv, column_acc.col)
            except L.TstwoError as e:
                if "unknown air kernel" not in str(e):
                    raise
                # the library was shut down since construction: compile_native notices and compiles again
                self.native = compile_native(self.program, len(cols))
                evaluate_program_native(cols, self.log_size, eval_log - self.log_size, self.native, coeffs, denom_inv, column_acc.col)


# ------------------------------------------------------------------ evals: wide Fibonacci, mul-add, Fibonacci over rows
class WideFibonacciEval:
    """WideFibonacciEval<N> (examples/fibonacci.ts): N columns, N - 2 constraints x_{i+2} = x_i^2 + x_{i+1}^2 on each row."""

    def __init__(self, log_n_rows: int, n_columns: int = 100):
        if n_columns < 3:
            raise ValueError("wide Fibonacci needs at least 3 columns")
        self.log_n_rows, self.n_columns = log_n_rows, n_columns

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 1

    def evaluate(self, eval):
        a, b = eval.next_trace_mask(), eval.next_trace_mask()
        for _ in range(2, self.n_columns):
            c = eval.next_trace_mask()
            eval.add_constraint(c - (a.square() + b.square()))
            a, b = b, c
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


class MulAddEval:
    """TestEval of the Rust tutorial's example 05: 3 columns, x_0 x_1 + x_0 - x_2 = 0 on each row."""

    def __init__(self, log_n_rows: int):
        self.log_n_rows = log_n_rows

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 1

    def evaluate(self, eval):
        x0, x1, x2 = eval.next_trace_mask(), eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_constraint(x0 * x1 + x0 - x2)
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


# the evals whose exact type runs on the hand-written kernel (2.8x faster than the interpreter on wide Fibonacci)
_HAND_WRITTEN_KINDS = {WideFibonacciEval: AIR_WIDE_FIB, MulAddEval: AIR_MUL_ADD}


def WideFibonacciComponent(log_n_rows: int, n_columns: int = 100,
                           location_allocator: TraceLocationAllocator | None = None) -> FrameworkComponent:
    """Rust's `type WideFibonacciComponent = FrameworkComponent<WideFibonacciEval<N>>`."""
    return FrameworkComponent(WideFibonacciEval(log_n_rows, n_columns), location_allocator)


def MulAddComponent(log_n_rows: int, location_allocator: TraceLocationAllocator | None = None) -> FrameworkComponent:
    """FrameworkComponent<MulAddEval>."""
    return FrameworkComponent(MulAddEval(log_n_rows), location_allocator)


def coset_index_to_circle_domain_index(coset_index: int, log_domain_size: int) -> int:
    """utils.rs: the circle-domain index of the point at `coset_index` of CanonicCoset(log_domain_size)."""
    if coset_index % 2 == 0:
        return coset_index // 2
    return ((2 << log_domain_size) - coset_index) // 2


def coset_order_positions(log_size: int) -> list:
    """Storage position (bit-reversed circle-domain order) of trace row k of the coset order, k < 2^log_size."""
    return [bit_reverse_index(coset_index_to_circle_domain_index(k, log_size), log_size) for k in range(1 << log_size)]


class FibonacciRowsEval:
    """Two main columns (a, b); row k + 1 follows row k: a' = b, b' = a^2 + b^2, from the public (a0, b0) at the first row, which
    the preprocessed column is_first marks.  Constraints (prev = offset -1):
        (1 - is_first) (a - prev_b)                    degree 2
        (1 - is_first) (b - prev_a^2 - prev_b^2)       degree 3
        is_first (a - a0),   is_first (b - b0)
    Degree 3 needs max_constraint_log_degree_bound = log_size + 2."""

    def __init__(self, log_n_rows: int, a0: int = 1, b0: int = 1):
        self.log_n_rows, self.a0, self.b0 = log_n_rows, int(a0) % P, int(b0) % P

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 2

    def evaluate(self, eval):
        is_first = eval.get_preprocessed_column(0)
        prev_a, a = eval.next_interaction_mask(ORIGINAL_TRACE_IDX, [-1, 0])
        prev_b, b = eval.next_interaction_mask(ORIGINAL_TRACE_IDX, [-1, 0])
        not_first = 1 - is_first
        eval.add_constraint(not_first * (a - prev_b))
        eval.add_constraint(not_first * (b - prev_a.square() - prev_b.square()))
        eval.add_constraint(is_first * (a - self.a0))
        eval.add_constraint(is_first * (b - self.b0))
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


def fibonacci_rows_trace(log_n_rows: int, a0: int = 1, b0: int = 1):
    """(a, b) as numpy uint32 columns in storage order (bit-reversed circle domain): row k of the coset order at
    bit_reverse(coset_index_to_circle_domain_index(k))."""
    import numpy as np
    n = 1 << log_n_rows
    a_seq, b_seq = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    a, b = int(a0) % P, int(b0) % P
    for k in range(n):
        a_seq[k], b_seq[k] = a, b
        a, b = b, (a * a + b * b) % P
    pos = np.asarray(coset_order_positions(log_n_rows))
    ca, cb = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    ca[pos], cb[pos] = a_seq, b_seq
    return ca, cb


def is_first_column(log_size: int):
    """The preprocessed selector: 1 at the first row of the coset order (storage position 0), else 0."""
    import numpy as np
    c = np.zeros(1 << log_size, dtype=np.uint32)
    c[coset_order_positions(log_size)[0]] = 1
    return c


# ------------------------------------------------------------------ LogUp examples: a permutation, a range check
class PermutationEval:
    """Columns a and b with the entries (+1, [a]) and (-1, [b]) of one relation, in one batch (finalize_logup_in_pairs).  The claimed
    sum is 0 exactly when b permutes a (with high probability over the lookup elements).  Degree 3: log_size + 2."""

    def __init__(self, log_n_rows: int, lookup_elements: LookupElements):
        self.log_n_rows, self.lookup_elements = log_n_rows, lookup_elements

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 2

    def evaluate(self, eval):
        a, b = eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, 1, [a]))
        eval.add_to_relation(RelationEntry(self.lookup_elements, -1, [b]))
        eval.finalize_logup_in_pairs()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


class RangeCheckTableEval:
    """The table side of a range check over [0, 2^log_range): preprocessed column 0 holds value k at coset row k, the main column
    `multiplicity` says how often the values components use it; entry (-multiplicity, [value]), finalize_logup().  Degree 2."""

    def __init__(self, log_range: int, lookup_elements: LookupElements):
        self.log_range, self.lookup_elements = log_range, lookup_elements

    def log_size(self) -> int:
        return self.log_range

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_range + 1

    def evaluate(self, eval):
        value = eval.get_preprocessed_column(0)
        multiplicity = eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, -multiplicity, [value]))
        eval.finalize_logup()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


class RangeCheckValuesEval:
    """The values side: two checked columns per row, entries (1, [v0]) and (1, [v1]) in one batch (finalize_logup_in_pairs).
    Degree 3: log_size + 2."""

    def __init__(self, log_n_rows: int, lookup_elements: LookupElements):
        self.log_n_rows, self.lookup_elements = log_n_rows, lookup_elements

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 2

    def evaluate(self, eval):
        v0, v1 = eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, 1, [v0]))
        eval.add_to_relation(RelationEntry(self.lookup_elements, 1, [v1]))
        eval.finalize_logup_in_pairs()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


class StateMachineEval:
    """stwo's state-machine example: columns x, y; the row uses the state (x, y) and yields the state (x + 1, y): entries
    (+1, [x, y]) and (-1, [x + 1, y]) in one batch (finalize_logup_in_pairs).  Over the trace of state_machine_trace the sum
    telescopes to 1 / combine([x0, y0]) - 1 / combine([x0 + 2^log, y0]).  The value x + 1 is an expression of a column: the
    interaction trace comes from logup.derive_interaction_trace.  Degree 3: log_size + 2."""

    def __init__(self, log_n_rows: int, lookup_elements: LookupElements):
        self.log_n_rows, self.lookup_elements = log_n_rows, lookup_elements

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 2

    def evaluate(self, eval):
        x, y = eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, 1, [x, y]))
        eval.add_to_relation(RelationEntry(self.lookup_elements, -1, [x + 1, y]))
        eval.finalize_logup_in_pairs()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


def state_machine_trace(log_n_rows: int, x0: int, y0: int):
    """(x, y) as numpy uint32 columns in storage order: coset row k holds (x0 + k, y0)."""
    import numpy as np
    n = 1 << log_n_rows
    x, y = np.empty(n, dtype=np.uint32), np.full(n, int(y0) % P, dtype=np.uint32)
    x[_coset_positions(log_n_rows)] = ((int(x0) % P + np.arange(n, dtype=np.uint64)) % P).astype(np.uint32)
    return x, y


def _col(x):
    from .backend import HipColumn
    return x if isinstance(x, HipColumn) else HipColumn(x)


def permutation_interaction_trace(log_n_rows: int, a, b, lookup_elements: LookupElements):
    """The interaction trace of PermutationEval on the device: (4 HipCircleEvaluations, claimed sum).  a, b: HipColumns or arrays."""
    gen = LogupTraceGenerator(log_n_rows)
    col = gen.new_col()
    col.write_frac(1, lookup_elements.combine_columns([_col(a)]))
    col.write_frac(P - 1, lookup_elements.combine_columns([_col(b)]))
    col.finalize_col()
    return gen.finalize_last()


def _coset_positions(log_size: int):
    """coset_order_positions as a numpy array, from the closed form of csrc/logup.hip: with j = k >> 1 and rev the bit reversal
    over log_size - 1 bits, row k sits at 2 rev(j) (k even) or 2 (2^(log_size-1) - 1 - rev(j)) + 1 (k odd)."""
    import numpy as np
    k = np.arange(1 << log_size, dtype=np.int64)
    j, r = k >> 1, np.zeros(1 << log_size, dtype=np.int64)
    for _ in range(log_size - 1):
        r, j = (r << 1) | (j & 1), j >> 1
    return np.where(k % 2 == 0, 2 * r, 2 * ((1 << (log_size - 1)) - 1 - r) + 1)


def range_check_table_column(log_range: int):
    """The preprocessed column of RangeCheckTableEval: value k at coset row k (numpy uint32, storage order)."""
    import numpy as np
    c = np.empty(1 << log_range, dtype=np.uint32)
    c[_coset_positions(log_range)] = np.arange(1 << log_range, dtype=np.uint32)
    return c


def range_check_multiplicities(log_range: int, *value_columns):
    """The multiplicity column of RangeCheckTableEval (numpy uint32, storage order) for the values in `value_columns`, which
    must lie in [0, 2^log_range)."""
    import numpy as np
    counts = np.zeros(1 << log_range, dtype=np.int64)
    for v in value_columns:
        v = np.asarray(v, dtype=np.int64)
        if v.size and (v.min() < 0 or v.max() >= 1 << log_range):
            raise ValueError("a checked value lies outside the range")
        counts += np.bincount(v, minlength=1 << log_range)
    m = np.empty(1 << log_range, dtype=np.uint32)
    m[_coset_positions(log_range)] = (counts % P).astype(np.uint32)
    return m


def range_check_table_column_device(log_range: int):
    """range_check_table_column built on the device (logup.coset_iota): a HipColumn."""
    from .logup import coset_iota
    return coset_iota(log_range)


def range_check_multiplicities_device(log_range: int, *value_columns, check: bool = True):
    """range_check_multiplicities counted on the device (logup.lookup_multiplicities, coset order): a HipColumn.  value_columns:
    HipColumns, which stay where they are, or arrays.  check=False skips the one-word read-back that raises the ValueError."""
    from .logup import lookup_multiplicities
    return lookup_multiplicities(log_range, *value_columns, order="coset", check=check)


def range_check_table_interaction_trace(log_range: int, multiplicity, lookup_elements: LookupElements):
    """The interaction trace of RangeCheckTableEval: (4 HipCircleEvaluations, claimed sum); multiplicity: HipColumn or array."""
    import numpy as np
    m = multiplicity.to_numpy() if hasattr(multiplicity, "to_numpy") else np.asarray(multiplicity, dtype=np.uint32)
    neg = ((P - m.astype(np.uint64)) % P).astype(np.uint32)
    gen = LogupTraceGenerator(log_range)
    col = gen.new_col()
    col.write_frac(_col(neg), lookup_elements.combine_columns([_col(range_check_table_column(log_range))]))
    col.finalize_col()
    return gen.finalize_last()


def range_check_values_interaction_trace(log_n_rows: int, v0, v1, lookup_elements: LookupElements):
    """The interaction trace of RangeCheckValuesEval: (4 HipCircleEvaluations, claimed sum)."""
    gen = LogupTraceGenerator(log_n_rows)
    col = gen.new_col()
    col.write_frac(1, lookup_elements.combine_columns([_col(v0)]))
    col.write_frac(1, lookup_elements.combine_columns([_col(v1)]))
    col.finalize_col()
    return gen.finalize_last()


class XorTableEval:
    """The table side of a lookup with a tuple key: XOR of two log_bits-bit words.  Preprocessed columns 0..2 hold (a, b, a ^ b)
    of k = a + 2^log_bits b at coset row k (xor_table_columns), the main column `multiplicity` says how often the values
    components use the row; entry (-multiplicity, [a, b, c]), finalize_logup().  Degree 2."""

    def __init__(self, log_bits: int, lookup_elements: LookupElements):
        self.log_bits, self.lookup_elements = log_bits, lookup_elements

    def log_size(self) -> int:
        return 2 * self.log_bits

    def max_constraint_log_degree_bound(self) -> int:
        return 2 * self.log_bits + 1

    def evaluate(self, eval):
        a, b, c = (eval.get_preprocessed_column(i) for i in range(3))
        multiplicity = eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(self.lookup_elements, -multiplicity, [a, b, c]))
        eval.finalize_logup()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


class XorValuesEval:
    """The values side: main columns a, b, c, enabler.  A component whose row count is no power of two pads its trace and
    switches the padded rows off: enabler is 0 or 1 (constraint enabler (1 - enabler) = 0), the entry is (enabler, [a, b, c]),
    finalize_logup(), so a padded row may hold anything.  Degree 2."""

    def __init__(self, log_n_rows: int, lookup_elements: LookupElements):
        self.log_n_rows, self.lookup_elements = log_n_rows, lookup_elements

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 1

    def evaluate(self, eval):
        a, b, c, enabler = (eval.next_trace_mask() for _ in range(4))
        eval.add_constraint(enabler * (1 - enabler))
        eval.add_to_relation(RelationEntry(self.lookup_elements, enabler, [a, b, c]))
        eval.finalize_logup()
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


def xor_table_columns(log_bits: int):
    """The preprocessed columns of XorTableEval: (a, b, a ^ b) of k = a + 2^log_bits b at coset row k (numpy uint32, storage order)."""
    import numpy as np
    k = np.arange(1 << (2 * log_bits), dtype=np.uint32)
    a, b = k & ((1 << log_bits) - 1), k >> log_bits
    pos = _coset_positions(2 * log_bits)
    cols = []
    for v in (a, b, a ^ b):
        c = np.empty(k.size, dtype=np.uint32)
        c[pos] = v
        cols.append(c)
    return cols


def xor_multiplicities_device(log_bits: int, a, b, enabler, check: bool = True):
    """The multiplicity column of XorTableEval counted on the device (logup.lookup_multiplicities_keyed, coset order): row
    a + 2^log_bits b receives the sum of `enabler` over the rows that hold (a, b); each limb is checked against log_bits on the
    enabled rows only.  c is not part of the key: a wrong c is the proof's business.  HipColumns stay where they are."""
    from .logup import LookupGroup, lookup_multiplicities_keyed
    return lookup_multiplicities_keyed([LookupGroup([(a, log_bits), (b, log_bits)], weight=enabler)], order="coset", check=check)

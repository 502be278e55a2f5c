"""The constraint framework: every AIR component (Rust stwo constraint_framework/: FrameworkEval, EvalAtRow, InfoEvaluator,
PointEvaluator, FrameworkComponent; the reference carries the shapes in constraint_framework/index.ts).

A component is a FrameworkComponent of an eval, an object with `log_size()`, `max_constraint_log_degree_bound()` and one
`evaluate(eval)` function.  Three evaluators drive it:
  InfoEvaluator     the mask offsets of each column, the number of constraints and the degree of each;
  ProgramEvaluator  the constraints as a straight-line program for tstwo_air_eval_program (include/tstwo_hip.h): identical loads
                    (same column and offset) and identical sub-expressions are computed once, registers are reused after their
                    last use, and the number of live registers is bounded by MAX_REGS;
  PointEvaluator    the constraints over QM31 at the out-of-domain point (the verifier, and the prover's sanity check).
The prover evaluates a component's constraints on the whole evaluation domain with one launch: WideFibonacciEval and MulAddEval
(exactly these types, not subclasses) run on the hand-written kernel of tstwo_air_constraint_quotients, every other eval on the
program interpreter.  WideFibonacciComponent and MulAddComponent are FrameworkComponents of those two evals, as in Rust.

Only the main trace (ORIGINAL_TRACE_IDX) is read at row offsets; preprocessed columns are read at offset 0 (as in Rust), and values
inside constraints are base-field (M31) values: interaction trees and secure-field (LogUp) columns are not supported.
"""
from __future__ import annotations

import bisect
import ctypes as C

from . import _lib as L
from .air import (AIR_MUL_ADD, AIR_WIDE_FIB, ORIGINAL_TRACE_IDX, PREPROCESSED_TRACE_IDX, DomainEvaluationAccumulator,
                  PointEvaluationAccumulator, TraceLocationAllocator, coset_vanishing, denominator_inverses,
                  evaluate_constraint_quotients, _lift)
from .backend import SecureColumnByCoords
from .circle import CanonicCoset, CirclePoint, bit_reverse_index
from .fields import M31, QM31, P
from .poly import evaluate_polynomials

# include/tstwo_hip.h TSTWO_AIR_OP_* and TSTWO_AIR_PROGRAM_MAX_*
OP_LOAD, OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_NEG, OP_ACC = range(8)
MAX_INSTR, MAX_REGS, MAX_CONSTRAINTS, MAX_COLS, MAX_OFFSET = 1536, 32, 256, 4096, 64
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


# ------------------------------------------------------------------ EvalAtRow
class EvalAtRow:
    """The surface `evaluate` sees (Rust EvalAtRow).  Subclasses produce the values."""

    def __init__(self):
        self.n_main = 0                 # main-trace mask columns handed out so far
        self.main_offsets = []          # offsets of each main column, in call order
        self.constraints = []

    def _value(self, column, offset):
        raise NotImplementedError

    def next_interaction_mask(self, interaction: int, offsets) -> list:
        if interaction == PREPROCESSED_TRACE_IDX:
            raise ValueError("preprocessed columns are read with get_preprocessed_column (offset 0 only)")
        if interaction != ORIGINAL_TRACE_IDX:
            raise ValueError("only the main trace (ORIGINAL_TRACE_IDX) is supported")
        offsets = [int(o) for o in offsets]
        if not offsets:
            raise ValueError("a mask needs at least one offset")
        if any(abs(o) > MAX_OFFSET for o in offsets):
            raise ValueError(f"row offsets are limited to |offset| <= {MAX_OFFSET}")
        k = self.n_main
        self.n_main += 1
        self.main_offsets.append(offsets)
        return [self._value(("main", k), o) for o in offsets]

    def next_trace_mask(self):
        return self.next_interaction_mask(ORIGINAL_TRACE_IDX, [0])[0]

    def get_preprocessed_column(self, i: int):
        if i < 0:
            raise ValueError("negative preprocessed column index")
        return self._value(("pre", int(i)), 0)

    def add_constraint(self, expr) -> None:
        self.constraints.append(expr)

    # camelCase aliases (the reference's names)
    nextInteractionMask = next_interaction_mask
    nextTraceMask = next_trace_mask
    getPreprocessedColumn = get_preprocessed_column
    addConstraint = add_constraint


class _SymbolicEval(EvalAtRow):
    def __init__(self):
        super().__init__()
        self.pre_used = set()

    def _value(self, column, offset):
        if column[0] == "pre":
            self.pre_used.add(column[1])
        return Expr.load(column, offset)

    def add_constraint(self, expr) -> None:
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

    def mask_offsets(self) -> list:
        """TreeVec: per preprocessed column read, [0]; per main column, its offsets."""
        return [[[0] for _ in range(self.n_preprocessed())], [list(o) for o in self.main_offsets]]


def required_log_degree_bound(log_size: int, max_degree: int) -> int:
    """The smallest max_constraint_log_degree_bound that holds the quotient of a degree-d constraint: about
    (d - 1) 2^log_size + 1 coefficients, so log_size + floor(log2(d - 1)) + 1 (and at least log_size + 1)."""
    if max_degree <= 2:
        return log_size + 1
    return log_size + (max_degree - 1).bit_length() - 1 + 1


def info(eval_) -> InfoEvaluator:
    ev = InfoEvaluator()
    eval_.evaluate(ev)
    return ev


class ProgramEvaluator(_SymbolicEval):
    """Records the constraints, then compile() turns them into the program of tstwo_air_eval_program."""

    def compile(self, n_main: int | None = None) -> "Program":
        return compile_program(self.constraints, self.n_main if n_main is None else n_main)


class Program:
    """words: 2 per instruction (include/tstwo_hip.h); n_instr, n_regs (registers used), n_constraints, n_loads."""

    def __init__(self, words, n_regs, n_constraints, n_loads):
        self.words, self.n_regs, self.n_constraints, self.n_loads = list(words), n_regs, n_constraints, n_loads

    @property
    def n_instr(self) -> int:
        return len(self.words) // 2


def encode(op: int, dst: int = 0, x: int = 0, w1: int = 0) -> tuple:
    return (op | (dst << 8) | (x << 16), w1 & 0xffffffff)


def compile_program(constraints: list, n_main: int) -> Program:
    """Straight-line program of the constraint DAG.  Nodes are merged structurally (same operation on the same merged operands;
    loads by column and offset; constants by value).  Instructions are ordered by a depth-first walk of each constraint in turn
    (the operand that needs more registers first), each value gets the lowest free register at its definition and frees it
    after its last use (an instruction may write the register its last operand read).  Raises ValueError when the program
    needs more than MAX_REGS registers or MAX_INSTR instructions."""
    canon = {}                # structural key -> canonical node

    def canonical(e: Expr) -> Expr:
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
    reg, held, free, n_regs, words, n_loads = {}, {}, [], 0, [], 0      # reg: value -> register, held: register -> value

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
            x = col[1] if col[0] == "main" else n_main + col[1]
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
            words.extend(encode(OP_ACC, 0, reg[id(n)]))
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
    if len(roots) > MAX_CONSTRAINTS:
        raise ValueError(f"more than {MAX_CONSTRAINTS} constraints in one component")
    return Program(words, n_regs, len(roots), n_loads)


class PointEvaluator(EvalAtRow):
    """Evaluates the constraints over QM31 (Rust PointEvaluator): main[k] = the values of main column k at its offsets, pre[i] =
    the value of the component's i-th preprocessed column."""

    def __init__(self, main: list, pre: list):
        super().__init__()
        self.main, self.pre = main, pre

    def next_interaction_mask(self, interaction: int, offsets) -> list:
        offsets = list(offsets)
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


def point_constraints(eval_, main: list, pre: list) -> list:
    """The constraints of eval_ at a point as QM31 values (no denominator): main[k] the sampled values of main column k (one per
    offset), pre[i] the component's i-th preprocessed column."""
    ev = PointEvaluator(main, pre)
    eval_.evaluate(ev)
    return [PointValue._q(c) for c in ev.constraints]
# ------------------------------------------------------------------ the device entry point
def evaluate_program(cols, trace_log_size: int, log_expand: int, program: Program, coeffs, denom_inv, accum: SecureColumnByCoords) -> None:
    """tstwo_air_eval_program: accum[r] += sum_k coeffs[k] e_k(r) * denom_inv[r >> trace_log_size] over the columns `cols`
    (HipColumns on the evaluation domain of log size trace_log_size + log_expand, bit-reversed)."""
    words = L.u32x(program.words)
    cw = (C.c_uint32 * max(4 * len(coeffs), 4))(*[w for c in coeffs for w in c.tup()])
    dinv = L.u32x([d.value if isinstance(d, M31) else int(d) for d in denom_inv])
    L.call("tstwo_air_eval_program", L.ptr_array([c.ptr for c in cols]), len(cols), trace_log_size, log_expand, words,
           program.n_instr, cw, len(coeffs), dinv, accum.ptrs())


# ------------------------------------------------------------------ FrameworkComponent (Rust constraint_framework/component.rs)
class FrameworkComponent:
    """A component defined by a FrameworkEval (`log_size()`, `max_constraint_log_degree_bound()`, `evaluate(eval)`).  Its main
    columns are allocated in the main trace tree by `location_allocator`; `preprocessed_column_indices[i]` is the position in the
    preprocessed tree (tree 0) of the column `get_preprocessed_column(i)` reads.  `kind` is the TSTWO_AIR_* kind of the
    hand-written kernel for the eval's exact type (None: the program path, and `program` holds the compiled constraints)."""

    def __init__(self, eval_, location_allocator: TraceLocationAllocator | None = None, preprocessed_column_indices=None):
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
        alloc = location_allocator or TraceLocationAllocator()
        self.trace_locations = alloc.next_for_structure({ORIGINAL_TRACE_IDX: self.n_columns})
        self.kind = _HAND_WRITTEN_KINDS.get(type(eval_))
        self.program = None
        if self.kind is None:
            pe = ProgramEvaluator()
            eval_.evaluate(pe)
            self.program = pe.compile(self.n_columns)

    # --- Component
    def max_constraint_log_degree_bound(self) -> int:
        return self.eval.max_constraint_log_degree_bound()

    def trace_log_degree_bounds(self) -> list:
        return [[self.log_size] * len(self.preprocessed_column_indices), [self.log_size] * self.n_columns]

    def mask_points(self, point: CirclePoint) -> list:
        """Preprocessed columns at [point]; main column k at point + step * offset for each of its offsets, in order."""
        return [[[point] for _ in self.preprocessed_column_indices],
                [[shifted_mask_point(point, self.log_size, o) for o in offs] for offs in self.mask_offsets]]

    def _columns(self) -> range:
        start, end = self.trace_locations[ORIGINAL_TRACE_IDX]
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
        for c in point_constraints(self.eval, main, pre):
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
        the preprocessed ones; each the committed evaluation when it already lives there (log blowup 1), else its polynomial
        evaluated there (one batched launch sequence per tree)."""
        return (self._on_eval_domain(trace, ORIGINAL_TRACE_IDX, self._columns(), twiddles)
                + self._on_eval_domain(trace, PREPROCESSED_TRACE_IDX, self.preprocessed_column_indices, twiddles))

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
            evaluate_program(cols, self.log_size, eval_log - self.log_size, self.program, coeffs, denom_inv, column_acc.col)


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

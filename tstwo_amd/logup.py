"""LogUp lookups (Rust stwo constraint_framework/logup.rs): lookup elements, relation entries, and the interaction trace built on
the device (csrc/logup.hip).

Constraint side (constraint_framework.EvalAtRow): add_to_relation(RelationEntry(relation, multiplicity, values)) records the
fraction multiplicity / relation.combine(values); finalize_logup_batched groups the fractions into batches, one interaction column
each (4 base columns of INTERACTION_TRACE_IDX, one QM31 value per row).  Trace side (LogupTraceGenerator): one column per batch,
column j = column j - 1 + the batch's fractions (tstwo_logup_column, one fused launch per column), then the last column becomes the
running sum over the coset order, shifted by claimed_sum / 2^log_size so that it ends at 0 (tstwo_logup_finalize_last), which
also returns the claimed sum.

derive_interaction_trace(eval, main, preprocessed) drives the generator from `evaluate` alone: the relation entries are recorded
as they were added (constraint_framework.RelationEvaluator), every multiplicity or value that is an expression of columns becomes
one output column of one tstwo_air_eval_columns program, and the batches are written in order.  The hand-written generators
(constraint_framework.*_interaction_trace) are the same calls spelled out.

Caller protocol (the verifier mirrors it): commit the preprocessed tree, commit the main tree, LookupElements.draw, generate the
interaction trace, channel.mix_felts(claimed sums in component order), commit the interaction tree, prove.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from .backend import HipColumn, SecureColumnByCoords
from .circle import CanonicCoset
from .fields import M31, QM31, P
from .poly import HipCircleEvaluation

INTERACTION_TRACE_IDX = 2
# include/tstwo_hip.h TSTWO_LOGUP_MAX_*
MAX_FRACS, MAX_TERMS, MAX_LOG = 8, 16, 28


def _felt(v) -> QM31:
    if isinstance(v, QM31):
        return v
    if isinstance(v, M31):
        return QM31.from_(v)
    if isinstance(v, int):
        return QM31.from_(M31(int(v) % P))
    raise TypeError(f"a relation value is an int, M31 or QM31 here, not {type(v).__name__}")


class LookupElements:
    """The random elements of one relation (Rust LookupElements<N>): z, alpha and alpha_powers[i] = alpha^i, i < size."""

    def __init__(self, z: QM31, alpha: QM31, size: int):
        if size < 1:
            raise ValueError("a relation combines at least one value")
        self.z, self.alpha = z, alpha
        self.alpha_powers = [QM31.one()]
        while len(self.alpha_powers) < size:
            self.alpha_powers.append(self.alpha_powers[-1].mul(alpha))

    @staticmethod
    def draw(channel, size: int) -> "LookupElements":
        z, alpha = channel.draw_felts(2)
        return LookupElements(z, alpha, size)

    @property
    def size(self) -> int:
        return len(self.alpha_powers)

    def _values(self, values) -> list:
        values = list(values)
        if len(values) > self.size:
            raise ValueError(f"{len(values)} values for a relation of size {self.size}")
        return values

    def combine(self, values):
        """sum_i alpha^i values[i] - z.  Values inside `evaluate` (Expr / SecureExpr, PointValue) give the same kind of secure
        value back; ints, M31 and QM31 give a QM31."""
        from .constraint_framework import Expr, PointValue, SecureExpr
        values = self._values(values)
        if any(isinstance(v, (Expr, SecureExpr)) for v in values):
            acc = SecureExpr.lift(0)
            for v, p in zip(values, self.alpha_powers):
                acc = acc + SecureExpr.lift(v) * p
            return acc - self.z
        if any(isinstance(v, PointValue) for v in values):
            acc = PointValue(QM31.zero())
            for v, p in zip(values, self.alpha_powers):
                acc = acc + PointValue(PointValue._q(v)) * p
            return acc - self.z
        acc = QM31.zero()
        for v, p in zip(values, self.alpha_powers):
            acc = acc.add(p.mul(_felt(v)))
        return acc.sub(self.z)

    def combine_columns(self, values) -> "LinearForm":
        """combine() over whole device columns, for LogupColGenerator.write_frac: values are HipColumns (M31) or constants, which
        fold into the constant term here.  No device work."""
        values = self._values(values)
        terms, constant = [], self.z.neg()
        for v, p in zip(values, self.alpha_powers):
            if isinstance(v, HipColumn):
                terms.append((p, v))
            else:
                constant = constant.add(p.mul(_felt(v)))
        return LinearForm(terms, constant)

    combineColumns = combine_columns


class LinearForm:
    """sum_t coeff_t cols_t[r] + constant: M31 columns, QM31 coefficients and constant (a tstwo_logup_frac denominator)."""

    def __init__(self, terms, constant: QM31):
        self.terms, self.constant = list(terms), constant


class RelationEntry:
    """One use of a relation on a row: multiplicity / relation.combine(values) joins the row's LogUp sum."""

    def __init__(self, relation: LookupElements, multiplicity, values):
        self.relation, self.multiplicity, self.values = relation, multiplicity, list(values)


class Fraction:
    __slots__ = ("numerator", "denominator")

    def __init__(self, numerator, denominator):
        self.numerator, self.denominator = numerator, denominator


# ------------------------------------------------------------------ the device entries
def logup_column(fracs, prev: SecureColumnByCoords | None, log_size: int, out: SecureColumnByCoords) -> None:
    """tstwo_logup_column: out[r] = prev[r] (or 0) + sum num / den over fracs = [(numerator: int | M31 | HipColumn, LinearForm)]."""
    if not 1 <= len(fracs) <= MAX_FRACS:
        raise ValueError(f"1 to {MAX_FRACS} fractions per column")
    n = 1 << log_size
    descs = (L.LogupFrac * len(fracs))()
    keep = []                           # the host tables must live until the call returns
    for d, (num, form) in zip(descs, fracs):
        if not 1 <= len(form.terms) <= MAX_TERMS:
            raise ValueError(f"a denominator needs 1 to {MAX_TERMS} column terms")
        if any(col.len() != n for _, col in form.terms):
            raise ValueError("every column of a fraction must hold 2^log_size values")
        cols = L.ptr_array([col.ptr for _, col in form.terms])
        coeffs = L.u32x([w for p, _ in form.terms for w in p.tup()])
        keep += [cols, coeffs]
        d.cols, d.coeffs, d.n_terms = C.cast(cols, C.POINTER(L.vp)), C.cast(coeffs, L.u32p), len(form.terms)
        d.constant[:] = list(form.constant.tup())
        if isinstance(num, HipColumn):
            if num.len() != n:
                raise ValueError("the numerator column must hold 2^log_size values")
            d.num, d.num_const = num.ptr, 0
        else:
            d.num, d.num_const = None, (num.value if isinstance(num, M31) else int(num)) % P
    prev_ptrs = L.p4([c.ptr for c in prev.columns]) if prev is not None else None
    L.call("tstwo_logup_column", descs, len(fracs), prev_ptrs, log_size, out.ptrs())


def logup_finalize_last(col: SecureColumnByCoords, log_size: int) -> QM31:
    """tstwo_logup_finalize_last: the column becomes its shifted running sum in coset order; returns the claimed sum."""
    claimed = (C.c_uint32 * 4)()
    L.call("tstwo_logup_finalize_last", col.ptrs(), log_size, claimed)
    return QM31.from_u32_unchecked(*claimed)


ORDERS = {"natural": 0, "coset": 1}     # include/tstwo_hip.h TSTWO_LOOKUP_ORDER_*


def lookup_multiplicities(log_range: int, *value_columns, order: str = "coset", check: bool = True) -> HipColumn:
    """tstwo_lookup_multiplicities: the column of 2^log_range counts, count of k = the number of words equal to k over
    `value_columns` (HipColumns of any length, or arrays, which are uploaded).  order "coset": the count of k at the storage
    position of coset row k, a trace column beside range_check_table_column; "natural": at word k (an MLE).
    check=True reads one word back and raises ValueError when a value lies outside [0, 2^log_range); check=False reads nothing
    back and skips such values."""
    if order not in ORDERS:
        raise ValueError(f"order is 'natural' or 'coset', not {order!r}")
    cols = [c if isinstance(c, HipColumn) else HipColumn(c) for c in value_columns]
    out = HipColumn.uninitialized(1 << log_range)
    rejected = HipColumn.uninitialized(1) if check else None
    L.call("tstwo_lookup_multiplicities", L.ptr_array([c.ptr for c in cols]), (C.c_size_t * max(len(cols), 1))(*[c.len() for c in cols]),
           len(cols), log_range, ORDERS[order], out.ptr, rejected.ptr if check else None)
    if check and int(rejected.to_numpy()[0]):
        raise ValueError("a checked value lies outside the range")
    return out


MAX_LIMBS, MAX_GROUPS = 4, 64           # include/tstwo_hip.h TSTWO_LOOKUP_MAX_LIMBS / _GROUPS


class LookupGroup:
    """One tstwo_lookup_group: rows whose key is joined from limb columns, limbs = [(column, bits), ...] with the least
    significant limb first (limb j of a row must be < 2^bits_j), and an optional weight column (None: every row weighs 1; a row
    of weight 0 is skipped unchecked).  Columns are HipColumns, which stay where they are, or arrays, which are uploaded; all of
    one length."""

    def __init__(self, limbs, weight=None):
        limbs = list(limbs)
        if not 1 <= len(limbs) <= MAX_LIMBS:
            raise ValueError(f"1 to {MAX_LIMBS} limbs per group")
        self.limbs = [c if isinstance(c, HipColumn) else HipColumn(c) for c, _ in limbs]
        self.bits = [int(b) for _, b in limbs]
        if any(b < 1 for b in self.bits):
            raise ValueError("every limb needs at least 1 bit")
        self.weight = weight if weight is None or isinstance(weight, HipColumn) else HipColumn(weight)
        self.len = self.limbs[0].len()
        if any(c.len() != self.len for c in self.limbs + ([self.weight] if self.weight is not None else [])):
            raise ValueError("the columns of a group must have one length")

    @property
    def log_range(self) -> int:
        return sum(self.bits)


def lookup_multiplicities_keyed(groups, order: str = "coset", check: bool = True) -> HipColumn:
    """tstwo_lookup_multiplicities_keyed: the column of 2^log_range sums, log_range = the groups' common bit sum; the sum of
    k = a_0 + 2^bits_0 a_1 + ... is the sum of the weights of the rows with limbs (a_0, a_1, ...) over `groups` (LookupGroups),
    mod P.  order as for lookup_multiplicities.  check=True reads one word back and raises ValueError when a row of non-zero
    weight has a limb outside its width; check=False reads nothing back and skips such rows."""
    if order not in ORDERS:
        raise ValueError(f"order is 'natural' or 'coset', not {order!r}")
    groups = list(groups)
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"1 to {MAX_GROUPS} groups")
    log_range = groups[0].log_range
    if any(g.log_range != log_range for g in groups):
        raise ValueError("the bits of every group must add up to the same log_range")
    if not 1 <= log_range <= MAX_LOG:
        raise ValueError(f"log_range must be 1 to {MAX_LOG}")
    descs = (L.LookupGroup * len(groups))()
    for d, g in zip(descs, groups):
        for j, (c, b) in enumerate(zip(g.limbs, g.bits)):
            d.limbs[j], d.bits[j] = c.ptr, b
        d.n_limbs, d.weight, d.len = len(g.limbs), g.weight.ptr if g.weight is not None else None, g.len
    out = HipColumn.uninitialized(1 << log_range)
    rejected = HipColumn.uninitialized(1) if check else None
    L.call("tstwo_lookup_multiplicities_keyed", descs, len(groups), log_range, ORDERS[order], out.ptr, rejected.ptr if check else None)
    if check and int(rejected.to_numpy()[0]):
        raise ValueError("a checked value lies outside the range")
    return out


def coset_iota(log_size: int) -> HipColumn:
    """tstwo_coset_iota: value k at the storage position of coset row k (the preprocessed column of a range-check table)."""
    out = HipColumn.uninitialized(1 << log_size)
    L.call("tstwo_coset_iota", out.ptr, log_size)
    return out


# ------------------------------------------------------------------ the generator (Rust LogupTraceGenerator)
class LogupTraceGenerator:
    """The interaction trace of one component on whole device columns: new_col() per batch, write_frac() per fraction of the
    batch, finalize_col(), and finalize_last() for the evaluations (4 per batch) and the claimed sum."""

    def __init__(self, log_size: int):
        if not 1 <= log_size <= MAX_LOG:
            raise ValueError(f"log_size must be 1 to {MAX_LOG}")
        self.log_size = log_size
        self.trace = []                 # SecureColumnByCoords per finished column
        self._open = None

    def new_col(self) -> "LogupColGenerator":
        if self._open is not None:
            raise ValueError("finalize_col() the previous column first")
        self._open = LogupColGenerator(self)
        return self._open

    def finalize_last(self):
        """(HipCircleEvaluations on CanonicCoset(log_size).circle_domain(), 4 per column, claimed sum).  Raises TstwoError
        "0 has no inverse" when a denominator vanished on some row."""
        if self._open is not None:
            raise ValueError("finalize_col() the last column first")
        if not self.trace:
            raise ValueError("no interaction column was written")
        L.call("tstwo_check_zero_flag")
        claimed = logup_finalize_last(self.trace[-1], self.log_size)
        domain = CanonicCoset(self.log_size).circleDomain()
        return [HipCircleEvaluation(domain, c) for col in self.trace for c in col.columns], claimed

    newCol = new_col
    finalizeLast = finalize_last


class LogupColGenerator:
    def __init__(self, gen: LogupTraceGenerator):
        self.gen, self.fracs = gen, []

    def write_frac(self, numerator, denominator: LinearForm) -> None:
        """numerator: an int / M31 for every row, or a HipColumn (M31); denominator: LookupElements.combine_columns(...)."""
        if not isinstance(denominator, LinearForm):
            raise TypeError("the denominator is a LookupElements.combine_columns(...) form")
        if len(self.fracs) >= MAX_FRACS:
            raise ValueError(f"at most {MAX_FRACS} fractions per column")
        self.fracs.append((numerator, denominator))

    def finalize_col(self) -> None:
        if not self.fracs:
            raise ValueError("a column needs at least one fraction")
        g = self.gen
        out = SecureColumnByCoords.uninitialized(1 << g.log_size)
        logup_column(self.fracs, g.trace[-1] if g.trace else None, g.log_size, out)
        g.trace.append(out)
        g._open = None

    writeFrac = write_frac
    finalizeCol = finalize_col


# ------------------------------------------------------------------ the interaction trace derived from `evaluate`
class InteractionPlan:
    """What derive_interaction_trace does for one eval, worked out on the host: `exprs`, the distinct expressions a columns
    program evaluates (canonical nodes, in order of first use), and `batches`, per interaction column the fractions
    (relation, numerator ref, value refs) in entry order.  A ref is ("const", value), ("col", ("main" | "pre", index)) for an
    input column used as it is, or ("out", k) for exprs[k].  n_main / n_pre: the input columns `evaluate` reads."""

    def __init__(self, exprs, batches, n_main, n_pre):
        self.exprs, self.batches, self.n_main, self.n_pre = exprs, batches, n_main, n_pre


def plan_interaction_trace(eval_) -> InteractionPlan:
    """Runs `evaluate` on a RelationEvaluator and sorts every multiplicity and value into constants, input columns and
    expressions.  No device work; raises the ValueErrors of derive_interaction_trace."""
    from .constraint_framework import Canonical, Expr, SecureExpr, relation_entries
    ev = relation_entries(eval_)
    canonical, index, exprs = Canonical(), {}, []

    def ref(v, what):
        if isinstance(v, (SecureExpr, QM31)) and what == "multiplicity":
            raise ValueError("a secure (QM31) multiplicity is not supported: numerators are M31 columns or constants")
        if isinstance(v, SecureExpr):
            raise ValueError("a secure (QM31) expression as a relation value is not supported: denominator terms are M31 columns")
        if not isinstance(v, Expr):
            return ("const", v if isinstance(v, QM31) else _m31(v))
        node = canonical(v)
        if node.op == "const":
            return ("const", M31(node.args))
        if node.op == "load":
            column, offset = node.args
            if column[0] == "int":
                raise ValueError("a relation entry cannot read the interaction trace it defines")
            if offset == 0:
                return ("col", column)
        if id(node) not in index:
            index[id(node)] = len(exprs)
            exprs.append(node)
        return ("out", index[id(node)])

    fracs = []
    for relation, multiplicity, values in ev.entries:
        values = relation._values(values)
        num = ref(multiplicity, "multiplicity")
        refs = [ref(v, "value") for v in values]
        n_terms = sum(r[0] != "const" for r in refs)
        if not 1 <= n_terms <= MAX_TERMS:
            raise ValueError(f"a denominator needs 1 to {MAX_TERMS} column terms")
        fracs.append((relation, num, refs))
    batches = [[f for b, f in zip(ev.batching, fracs) if b == j] for j in range(max(ev.batching) + 1)]
    if any(len(b) > MAX_FRACS for b in batches):
        raise ValueError(f"at most {MAX_FRACS} fractions per column")
    return InteractionPlan(exprs, batches, ev.n_main, max(ev.pre_used) + 1 if ev.pre_used else 0)


def _m31(v) -> M31:
    if isinstance(v, M31):
        return v
    if isinstance(v, int):
        return M31(int(v) % P)
    raise TypeError(f"a multiplicity or relation value is an int, M31, QM31 or an expression here, not {type(v).__name__}")


def derive_interaction_trace(eval_, main, preprocessed=(), *, native: bool = False):
    """The interaction trace of a LogUp component from its `evaluate` alone: (HipCircleEvaluations, 4 per batch, claimed sum), the
    return of LogupTraceGenerator.finalize_last().  main, preprocessed: the component's columns (HipColumns, or arrays in storage
    order) in the order `evaluate` consumes them (next_trace_mask / next_interaction_mask, get_preprocessed_column(i)).
      an int or M31 multiplicity is the fraction's constant numerator; a column read at offset 0 is used as it is;
      every other expression of columns (x + 1, a * b - c, a value at another row, -multiplicity), as a multiplicity or as a value,
      is one output of a tstwo_air_eval_columns program (equal expressions share one; more than 64 take several calls);
      constant values fold into the denominator's constant as LookupElements.combine_columns folds them.
    native=True (opt-in): every columns program runs as a native kernel (evaluate_columns(..., native=True)); same columns, same sum.
    Nothing is read back before finalize_last.  Raises ValueError for an `evaluate` without relation entries, an entry without a
    column among its values, a secure (QM31) multiplicity, more than 8 fractions in a batch or more than 16 column values."""
    from .constraint_framework import MAX_OUT, compile_columns, evaluate_columns
    plan = plan_interaction_trace(eval_)
    log_size = eval_.log_size()
    gen = LogupTraceGenerator(log_size)
    main = [c if isinstance(c, HipColumn) else HipColumn(c) for c in main]
    pre = [c if isinstance(c, HipColumn) else HipColumn(c) for c in preprocessed]
    if len(main) != plan.n_main:
        raise ValueError(f"evaluate reads {plan.n_main} main columns, {len(main)} given")
    if len(pre) < plan.n_pre:
        raise ValueError(f"evaluate reads {plan.n_pre} preprocessed columns, {len(pre)} given")
    outs = []
    for i in range(0, len(plan.exprs), MAX_OUT):
        chunk = plan.exprs[i:i + MAX_OUT]
        outs += evaluate_columns(main + pre, log_size, compile_columns(chunk, len(main), len(pre)), len(chunk), native=native)

    def resolve(r):
        kind, x = r
        return x if kind == "const" else outs[x] if kind == "out" else (main if x[0] == "main" else pre)[x[1]]

    for batch in plan.batches:
        col = gen.new_col()
        for relation, num, refs in batch:
            col.write_frac(resolve(num), relation.combine_columns([resolve(r) for r in refs]))
        col.finalize_col()
    return gen.finalize_last()


deriveInteractionTrace = derive_interaction_trace

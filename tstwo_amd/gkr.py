"""LogUp-GKR on the device: GkrOps / MleOps (backend/cpu/lookups/{gkr,mle}.ts), the prover's Layer / EqEvals /
GkrMultivariatePolyOracle (lookups/gkr_prover.ts) and prove_batch (gkr_prover.ts:440-580).

MLEs live in HBM: an Mle<SecureField> is a SecureColumnByCoords (4 SoA columns), an Mle<BaseField> one HipColumn; the first
variable is the most significant bit of the index.  Every pass over 2^n values is a kernel of csrc/gkr_ops.hip; the host keeps the
O(layers) protocol (sumcheck.py) and the channel between the layers.

prove_batch enqueues a whole layer without reading anything back where it can (a Blake2s channel with the Rust draw semantics, at
most 64 instances): per round one fused fold + sum launch per active instance, then one tstwo_gkr_round_finish launch that does
what the host would do between two rounds (round polynomials, their combination, the channel, the new claims and corrections) and
leaves the challenge in device memory for the next round's fold; per layer one upload and one read-back (channel, round
polynomials, assignment, masks).  Elsewhere, and with device_rounds=False, the protocol of a round runs on the host: one read-back
per round (the (f(0), f(2)) slots of every active instance) and one per layer (the 2-point masks).  The first read-back also takes
every instance's output values and first mask.  prove_batch(one_call=True) hands the whole proof to tstwo_gkr_prove_batch: the
transcript between the layers stays on the device too, and one block (channel, claims, round polynomials, masks, the final point)
is read back at the end.

The two ends: logup_input_layer builds a LogUp input layer from M31 trace columns (denominators sum_i alpha^i col_i - z by
tstwo_gkr_logup_denominators; numerators none, a base column or a secure MLE), and verify_input_claims checks what
partially_verify_batch leaves open — each input layer evaluated at the artifact's point by Mle.eval_at_point, one pass over the
values on the device (csrc/mle_eval.hip) — with check_logup_sum for the fractions the LogUp instances output.  gkr_lookup.py runs
a range check through all of it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .backend import HipColumn, SecureColumnByCoords
from .fields import M31, QM31
from .gkr_verifier import GkrArtifact, GkrBatchProof, GkrMask
from .sumcheck import (SumcheckProof, UnivariatePoly, _qadd, _qinv, _qmul, _qsub, _Z, combine, eq, fold_mle_evals,
                       random_linear_combination)

GRAND_PRODUCT, LOGUP_GENERIC, LOGUP_MULTIPLICITIES, LOGUP_SINGLES = 0, 1, 2, 3      # TSTWO_GKR_* (include/tstwo_hip.h)
_KIND_NAMES = {GRAND_PRODUCT: "GrandProduct", LOGUP_GENERIC: "LogUpGeneric", LOGUP_MULTIPLICITIES: "LogUpMultiplicities",
               LOGUP_SINGLES: "LogUpSingles"}


def _q(v: QM31):
    return L.u32x(v.tup())


def _qs(words):
    return QM31.from_u32_unchecked(*[int(w) for w in words])


def _log2(n: int) -> int:
    if n <= 0 or n & (n - 1):
        raise ValueError("length is not power of two")
    return n.bit_length() - 1


class Mle:
    """Mle<SecureField> (SecureColumnByCoords) or Mle<BaseField> (HipColumn) in device memory (lookups/mle.ts)."""

    def __init__(self, col):
        self.col = col
        self.is_base = isinstance(col, HipColumn)
        self._nv = _log2(col.len())

    @staticmethod
    def secure(cols4) -> "Mle":
        """From 4 coordinate arrays (numpy) or a SecureColumnByCoords."""
        return Mle(cols4 if isinstance(cols4, SecureColumnByCoords) else SecureColumnByCoords.from_numpy([np.asarray(c, dtype=np.uint32) for c in cols4]))

    @staticmethod
    def base(values) -> "Mle":
        return Mle(values if isinstance(values, HipColumn) else HipColumn(np.asarray(values, dtype=np.uint32)))

    @staticmethod
    def uninitialized_secure(n: int) -> "Mle":
        return Mle(SecureColumnByCoords.uninitialized(n))

    def n_variables(self) -> int:
        return self._nv

    nVariables = n_variables

    def len(self) -> int:
        return 1 << self._nv

    def ptrs(self):
        """The 4 column pointers (a base column repeats its one pointer)."""
        return L.p4([self.col.ptr] * 4) if self.is_base else self.col.ptrs()

    def ptr_list(self):
        return [self.col.ptr] if self.is_base else [c.ptr for c in self.col.columns]

    def to_numpy(self):
        """(n,) for a base MLE, (4, n) for a secure one."""
        return self.col.to_numpy() if self.is_base else np.stack(self.col.to_numpy())

    def at(self, i: int) -> QM31:
        return QM31.from_(self.col.at(i)) if self.is_base else self.col.at(i)

    def fix_first_variable(self, r: QM31) -> "Mle":
        return HipMleOps.fixFirstVariable(self, r)

    fixFirstVariable = fix_first_variable

    def eval_at_point(self, point) -> QM31:
        """Mle.evalAtPoint (lookups/mle.ts:81-114): one pass over the values on the device, one read-back."""
        return eval_mles_at_point([self], point)[0]

    evalAtPoint = eval_at_point

    def free(self) -> None:
        for c in ([self.col] if self.is_base else self.col.columns):
            c.buf.free()


def eval_mles_at_point(mles, point):
    """Mle.evalAtPoint of several MLEs at one point (tstwo_mle_eval_at_point_base / _secure): one call, and one read-back, per
    kind and size; the values come back in input order.  A point whose length is not an MLE's n_variables() raises ValueError (Rust
    asserts it; the reference misbehaves silently)."""
    mles, point = list(mles), list(point)
    groups = {}
    for i, m in enumerate(mles):
        if m.n_variables() != len(point):
            raise ValueError(f"a point of {len(point)} coordinates for an MLE of {m.n_variables()} variables")
        groups.setdefault((m.is_base, m.n_variables()), []).append(i)
    words = L.u32x([w for p in point for w in p.tup()])
    out = [None] * len(mles)
    for (is_base, n), idx in groups.items():
        res = (C.c_uint32 * (4 * len(idx)))()
        L.call("tstwo_mle_eval_at_point_base" if is_base else "tstwo_mle_eval_at_point_secure",
               L.ptr_array([p for i in idx for p in mles[i].ptr_list()]), len(idx), n, words, res)
        for k, i in enumerate(idx):
            out[i] = _qs(res[4 * k:4 * k + 4])
    return out


class Layer:
    """gkr_prover.ts Layer: GrandProduct(data) | LogUpGeneric(num, den) | LogUpMultiplicities(base num, den) | LogUpSingles(den).
    `den` holds the product column of a grand-product layer."""

    def __init__(self, kind: int, num: Mle | None, den: Mle):
        if kind not in _KIND_NAMES:
            raise ValueError(f"unknown layer kind {kind}")
        if kind in (LOGUP_GENERIC, LOGUP_MULTIPLICITIES):
            if num is None or num.n_variables() != den.n_variables() or num.is_base != (kind == LOGUP_MULTIPLICITIES):
                raise ValueError("numerators must match the denominators (base for LogUpMultiplicities, secure otherwise)")
        if den.is_base:
            raise ValueError("denominators / products are secure MLEs")
        self.kind, self.num, self.den = kind, (num if kind in (LOGUP_GENERIC, LOGUP_MULTIPLICITIES) else None), den

    @staticmethod
    def grand_product(data: Mle) -> "Layer": return Layer(GRAND_PRODUCT, None, data)
    @staticmethod
    def logup_generic(num: Mle, den: Mle) -> "Layer": return Layer(LOGUP_GENERIC, num, den)
    @staticmethod
    def logup_multiplicities(num: Mle, den: Mle) -> "Layer": return Layer(LOGUP_MULTIPLICITIES, num, den)
    @staticmethod
    def logup_singles(den: Mle) -> "Layer": return Layer(LOGUP_SINGLES, None, den)

    @property
    def type(self) -> str:
        return _KIND_NAMES[self.kind]

    def n_variables(self) -> int:
        return self.den.n_variables()

    nVariables = n_variables

    def is_output_layer(self) -> bool:
        return self.n_variables() == 0

    def next_layer(self) -> "Layer | None":
        return HipGkrOps.nextLayer(self)

    def columns(self):
        return [m for m in (self.num, self.den) if m is not None]

    def try_into_output_layer_values(self):
        """gkr_prover.ts tryIntoOutputLayerValues."""
        if not self.is_output_layer():
            raise ValueError("Layer is not an output layer")
        return _output_values(self, [m.at(0).tup() for m in self.columns()])

    def fix_first_variable(self, x0: QM31) -> "Layer":
        """gkr_prover.ts:195-222: LogUpMultiplicities becomes LogUpGeneric."""
        if self.n_variables() == 0:
            return self
        kind = LOGUP_GENERIC if self.kind == LOGUP_MULTIPLICITIES else self.kind
        num = self.num.fix_first_variable(x0) if self.num is not None else None
        return Layer(kind, num, self.den.fix_first_variable(x0))

    def eval_at_point(self, point):
        """The layer's columns at `point`, in mask order: [den] for a grand product, [num, den] for LogUp, [1, den] for
        LogUpSingles — what partially_verify_batch leaves in claims_to_verify_by_instance."""
        vals = eval_mles_at_point(self.columns(), point)
        return [QM31.one()] + vals if self.kind == LOGUP_SINGLES else vals

    evalAtPoint = eval_at_point

    def into_multivariate_poly(self, lam: QM31, eq_evals: "EqEvals") -> "GkrMultivariatePolyOracle":
        return GkrMultivariatePolyOracle(eq_evals, self, QM31.one(), lam)

    def free(self) -> None:
        for m in self.columns():
            m.free()


def _output_values(layer: Layer, words):
    """Output values from the first word(s) of each column (num first): gkr_prover.ts tryIntoOutputLayerValues."""
    if layer.kind == GRAND_PRODUCT:
        return [_qs(words[0])]
    if layer.kind == LOGUP_SINGLES:
        return [QM31.one(), _qs(words[0])]
    n = words[0]
    num = QM31.from_u32_unchecked(int(n[0]), 0, 0, 0) if layer.kind == LOGUP_MULTIPLICITIES else _qs(n)
    return [num, _qs(words[1])]


def _mask_of(layer: Layer, pairs) -> GkrMask:
    """tryIntoMask (gkr_prover.ts:353-395) from the two values of each column of a 1-variable layer (num first)."""
    if layer.kind == LOGUP_MULTIPLICITIES:
        raise NotImplementedError("LogUpMultiplicities should never reach tryIntoMask")
    cols = [(_qs(a), _qs(b)) for a, b in pairs]
    if layer.kind == LOGUP_SINGLES:
        cols = [(QM31.one(), QM31.one())] + cols
    return GkrMask(cols)


def _read_pairs(layer: Layer, count: int):
    """Pieces for download_many: the first `count` words of each coordinate column (num first, den second)."""
    pieces = []
    for m in layer.columns():
        pieces += [(p, count) for p in m.ptr_list()]
    return pieces


def _unpack(layer: Layer, words, count: int):
    """Inverse of _read_pairs: per column, `count` QM31 values as 4-tuples."""
    out, k = [], 0
    for m in layer.columns():
        w = len(m.ptr_list())
        cols = words[k:k + w]
        k += w
        out.append([tuple(int(c[j]) for c in cols) + (0,) * (4 - w) for j in range(count)])
    return out


class EqEvals:
    """eq((0, x), y) for x in {0,1}^(|y|-1) (gkr_prover.ts:38-95 with Rust's generate)."""

    def __init__(self, y, evals: Mle):
        self.y, self.evals = list(y), evals

    @staticmethod
    def generate(y) -> "EqEvals":
        y = list(y)
        if not y:
            return EqEvals(y, HipGkrOps.genEqEvals([], QM31.one()))
        return EqEvals(y, HipGkrOps.genEqEvals(y[1:], eq([QM31.zero()], [y[0]])))

    def get_y(self):
        return list(self.y)

    getY = get_y

    def at(self, i: int) -> QM31:
        return self.evals.at(i)

    def len(self) -> int:
        return self.evals.len()

    def free(self) -> None:
        self.evals.free()


def correct_sum_as_poly_in_first_variable(f0: QM31, f2: QM31, claim: QM31, y, k: int) -> UnivariatePoly:
    """gkr_prover.ts:609-660: r(t) = f(t) eq(t, y[n-k]) / eq(0, y[:n-k+1]) through r(0), r(1) = claim - r(0), r(2), r(b) = 0."""
    n = len(y)
    if k == 0:
        raise ValueError("k must not be 0")
    if k > n:
        raise ValueError("k must not exceed y.length")
    one, two = (1, 0, 0, 0), (2, 0, 0, 0)
    e0 = one                                             # eq({0}^(n-k+1), y[:n-k+1]) = prod (1 - y_j)
    for yj in y[:n - k + 1]:
        e0 = _qmul(e0, _qsub(one, yj.tup()))
    a = _qinv(e0)
    yk = y[n - k].tup()
    b = _qmul(_qsub(one, yk), _qinv(_qsub(one, _qadd(yk, yk))))
    r0 = _qmul(_qmul(f0.tup(), _qsub(one, yk)), a)      # eq([0], [yk]) = 1 - yk
    r1 = _qsub(claim.tup(), r0)
    r2 = _qmul(_qmul(f2.tup(), _eq2(yk)), a)
    q = lambda t: QM31.from_u32_unchecked(*t)           # noqa: E731
    return UnivariatePoly.interpolate_lagrange([q(_Z), q(one), q(two), q(b)], [q(r0), q(r1), q(r2), q(_Z)])


def _eq2(yk):
    """eq([2], [yk]) = 2 yk + (1 - 2)(1 - yk) = 3 yk - 1."""
    return _qsub(_qadd(_qadd(yk, yk), yk), (1, 0, 0, 0))


class GkrMultivariatePolyOracle:
    """gkr_prover.ts:290-420: P(x) = eq(x, y) * gate(input layer at (x, 0), (x, 1)), LogUp combined with lambda."""

    def __init__(self, eq_evals: EqEvals, input_layer: Layer, eq_fixed_var_correction: QM31, lam: QM31):
        self.eq_evals, self.input_layer, self.eq_fixed_var_correction, self.lam = eq_evals, input_layer, eq_fixed_var_correction, lam

    def n_variables(self) -> int:
        return self.input_layer.n_variables() - 1

    nVariables = n_variables

    def sum_as_poly_in_first_variable(self, claim: QM31) -> UnivariatePoly:
        return HipGkrOps.sumAsPolyInFirstVariable(self, claim)

    sumAsPolyInFirstVariable = sum_as_poly_in_first_variable

    def _next_correction(self, challenge: QM31) -> QM31:
        y = self.eq_evals.y
        return self.eq_fixed_var_correction.mul(eq([challenge], [y[len(y) - self.n_variables()]]))

    def fix_first_variable(self, challenge: QM31) -> "GkrMultivariatePolyOracle":
        if self.is_constant():
            return self
        return GkrMultivariatePolyOracle(self.eq_evals, self.input_layer.fix_first_variable(challenge),
                                         self._next_correction(challenge), self.lam)

    fixFirstVariable = fix_first_variable

    def is_constant(self) -> bool:
        return self.n_variables() == 0

    def try_into_mask(self) -> GkrMask:
        if not self.is_constant():
            raise ValueError("Polynomial is not constant")
        lay = self.input_layer
        return _mask_of(lay, [tuple(c) for c in _unpack(lay, L.download_many(_read_pairs(lay, 2)), 2)])

    tryIntoMask = try_into_mask


class HipMleOps:
    """MleOps<BaseField> / MleOps<SecureField> (backend/cpu/lookups/mle.ts:60-130)."""

    @staticmethod
    def fixFirstVariable(mle: Mle, assignment: QM31) -> Mle:
        """Returns the MLE with its first variable fixed to `assignment` (a new secure MLE of half the length)."""
        n = mle.n_variables()
        if n == 0:
            raise ValueError("cannot fix the first variable of a constant MLE")
        out = Mle.uninitialized_secure(1 << (n - 1))
        HipMleOps.fix_first_variable_into(mle, assignment, out)
        return out

    @staticmethod
    def fix_first_variable_into(mle: Mle, assignment, out: Mle) -> None:
        """The same into `out` (may be `mle` itself for a secure MLE: in place, the first half of its columns).  `assignment`: a
        QM31, or the device address (int) of 4 words written earlier on the stream."""
        if isinstance(assignment, int):
            if mle.is_base:
                L.call("tstwo_mle_fix_first_variable_base_dev", C.c_void_p(mle.col.ptr), mle.n_variables(), C.c_void_p(assignment), out.ptrs())
            else:
                L.call("tstwo_mle_fix_first_variable_secure_dev", mle.ptrs(), mle.n_variables(), C.c_void_p(assignment), out.ptrs())
        elif mle.is_base:
            L.call("tstwo_mle_fix_first_variable_base", C.c_void_p(mle.col.ptr), mle.n_variables(), _q(assignment), out.ptrs())
        else:
            L.call("tstwo_mle_fix_first_variable_secure", mle.ptrs(), mle.n_variables(), _q(assignment), out.ptrs())


    @staticmethod
    def evalAtPoint(mle: Mle, point) -> QM31:
        """Mle.evalAtPoint (lookups/mle.ts:81-114) on the device."""
        return mle.eval_at_point(point)


# ---------------------------------------------------------------- input layers from trace columns, and the claims on them
class GkrInputClaimMismatch(Exception):
    """An input layer does not take the value the GKR artifact claims for it at the out-of-domain point."""

    def __init__(self, instance: int, column: int):
        super().__init__(f"input layer of instance {instance}: column {column} does not evaluate to its claim")
        self.instance, self.column = instance, column


def logup_denominators(form) -> Mle:
    """tstwo_gkr_logup_denominators: the LinearForm sum_t coeff_t cols_t[r] + constant written out as a secure MLE (asynchronous;
    the row order of the columns is the order of the MLE)."""
    from .logup import MAX_TERMS
    if not 1 <= len(form.terms) <= MAX_TERMS:
        raise ValueError(f"a denominator needs 1 to {MAX_TERMS} column terms")
    n = form.terms[0][1].len()
    if any(col.len() != n for _, col in form.terms):
        raise ValueError("the columns of a denominator must have one length")
    out = Mle.uninitialized_secure(n)
    L.call("tstwo_gkr_logup_denominators", L.ptr_array([col.ptr for _, col in form.terms]),
           L.u32x([w for p, _ in form.terms for w in p.tup()]), len(form.terms), _q(form.constant), _log2(n), out.ptrs())
    return out


def logup_input_layer(form_or_relation, values=None, numerators=None) -> Layer:
    """A LogUp input layer over trace columns.  The denominators are a logup.LinearForm, or relation.combine_columns(values) of a
    logup.LookupElements (sum_i alpha^i values_i - z).  numerators: None = LogUpSingles; a HipColumn or a base Mle =
    LogUpMultiplicities; a secure Mle = LogUpGeneric."""
    from .logup import LinearForm
    if isinstance(form_or_relation, LinearForm):
        if values is not None:
            raise ValueError("values go with a relation, not with a LinearForm")
        form = form_or_relation
    else:
        if values is None:
            raise ValueError("a relation needs the values it combines")
        form = form_or_relation.combine_columns(values)
    den = logup_denominators(form)
    if numerators is None:
        return Layer.logup_singles(den)
    num = numerators if isinstance(numerators, Mle) else Mle.base(numerators)
    return Layer.logup_multiplicities(num, den) if num.is_base else Layer.logup_generic(num, den)


def verify_input_claims(artifact: GkrArtifact, layers) -> None:
    """The check partially_verify_batch leaves open: input layer i, evaluated on the device at the last n_i coordinates of
    artifact.ood_point, gives claims_to_verify_by_instance[i].  Raises GkrInputClaimMismatch(instance, column)."""
    layers = list(layers)
    if len(layers) != len(artifact.n_variables_by_instance):
        raise ValueError(f"{len(layers)} input layers for {len(artifact.n_variables_by_instance)} instances")
    n = max(artifact.n_variables_by_instance)
    for i, (lay, nv, claims) in enumerate(zip(layers, artifact.n_variables_by_instance, artifact.claims_to_verify_by_instance)):
        if lay.n_variables() != nv:
            raise ValueError(f"input layer {i} has {lay.n_variables()} variables, the artifact says {nv}")
        got = lay.eval_at_point(artifact.ood_point[n - nv:])
        if len(got) != len(claims):
            raise ValueError(f"input layer {i} has {len(got)} columns, the artifact claims {len(claims)}")
        for col, (g, want) in enumerate(zip(got, claims)):
            if g.tup() != want.tup():
                raise GkrInputClaimMismatch(i, col)


def check_logup_sum(output_claims_by_instance, gates, claimed: QM31 | None = None) -> None:
    """The fractions (numerator, denominator) the LogUp instances output add up to `claimed` (zero by default).  Host only, by
    cross-multiplication: N / D = sum n_i / d_i is kept as (N, D) and nothing is inverted.  Raises InvalidLogupSum, also for a
    zero denominator (prover.InvalidLogupSum: the error of the STARK's own LogUp sum check)."""
    from .gkr_verifier import Gate
    from .prover import InvalidLogupSum
    claimed = QM31.zero() if claimed is None else claimed
    num, den = QM31.zero(), QM31.one()
    for out, gate in zip(output_claims_by_instance, gates):
        if gate is not Gate.LogUp:
            continue
        n_i, d_i = out
        if d_i.tup() == _Z:
            raise InvalidLogupSum("a LogUp instance outputs the denominator zero")
        num, den = num.mul(d_i).add(n_i.mul(den)), den.mul(d_i)
    if num.tup() != claimed.mul(den).tup():
        raise InvalidLogupSum("the LogUp fractions do not add up to the claimed sum")


_NULL4 = None


def _null4():
    global _NULL4
    if _NULL4 is None:
        _NULL4 = L.p4([0, 0, 0, 0])
    return _NULL4


class HipGkrOps:
    """GkrOps (backend/index.ts:93-95; backend/cpu/lookups/gkr.ts:84-178) on the GPU."""

    @staticmethod
    def genEqEvals(y, v: QM31) -> Mle:
        """eq(x, y) * v for all x in {0,1}^|y| (first variable = most significant bit)."""
        out = Mle.uninitialized_secure(1 << len(y))
        words = np.array([w for yi in y for w in yi.tup()] or [0], dtype=np.uint32)
        L.call("tstwo_gkr_gen_eq_evals", words.ctypes.data_as(L.u32p), len(y), _q(v), out.ptrs())
        return out

    @staticmethod
    def nextLayer(layer: Layer) -> Layer | None:
        n = layer.n_variables()
        if n == 0:
            return None
        if layer.kind == GRAND_PRODUCT:
            out = Mle.uninitialized_secure(1 << (n - 1))
            L.call("tstwo_gkr_next_layer_grand_product", layer.den.ptrs(), n, out.ptrs())
            return Layer(GRAND_PRODUCT, None, out)
        num, den = Mle.uninitialized_secure(1 << (n - 1)), Mle.uninitialized_secure(1 << (n - 1))
        L.call("tstwo_gkr_next_layer_logup", layer.kind, layer.num.ptrs() if layer.num else _null4(), layer.den.ptrs(), n,
               num.ptrs(), den.ptrs())
        return Layer(LOGUP_GENERIC, num, den)

    @staticmethod
    def sum_f0_f2(h: GkrMultivariatePolyOracle):
        """The raw (f(0), f(2)) of the layer's round sum, before the correction (one synchronous launch)."""
        lay = h.input_layer
        out = np.zeros(8, dtype=np.uint32)
        L.call("tstwo_gkr_sum_poly", lay.kind, h.eq_evals.evals.ptrs(), lay.num.ptrs() if lay.num else _null4(), lay.den.ptrs(),
               h.n_variables(), _q(h.lam), out.ctypes.data_as(L.u32p))
        return _qs(out[:4]), _qs(out[4:])

    @staticmethod
    def sumAsPolyInFirstVariable(h: GkrMultivariatePolyOracle, claim: QM31) -> UnivariatePoly:
        """f(t) = sum_x h(t, x) (gkr.ts:142-178); fails with "Number of variables must not be zero" for a constant oracle."""
        k = h.n_variables()
        if k < 0:
            raise ValueError("the oracle's input layer is an output layer")
        f0, f2 = HipGkrOps.sum_f0_f2(h)
        c = h.eq_fixed_var_correction
        return correct_sum_as_poly_in_first_variable(f0.mul(c), f2.mul(c), claim, h.eq_evals.y, k)


# ---------------------------------------------------------------- prove_batch (gkr_prover.ts:440-580)
class _Instance:
    """Per-instance prover state of one GKR layer: the layer being reduced, its correction, and where its round goes."""

    def __init__(self, idx: int, layer: Layer, owned: bool, lam: QM31, slot: int):
        self.idx, self.layer, self.owned, self.lam, self.slot = idx, layer, owned, lam, slot
        self.correction = QM31.one()
        self.pending = None              # challenge not yet applied to the device layer: a QM31, or the device address of its 4 words

    def n_vars(self) -> int:             # the oracle's variables still to fix
        return self.layer.n_variables() - 1 - (1 if self.pending is not None else 0)

    def _fold_target(self):
        """Columns the next fold writes: in place for a layer the prover owns, new buffers for the caller's input (and for base
        numerators, which become secure)."""
        n = self.layer.n_variables() - 1
        lay = self.layer
        if self.owned and lay.kind != LOGUP_MULTIPLICITIES:
            return lay.num, lay.den
        num = Mle.uninitialized_secure(1 << n) if lay.num is not None else None
        den = lay.den if self.owned else Mle.uninitialized_secure(1 << n)
        return num, den

    def _replace(self, num, den):
        old = self.layer
        kind = LOGUP_GENERIC if old.kind == LOGUP_MULTIPLICITIES else old.kind
        if self.owned and old.num is not None and old.num is not num:
            old.num.free()
        n = old.n_variables() - 1
        self.layer = Layer(kind, _shrink(num, n) if num is not None else None, _shrink(den, n))
        self.owned = True

    def launch_round(self, eq_evals: EqEvals, slots) -> None:
        """Enqueue this round's (f(0), f(2)) into its slot, folding in the pending challenge first (one launch)."""
        lay = self.layer
        out_ptr = C.c_void_p(slots.ptr + 32 * self.slot)
        num_p = lay.num.ptrs() if lay.num else _null4()
        if self.pending is None:
            L.call("tstwo_gkr_sum_poly_async", lay.kind, eq_evals.evals.ptrs(), num_p, lay.den.ptrs(), self.n_vars(), _q(self.lam), out_ptr)
            return
        k = self.n_vars()
        num, den = self._fold_target()
        if isinstance(self.pending, int):
            L.call("tstwo_gkr_round_dev", lay.kind, eq_evals.evals.ptrs(), num_p, lay.den.ptrs(), num.ptrs() if num else _null4(),
                   den.ptrs(), k, C.c_void_p(self.pending), _q(self.lam), out_ptr)
        else:
            L.call("tstwo_gkr_round", lay.kind, eq_evals.evals.ptrs(), num_p, lay.den.ptrs(), num.ptrs() if num else _null4(), den.ptrs(),
                   k, _q(self.pending), _q(self.lam), out_ptr)
        self._replace(num, den)
        self.pending = None

    def apply_pending(self) -> None:
        """The last challenge of the layer: a plain fold leaves the 2-point layer the mask is read from."""
        if self.pending is None:
            return
        num, den = self._fold_target()
        lay = self.layer
        if lay.num is not None:
            HipMleOps.fix_first_variable_into(lay.num, self.pending, num)
        HipMleOps.fix_first_variable_into(lay.den, self.pending, den)
        self._replace(num, den)
        self.pending = None

    def fix(self, challenge: QM31, y) -> None:
        self.correction = self.correction.mul(eq([challenge], [y[len(y) - self.n_vars()]]))
        self.pending = challenge


def _shrink(m: Mle, n_vars: int) -> Mle:
    """The same device columns seen as an MLE of n_vars variables (their first 2^n_vars words)."""
    if m.n_variables() == n_vars:
        return m
    cols = [HipColumn(_buf=c.buf, _len=1 << n_vars) for c in m.col.columns]
    return Mle(SecureColumnByCoords(cols))


def _gen_layers(layer: Layer):
    out = [layer]
    while (nxt := HipGkrOps.nextLayer(out[-1])) is not None:
        out.append(nxt)
    return out


def _host_rounds(channel, insts, claims, eq_evals, alpha: QM31, n_rounds: int, slots):
    """The layer's batched sum-check (sumcheck.ts proveBatch) with the protocol on the host: one read-back per round (the sums of
    the active instances).  Returns (round polynomials, assignment); `claims` is updated in place."""
    half = QM31.from_u32_unchecked(2, 0, 0, 0).inverse()
    round_polys, assignment = [], []
    for rnd in range(n_rounds):
        rem = n_rounds - rnd
        active = [sc for _, sc, _ in insts if sc is not None and sc.n_vars() == rem]
        for sc in active:
            sc.launch_round(eq_evals, slots)
        words = L.download_many([(slots.ptr, 8 * len(insts))])[0] if active else None
        polys = []
        for i, sc, _ in insts:
            if sc is not None and sc in active:
                f = words[8 * sc.slot:8 * sc.slot + 8]
                f0, f2 = _qs(f[:4]).mul(sc.correction), _qs(f[4:]).mul(sc.correction)
                polys.append(correct_sum_as_poly_in_first_variable(f0, f2, claims[i], eq_evals.y, rem))
            else:
                polys.append(UnivariatePoly.from_(claims[i].mul(half)))
        rp = combine(polys, alpha)
        channel.mix_felts(rp.coeffs)
        ch = channel.draw_felt()
        for (i, _, _), p in zip(insts, polys):
            claims[i] = p.eval_at_point(ch)
        for sc in active:
            sc.fix(ch, eq_evals.y)
        round_polys.append(rp)
        assignment.append(ch)
    return round_polys, assignment


MAX_DEVICE_INSTANCES = 64           # one lane of tstwo_gkr_round_finish's wave per instance
_HALF, _THIRD = (1 << 30, 0, 0, 0), (0x55555555, 0, 0, 0)
DEGENERATE_EQ_POINTS = (_Z, (1, 0, 0, 0), _HALF, _THIRD)      # y_k at which correct_sum_as_poly_in_first_variable divides by zero


def inv_eq0_table(y):
    """a of correct_sum_as_poly_in_first_variable for every round of a layer: entry r = 1 / eq({0}^(r+1), y[:r+1]), from prefix
    products and ONE inversion (Montgomery's trick).  4-tuples in, 4-tuples out; a zero eq raises like the inversion it replaces."""
    one = (1, 0, 0, 0)
    pre, acc = [], one                   # pre[r] = prod_{j <= r} (1 - y_j)
    for yj in y:
        acc = _qmul(acc, _qsub(one, yj))
        pre.append(acc)
    prods, acc = [], one                 # prods[r] = pre[0] ... pre[r]
    for e in pre:
        if e == _Z:
            raise ZeroDivisionError("0 has no inverse")
        acc = _qmul(acc, e)
        prods.append(acc)
    inv = _qinv(acc) if pre else one
    out = [None] * len(pre)
    for r in range(len(pre) - 1, -1, -1):
        out[r] = _qmul(inv, prods[r - 1]) if r else inv
        inv = _qmul(inv, pre[r])
    return out


def round_finish(chan_ptr: int, sums_ptr: int, state_ptr: int, n_instances: int, active_mask: int, y_k, inv_eq0, alpha,
                 round_poly_ptr: int, challenge_ptr: int) -> None:
    """tstwo_gkr_round_finish: the end of one sum-check round on the device (asynchronous).  Scalars are 4-tuples.  Raises the host
    path's ZeroDivisionError for an eq point at which it divides by zero, before anything is launched."""
    if tuple(y_k) in DEGENERATE_EQ_POINTS:
        raise ZeroDivisionError("0 has no inverse")
    v = C.c_void_p
    L.call("tstwo_gkr_round_finish", v(chan_ptr), v(sums_ptr), v(state_ptr), n_instances, C.c_uint64(active_mask), L.u32x(y_k),
           L.u32x(inv_eq0), L.u32x(alpha), v(round_poly_ptr), v(challenge_ptr))


class _DeviceRounds:
    """The buffers of prove_batch's device path, allocated once: one block holding the channel (16 words), every instance's
    (claim, correction) (8 words each), the round polynomials (20 words a round) and the assignment (4 words a round), so that a
    layer costs one upload (channel + claims) and one read-back (the whole block + the masks)."""

    def __init__(self, channel, n_inst: int, max_rounds: int):
        from .channel import DeviceChannel
        self.n_inst, self.max_rounds = n_inst, max_rounds
        self.state_off, self.poly_off = 16, 16 + 8 * n_inst
        self.assign_off = self.poly_off + 20 * max_rounds
        self.words = self.assign_off + 4 * max_rounds
        self.buf = L.DeviceBuffer(4 * self.words)
        self.chan = DeviceChannel(channel, self.buf)

    def ptr(self, word: int) -> int:
        return self.buf.ptr + 4 * word

    def free(self) -> None:
        self.buf.free()

    def run_layer(self, channel, insts, claims, n_v_of, eq_evals: EqEvals, alpha: QM31, n_rounds: int, slots):
        """Enqueues the layer's rounds and the last fold.  Returns the pieces to read back (the block first)."""
        y = [v.tup() for v in eq_evals.y]
        inv_eq0 = inv_eq0_table(y)
        if any(v in DEGENERATE_EQ_POINTS for v in y):
            raise ZeroDivisionError("0 has no inverse")
        state = np.zeros(8 * len(insts), dtype=np.uint32)
        for j, (i, _, _) in enumerate(insts):
            state[8 * j:8 * j + 4] = claims[i].tup()
            state[8 * j + 4] = 1
        self.chan.load(channel, tail=state)
        alpha_t = alpha.tup()
        for rnd in range(n_rounds):
            rem = n_rounds - rnd
            mask = 0
            for j, (i, sc, _) in enumerate(insts):
                if sc is None or n_v_of[i] < rem:
                    continue
                mask |= 1 << j
                sc.launch_round(eq_evals, slots)
                sc.pending = self.ptr(self.assign_off + 4 * rnd)        # the challenge this round is about to draw
            round_finish(self.ptr(0), slots.ptr, self.ptr(self.state_off), len(insts), mask, y[rnd], inv_eq0[rnd], alpha_t,
                         self.ptr(self.poly_off + 20 * rnd), self.ptr(self.assign_off + 4 * rnd))
        return [(self.buf.ptr, self.words)]

    def unpack(self, words, n_rounds: int):
        """The block as read back: continues the host channel from the device state; returns (round polynomials, assignment)."""
        self.chan.sync_to_host(words[:10])
        round_polys, assignment = [], []
        for rnd in range(n_rounds):
            p = words[self.poly_off + 20 * rnd:self.poly_off + 20 * rnd + 20]
            round_polys.append(UnivariatePoly([_qs(p[4 + 4 * k:8 + 4 * k]) for k in range(int(p[0]))]))
            assignment.append(_qs(words[self.assign_off + 4 * rnd:self.assign_off + 4 * rnd + 4]))
        return round_polys, assignment


def device_rounds_supported(channel, n_instances: int) -> bool:
    """Whether prove_batch can run its sum-check rounds on the device: a Blake2s channel with the Rust draw semantics and at most
    64 instances."""
    from .channel import Blake2sChannel
    return isinstance(channel, Blake2sChannel) and not channel.ts_compat and n_instances <= MAX_DEVICE_INSTANCES


def one_call_layout(n_vars_by_instance):
    """Word offsets of what tstwo_gkr_prove_batch leaves in its block (include/tstwo_hip.h; csrc/gkr_plan.h): a dict with `status`,
    `claims`, `outputs` (8 words per instance), `ood` (the final point), per layer `polys[L]` (20 words a round), `masks[L]` (16
    words per active instance, in instance order) and `active[L]` (those instances), and `words`, the block's size."""
    nv = list(n_vars_by_instance)
    n, n_layers = len(nv), max(nv)
    claims = 32 + 16 * n
    ood0 = claims + 16 * n
    off = ood0 + 12 * n_layers
    polys, masks, active = [], [], []
    for layer in range(n_layers):
        act = [i for i in range(n) if nv[i] >= n_layers - layer]
        polys.append(off)
        masks.append(off + 20 * layer)
        active.append(act)
        off += 20 * layer + 16 * len(act)
    return {"status": 16, "claims": claims, "outputs": claims + 8 * n, "ood": ood0 + 4 * n_layers * (n_layers & 1), "polys": polys,
            "masks": masks, "active": active, "words": off}


def _prove_batch_one_call(channel, layers_in):
    """prove_batch through tstwo_gkr_prove_batch: one library call, one read-back.  The refusals of the other two paths are raised
    here, before the call, with their exceptions."""
    n_inst = len(layers_in)
    if not device_rounds_supported(channel, n_inst):
        raise ValueError("one_call needs a Blake2sChannel with the Rust draw semantics and at most 64 instances")
    nv = [lay.n_variables() for lay in layers_in]
    if min(nv) == 0:
        raise ValueError("Some output claims were not set during proving (an input layer of 0 variables is an output layer)")
    for lay in layers_in:
        if lay.kind == LOGUP_MULTIPLICITIES and lay.n_variables() == 1:
            raise NotImplementedError("LogUpMultiplicities should never reach tryIntoMask")
    inst = (L.GkrInstance * n_inst)()
    for rec, lay in zip(inst, layers_in):
        rec.kind, rec.log_n = lay.kind, lay.n_variables()
        num = lay.num.ptr_list() if lay.num is not None else []
        rec.num = (L.vp * 4)(*(num + [None] * (4 - len(num))))
        rec.den = (L.vp * 4)(*lay.den.ptr_list())
    L.ensure_init()
    words = C.c_size_t(0)
    L.call("tstwo_gkr_prove_batch_words", inst, n_inst, C.byref(words))
    lay_out = one_call_layout(nv)
    assert words.value == lay_out["words"], "the block layout of include/tstwo_hip.h"
    block = np.zeros(words.value, dtype=np.uint32)
    digest = np.frombuffer(channel.digest(), dtype="<u4")
    chan = L.u32x(list(digest) + [channel.n_challenges, channel.n_sent])
    try:
        L.call("tstwo_gkr_prove_batch", chan, inst, n_inst, block.ctypes.data_as(L.u32p), words.value)
    except L.TstwoError as e:
        if str(e) == "sum-check: degenerate eq point":
            raise ZeroDivisionError("0 has no inverse") from None
        raise
    channel._digest = block[:8].astype("<u4").tobytes()
    channel.n_challenges, channel.n_sent = int(block[8]), int(block[9])
    n_cols = [1 if lay.kind == GRAND_PRODUCT else 2 for lay in layers_in]
    felts = lambda off, k: [_qs(block[off + 4 * j:off + 4 * j + 4]) for j in range(k)]          # noqa: E731
    n_layers = max(nv)
    masks = [[] for _ in range(n_inst)]
    sumcheck_proofs = []
    for layer in range(n_layers):
        polys = []
        for rnd in range(layer):
            p = lay_out["polys"][layer] + 20 * rnd
            polys.append(UnivariatePoly(felts(p + 4, int(block[p]))))
        sumcheck_proofs.append(SumcheckProof(polys))
        for j, i in enumerate(lay_out["active"][layer]):
            m = felts(lay_out["masks"][layer] + 16 * j, 4)
            masks[i].append(GkrMask([(m[0], m[1]), (m[2], m[3])][:n_cols[i]]))
    outputs = [felts(lay_out["outputs"] + 8 * i, n_cols[i]) for i in range(n_inst)]
    claims = [felts(lay_out["claims"] + 8 * i, n_cols[i]) for i in range(n_inst)]
    ood = felts(lay_out["ood"], n_layers)
    return GkrBatchProof(sumcheck_proofs, masks, outputs), GkrArtifact(ood, claims, nv)


def prove_batch(channel, input_layer_by_instance, device_rounds=None, one_call=False):
    """Batch-proves the instances' circuits (gkr_prover.ts proveBatch).  The input layers are left untouched; every layer the
    prover generates is freed once consumed.  Returns (GkrBatchProof, GkrArtifact).

    one_call: True = the whole proof in one library call (tstwo_gkr_prove_batch: the transcript stays on the device between the
    layers, one read-back at the end); ValueError where device_rounds_supported is false.  The same proof, artifact and channel
    state as the two paths below; device_rounds is then not looked at.

    device_rounds: True = the sum-check rounds run on the device (tstwo_gkr_round_finish: nothing is read back inside a layer;
    ValueError where that path cannot be taken); False = the host loop, one read-back per round; None = the device path where it
    can be taken (device_rounds_supported), else the host loop.  Both give the same proof, artifact and channel state."""
    layers_in = list(input_layer_by_instance)
    n_inst = len(layers_in)
    if n_inst == 0:
        raise ValueError("no instances")
    if one_call:
        return _prove_batch_one_call(channel, layers_in)
    if device_rounds is None:
        device_rounds = device_rounds_supported(channel, n_inst)
    elif device_rounds and not device_rounds_supported(channel, n_inst):
        raise ValueError("device_rounds needs a Blake2sChannel with the Rust draw semantics and at most 64 instances")
    n_layers_by = [lay.n_variables() for lay in layers_in]
    n_layers = max(n_layers_by)
    if min(n_layers_by) == 0:
        raise ValueError("Some output claims were not set during proving (an input layer of 0 variables is an output layer)")
    stacks = [_gen_layers(lay)[::-1] for lay in layers_in]         # [output, 1 variable, ..., input]

    # one read-back: every instance's output values and the mask of its first (constant-oracle) layer
    pieces, spans = [], []
    for st in stacks:
        a = _read_pairs(st[0], 1)
        b = _read_pairs(st[1], 2)
        spans.append((len(a), len(b)))
        pieces += a + b
    words = L.download_many(pieces)
    outputs, first_masks, k = [], [], 0
    for st, (na, nb) in zip(stacks, spans):
        outputs.append(_output_values(st[0], [w[0] for w in _unpack(st[0], words[k:k + na], 1)]))
        first_masks.append(_mask_of(st[1], [tuple(c) for c in _unpack(st[1], words[k + na:k + na + nb], 2)]))
        k += na + nb
    for st, lay_in in zip(stacks, layers_in):
        for lay in st[:2]:
            if lay is not lay_in:
                lay.free()
        del st[:2]

    slots = L.DeviceBuffer(32 * n_inst)
    dev = None                                # the device path's buffers, allocated at the first layer with rounds
    output_claims = [None] * n_inst
    masks = [[] for _ in range(n_inst)]
    sumcheck_proofs = []
    ood = []
    claims_to_verify = [None] * n_inst
    for layer in range(n_layers):
        rem_layers = n_layers - layer
        for i in range(n_inst):
            if n_layers_by[i] == rem_layers:
                claims_to_verify[i] = list(outputs[i])
                output_claims[i] = outputs[i]
        for c in claims_to_verify:
            if c is not None:
                channel.mix_felts(c)
        eq_evals = EqEvals.generate(ood) if layer > 0 else None
        alpha = channel.draw_felt()
        lam = channel.draw_felt()
        insts, new_masks = [], {}
        for i, c in enumerate(claims_to_verify):
            if c is None:
                continue
            if n_layers_by[i] == rem_layers:          # constant oracle: its mask was read up front
                new_masks[i] = first_masks[i]
                sc = None
            else:
                lay = stacks[i].pop(0)
                sc = _Instance(i, lay, lay is not layers_in[i], lam, len(insts))
            insts.append((i, sc, random_linear_combination(c, lam)))
        # batched sum-check (sumcheck.ts proveBatch) over the layer's oracles
        n_rounds = layer
        claims, n_v_of = {}, {}
        for i, sc, claim in insts:
            n_v_of[i] = layer - (n_layers - n_layers_by[i])
            claims[i] = claim.mulM31(M31(1 << (n_rounds - n_v_of[i])))
        reduced = [sc for _, sc, _ in insts if sc is not None]
        if device_rounds and n_rounds:
            # every round enqueued without a read-back; the layer's one read-back brings the channel, the round polynomials, the
            # assignment and the masks
            if dev is None:
                dev = _DeviceRounds(channel, n_inst, n_layers - 1)
            pieces = dev.run_layer(channel, insts, claims, n_v_of, eq_evals, alpha, n_rounds, slots)
            for sc in reduced:
                sc.apply_pending()
                pieces += _read_pairs(sc.layer, 2)
            words = L.download_many(pieces)
            round_polys, assignment = dev.unpack(words[0], n_rounds)
            words = words[1:]
        else:
            round_polys, assignment = _host_rounds(channel, insts, claims, eq_evals, alpha, n_rounds, slots)
            # masks of the reduced layers: one read-back for all of them
            pieces = []
            for sc in reduced:
                sc.apply_pending()
                pieces += _read_pairs(sc.layer, 2)
            words = L.download_many(pieces) if pieces else []
        sumcheck_proofs.append(SumcheckProof(round_polys))
        k = 0
        for sc in reduced:
            n_p = len(_read_pairs(sc.layer, 2))
            new_masks[sc.idx] = _mask_of(sc.layer, [tuple(c) for c in _unpack(sc.layer, words[k:k + n_p], 2)])
            k += n_p
            if sc.owned:
                sc.layer.free()
        if eq_evals is not None:
            eq_evals.free()
        for i, _, _ in insts:
            channel.mix_felts([v for col in new_masks[i].columns() for v in col])
            masks[i].append(new_masks[i])
        ch = channel.draw_felt()
        ood = list(assignment) + [ch]
        for i, _, _ in insts:
            claims_to_verify[i] = new_masks[i].reduce_at_point(ch)
    slots.free()
    if dev is not None:
        dev.free()
    proof = GkrBatchProof(sumcheck_proofs, masks, output_claims)
    return proof, GkrArtifact(ood, claims_to_verify, n_layers_by)


__all__ = ["GRAND_PRODUCT", "LOGUP_GENERIC", "LOGUP_MULTIPLICITIES", "LOGUP_SINGLES", "EqEvals", "GkrArtifact", "GkrBatchProof",
           "GkrInputClaimMismatch", "GkrMask", "GkrMultivariatePolyOracle", "HipGkrOps", "HipMleOps", "Layer", "Mle", "check_logup_sum",
           "correct_sum_as_poly_in_first_variable", "device_rounds_supported", "eval_mles_at_point", "fold_mle_evals", "inv_eq0_table",
           "logup_denominators", "logup_input_layer", "one_call_layout", "prove_batch", "round_finish", "verify_input_claims"]

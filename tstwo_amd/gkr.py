"""LogUp-GKR on the device: GkrOps / MleOps (backend/cpu/lookups/{gkr,mle}.ts), the prover's Layer / EqEvals /
GkrMultivariatePolyOracle (lookups/gkr_prover.ts) and prove_batch (gkr_prover.ts:440-580).

MLEs live in HBM: an Mle<SecureField> is a SecureColumnByCoords (4 SoA columns), an Mle<BaseField> one HipColumn; the first
variable is the most significant bit of the index.  Every pass over 2^n values is a kernel of csrc/gkr.hip; the host keeps the
O(rounds) protocol (sumcheck.py) and the channel.

prove_batch reads back at most one small buffer per sum-check round (the (f(0), f(2)) slots of every active instance, written
by one fused fold + sum launch each) and one per layer (the 2-point masks); the first read-back also takes every instance's
output values and first mask.
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

    def free(self) -> None:
        for c in ([self.col] if self.is_base else self.col.columns):
            c.buf.free()


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
    def fix_first_variable_into(mle: Mle, assignment: QM31, out: Mle) -> None:
        """The same into `out` (may be `mle` itself for a secure MLE: in place, the first half of its columns)."""
        if mle.is_base:
            L.call("tstwo_mle_fix_first_variable_base", C.c_void_p(mle.col.ptr), mle.n_variables(), _q(assignment), out.ptrs())
        else:
            L.call("tstwo_mle_fix_first_variable_secure", mle.ptrs(), mle.n_variables(), _q(assignment), out.ptrs())


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
        self.pending = None              # challenge not yet applied to the device layer

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


def prove_batch(channel, input_layer_by_instance):
    """Batch-proves the instances' circuits (gkr_prover.ts proveBatch).  The input layers are left untouched; every layer the
    prover generates is freed once consumed.  Returns (GkrBatchProof, GkrArtifact)."""
    layers_in = list(input_layer_by_instance)
    n_inst = len(layers_in)
    if n_inst == 0:
        raise ValueError("no instances")
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
    output_claims = [None] * n_inst
    masks = [[] for _ in range(n_inst)]
    sumcheck_proofs = []
    ood = []
    claims_to_verify = [None] * n_inst
    half = QM31.from_u32_unchecked(2, 0, 0, 0).inverse()
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
        claims = {}
        for i, sc, claim in insts:
            n_v = layer - (n_layers - n_layers_by[i])
            claims[i] = claim.mulM31(M31(1 << (n_rounds - n_v)))
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
        sumcheck_proofs.append(SumcheckProof(round_polys))
        # masks of the reduced layers: one read-back for all of them
        reduced = [sc for _, sc, _ in insts if sc is not None]
        for sc in reduced:
            sc.apply_pending()
        if reduced:
            pieces = []
            for sc in reduced:
                pieces += _read_pairs(sc.layer, 2)
            words = L.download_many(pieces)
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
    proof = GkrBatchProof(sumcheck_proofs, masks, output_claims)
    return proof, GkrArtifact(ood, claims_to_verify, n_layers_by)


__all__ = ["GRAND_PRODUCT", "LOGUP_GENERIC", "LOGUP_MULTIPLICITIES", "LOGUP_SINGLES", "EqEvals", "GkrArtifact", "GkrBatchProof",
           "GkrMask", "GkrMultivariatePolyOracle", "HipGkrOps", "HipMleOps", "Layer", "Mle", "correct_sum_as_poly_in_first_variable",
           "fold_mle_evals", "prove_batch"]

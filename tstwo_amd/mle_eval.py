"""The mle_eval component: an AIR statement that ties a claim on a LogUp-GKR input layer to committed columns (DESIGN §4.5;
Rust stwo has such a component as an example, the reference has none, so the construction is this project's own).

For public values, a point r in QM31^n, a claim v and a secure linear form L[p] = w_0 + sum_k w_k c_k[p] over base columns of
the main or the preprocessed tree, a component of log size n proves

    sum_p eq(p, r) L[p] = v,

where eq(p, r) is word p of gen_eq_evals(r, 1): r_0 belongs to the most significant bit of the storage position p, the
convention of gkr.eval_mles_at_point and gkr.logup_denominators, so the left side is Mle.evalAtPoint of the form.  Several
claims at one point are batched by the caller into one form with powers of a drawn gamma (batched_form); a LogUp denominator
claim is itself a form whose z sits in w_0, because the eq table sums to 1.

Storage position p holds the row with circle-domain index d = bit_reverse_index(p, n); with h = 2^(n-1) and d' = d mod h, a mask
offset of +2 moves d to d + 1 (mod h) in the first half (d < h) and to d - 1 (mod h) in the second, and bit j of d is variable
j of the eq table.  t(p) is the number of trailing one bits of d' (n - 1 when d' = h - 1): the step from d' to d' + 1 clears
bits 0 .. t-1 and sets bit t.

Preprocessed columns (mle_eval_selector_columns: 2n + 2 columns of 0 / 1 that depend on n only, tstwo_mle_eval_selectors):
    G_t[p] = [d < h and t(p) = t],  K_t[p] = [d >= h and t(p) = t]  (t < n),   F0[p] = [d = 0],   F1[p] = [d = h].
Interaction columns (secure, 4 base columns each): E at offsets [-2, 0, 2], S at offsets [-1, 0].
Constants (mle_eval_constants, host, from r): for t < n - 1, A_t = (1 - r_t) prod_{j<t} r_j and B_t = r_t prod_{j<t} (1 - r_j);
A_{n-1} = prod_{j<n-1} r_j and B_{n-1} = prod_{j<n-1} (1 - r_j); the anchors prod_j (1 - r_j) and r_{n-1} prod_{j<n-1} (1 - r_j).
Constraints (secure, degree 2):
    1. step     (sum_t G_t A_t) E[+2] + (sum_t K_t A_t) E[-2] - (sum_t (G_t + K_t) B_t) E[0] = 0
    2. anchors  F0 (E[0] - anchor_0) + F1 (E[0] - anchor_1) = 0
    3. sum      S[0] - S[-1] - E[0] L + v / 2^n = 0
1 and 2 determine E when no A_t is zero, so a point with a coordinate 0 or 1 is refused (ValueError).  S is the coset-order
running sum of E L - v / 2^n, what tstwo_logup_finalize_last writes: the last coset row holds 0, so S[-1] at the first row is 0.

The component declares E and S as interaction columns and adds no relation entry: it has no claimed_sum, and prove / verify do
not count v in their LogUp sum check.  v comes from the GKR artifact, never from the prover.
"""
from __future__ import annotations

from . import _lib as L
from .backend import HipColumn
from .circle import CanonicCoset
from .fields import M31, QM31
from .gkr import GkrInputClaimMismatch, HipGkrOps, Mle
from .logup import INTERACTION_TRACE_IDX, MAX_LOG, MAX_TERMS, LinearForm, logup_finalize_last
from .poly import HipCircleEvaluation

MIN_LOG = 2


def n_selector_columns(log_size: int) -> int:
    return 2 * log_size + 2


def _check_log(log_size: int) -> None:
    if not MIN_LOG <= log_size <= MAX_LOG:
        raise ValueError(f"log_size must be {MIN_LOG} to {MAX_LOG}")


def _check_point(point, log_size: int) -> list:
    point = list(point)
    if len(point) != log_size:
        raise ValueError(f"a point of {len(point)} coordinates for a component of log size {log_size}")
    zero, one = QM31.zero().tup(), QM31.one().tup()
    for j, r in enumerate(point):
        if r.tup() in (zero, one):
            raise ValueError(f"coordinate {j} of the point is {r.tup()[0]}: the step constraint does not determine the eq table there")
    return point


def mle_eval_selector_columns(log_size: int) -> list:
    """The 2 log_size + 2 preprocessed columns G_0 .. G_{n-1}, K_0 .. K_{n-1}, F0, F1 as HipColumns of 2^log_size words
    (tstwo_mle_eval_selectors: one launch, asynchronous)."""
    _check_log(log_size)
    out = [HipColumn.uninitialized(1 << log_size) for _ in range(n_selector_columns(log_size))]
    L.call("tstwo_mle_eval_selectors", log_size, L.ptr_array([c.ptr for c in out]))
    return out


def mle_eval_constants(point):
    """(A, B, anchor_0, anchor_1) of the module docstring, QM31 values computed on the host from the point."""
    point = list(point)
    n, one = len(point), QM31.one()
    if n < 1:
        raise ValueError("a point of at least one coordinate")
    a, b = [], []
    pr, pn = one, one                  # prod_{j<t} r_j, prod_{j<t} (1 - r_j)
    for t in range(n - 1):
        a.append(one.sub(point[t]).mul(pr))
        b.append(point[t].mul(pn))
        pr, pn = pr.mul(point[t]), pn.mul(one.sub(point[t]))
    a.append(pr)
    b.append(pn)
    return a, b, pn.mul(one.sub(point[n - 1])), pn.mul(point[n - 1])


class MleEvalForm:
    """The secure linear form of the statement as the constraints see it: constant + sum weight_k * column_k, a column being
    ("main", i), the component's i-th main column, or ("pre", i), the i-th preprocessed column the component names after its
    2 log_size + 2 selectors.  n_main: the main columns of the component (all are read in order, used or not; by default the
    highest index used + 1)."""

    def __init__(self, terms, constant: QM31 | None = None, n_main: int | None = None):
        self.terms = [(w, (str(kind), int(i))) for w, (kind, i) in terms]
        if any(kind not in ("main", "pre") or i < 0 for _, (kind, i) in self.terms):
            raise ValueError('a form column is ("main", i) or ("pre", i)')
        self.constant = QM31.zero() if constant is None else constant
        used = [i for _, (kind, i) in self.terms if kind == "main"]
        self.n_main = max(used, default=-1) + 1 if n_main is None else int(n_main)
        if used and max(used) >= self.n_main:
            raise ValueError("a term names a main column beyond n_main")

    def n_pre(self) -> int:
        return max((i for _, (kind, i) in self.terms if kind == "pre"), default=-1) + 1

    def on_columns(self, main=(), pre=()) -> LinearForm:
        """The same form over whole device columns (logup.LinearForm), for mle_eval_interaction_trace: main[i] / pre[i] are the
        HipColumns the references name."""
        src = {"main": list(main), "pre": list(pre)}
        return LinearForm([(w, src[kind][i]) for w, (kind, i) in self.terms], self.constant)


def batched_form(claims, forms, gamma: QM31):
    """(form, claim) of sum_i gamma^i (form_i = claim_i): MleEvalForms at one point batched into one."""
    claims, forms = list(claims), list(forms)
    if not forms or len(claims) != len(forms):
        raise ValueError("one claim per form, at least one")
    power, total, constant, terms = QM31.one(), QM31.zero(), QM31.zero(), {}
    for v, f in zip(claims, forms):
        total = total.add(power.mul(v))
        constant = constant.add(power.mul(f.constant))
        for w, ref in f.terms:
            terms[ref] = terms.get(ref, QM31.zero()).add(power.mul(w))
        power = power.mul(gamma)
    return MleEvalForm([(w, ref) for ref, w in terms.items()], constant, max(f.n_main for f in forms)), total


class MleEvalEval:
    """The constraint-framework eval of the statement (module docstring) for FrameworkComponent: interpreted by default, and
    it also runs as a FrameworkComponent(native=True).  The component's preprocessed columns are the 2 log_size + 2 selectors in
    the order of mle_eval_selector_columns, then the form's preprocessed columns."""

    def __init__(self, log_size: int, point, claim: QM31, form: MleEvalForm):
        _check_log(log_size)
        self.log_n_rows = log_size
        self.point = _check_point(point, log_size)
        self.claim, self.form = claim, form
        self.a, self.b, self.anchor0, self.anchor1 = mle_eval_constants(self.point)
        self.shift = claim.mulM31(M31(1 << log_size).inverse())          # v / 2^n

    def log_size(self) -> int:
        return self.log_n_rows

    def max_constraint_log_degree_bound(self) -> int:
        return self.log_n_rows + 1

    def n_preprocessed(self) -> int:
        return n_selector_columns(self.log_n_rows) + self.form.n_pre()

    def evaluate(self, eval):
        n, sec = self.log_n_rows, eval._secure
        g = [eval.get_preprocessed_column(t) for t in range(n)]
        k = [eval.get_preprocessed_column(n + t) for t in range(n)]
        f0, f1 = eval.get_preprocessed_column(2 * n), eval.get_preprocessed_column(2 * n + 1)
        main = [eval.next_trace_mask() for _ in range(self.form.n_main)]
        pre = [eval.get_preprocessed_column(2 * n + 2 + i) for i in range(self.form.n_pre())]
        e_prev, e, e_next = eval.next_extension_interaction_mask(INTERACTION_TRACE_IDX, [-2, 0, 2])
        s_prev, s = eval.next_extension_interaction_mask(INTERACTION_TRACE_IDX, [-1, 0])
        # (a secure value stands on the left of every product: a base value does not know how to multiply one.  Every sum is a
        # chain over column loads alone, G_t + K_t is never formed: a shared sum per t would stay live across the 4 coordinates
        # and cost the program a register per t)
        a_next = a_prev = b_here = sec(0)
        for t in range(n):
            a_next = a_next + sec(self.a[t]) * g[t]
        for t in range(n):
            a_prev = a_prev + sec(self.a[t]) * k[t]
        for t in range(n):
            b_here = b_here + sec(self.b[t]) * g[t]
        for t in range(n):
            b_here = b_here + sec(self.b[t]) * k[t]
        eval.add_constraint(a_next * e_next + a_prev * e_prev - b_here * e)
        eval.add_constraint((e - self.anchor0) * f0 + (e - self.anchor1) * f1)
        form = sec(self.form.constant)
        for w, (kind, i) in self.form.terms:
            form = form + sec(w) * (main[i] if kind == "main" else pre[i])
        eval.add_constraint(s - s_prev - e * form + self.shift)
        return eval

    logSize = log_size
    maxConstraintLogDegreeBound = max_constraint_log_degree_bound


def mle_eval_terms(eq, form: LinearForm, out=None):
    """tstwo_mle_eval_terms: out[p] = eq[p] * form[p] over a secure Mle / SecureColumnByCoords `eq`; out defaults to eq itself
    (in place).  Asynchronous; returns out."""
    eq = eq.col if isinstance(eq, Mle) else eq
    out = eq if out is None else (out.col if isinstance(out, Mle) else out)
    n = eq.len()
    if not 1 <= len(form.terms) <= MAX_TERMS:
        raise ValueError(f"a form needs 1 to {MAX_TERMS} column terms")
    if out.len() != n or any(col.len() != n for _, col in form.terms):
        raise ValueError("the columns of the form, eq and out must have one length")
    L.call("tstwo_mle_eval_terms", eq.ptrs(), L.ptr_array([col.ptr for _, col in form.terms]),
           L.u32x([w for p, _ in form.terms for w in p.tup()]), len(form.terms), L.u32x(form.constant.tup()), n.bit_length() - 1,
           out.ptrs())
    return out


def mle_eval_interaction_trace(point, claim: QM31, form: LinearForm, instance: int = 0):
    """The interaction trace of MleEvalEval on the device: 8 HipCircleEvaluations on CanonicCoset(n).circle_domain(), the 4
    coordinate columns of E = gen_eq_evals(point, 1), then those of S.  form: the statement's form over whole device columns
    (MleEvalForm.on_columns, or a logup.LinearForm of HipColumns).  Three steps, nothing read back but the sum:
    tstwo_gkr_gen_eq_evals, tstwo_mle_eval_terms, tstwo_logup_finalize_last.  Raises GkrInputClaimMismatch(instance, 0) when
    the sum is not `claim`: such a trace cannot satisfy constraint 3."""
    point = _check_point(point, len(list(point)))
    log_size = len(point)
    _check_log(log_size)
    e = HipGkrOps.genEqEvals(point, QM31.one())
    s = Mle.uninitialized_secure(1 << log_size)
    mle_eval_terms(e, form, s)
    total = logup_finalize_last(s.col, log_size)
    if total.tup() != claim.tup():
        raise GkrInputClaimMismatch(instance, 0)
    domain = CanonicCoset(log_size).circleDomain()
    return [HipCircleEvaluation(domain, c) for c in e.col.columns + s.col.columns]


__all__ = ["MIN_LOG", "MleEvalEval", "MleEvalForm", "batched_form", "mle_eval_constants", "mle_eval_interaction_trace",
           "mle_eval_selector_columns", "mle_eval_terms", "n_selector_columns"]

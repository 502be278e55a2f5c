"""Messages that steer the operands of Hades round 0 to the edges of the felt252 arithmetic (plain integers: no GPU, no library).

The kernels keep the state in Montgomery form: rep(v) = v R mod p with R = 2^256.  After an absorb of (x, y) onto a state
(p0, p1, p2) and the round-0 constants, the words that enter the S-box are

    pre0 = rep(p0 + x + ARK[0][0])      pre1 = rep(p1 + y + ARK[0][1])      pre2 = rep(p2 + ARK[0][2])

and the two operands of each round-constant add are rep(p_i + x_i) and rep(ARK[0][i]).  Cubing is a bijection of the field
(gcd(3, p - 1) = 1, asserted below), so the caller can also choose the words A = rep(pre0^3), B = rep(pre1^3) that leave it, and
with c = rep(pre2^3) known, every operand of the MDS step t = (A + B) + c, t + 2A, t - 2B, t - 3c.

A Case holds a message (or, for a channel draw, a digest and n_sent), the knob it uses and the raw values it claims; CASES is the
list.  tests/test_cpu_poseidon_steer.py recomputes every claim forwards from poseidon_model arithmetic, proves on the two limb
models that the cases reach the carry, borrow and digit situations they are built for, and tests/test_gpu_poseidon_steer.py
sends them to the device.

Claim keys, all raw integers of the steered permutation's round 0:
  sum0, sum1    rep(p_i + x_i) + rep(ARK[0][i]) before the reduction
  pre0, pre1    the words that enter cube
  post0, post1  A and B
  ab            A + B before the reduction
  abc           ((A + B) mod p) + c before the reduction
  2A            A + A before the reduction
  t-2B, t-3c    t - (2B mod p) and t - (3c mod p) as integers: 0 a zero result, -1 a borrow through every limb
"""
from __future__ import annotations

import math
import random

import poseidon_model as M

P = M.P
R = 2**256
R_MOD = R % P
R_INV = pow(R, -1, P)
M32 = 2**32 - 1
assert math.gcd(3, P - 1) == 1
CBRT_EXP = pow(3, -1, P - 1)
S0_KEYS = ("sum0", "pre0", "post0", "2A")          # what a message's first element alone decides


def rep(v):
    return v * R % P


def unrep(t):
    return t * R_INV % P


def cbrt(v):
    return pow(v, CBRT_EXP, P)


def from_limbs(ls):
    return sum(v << (32 * j) for j, v in enumerate(ls))


class Case:
    """name; kind "msg" (msg: the elements; the steered absorb is number `perm`) or "draw" (digest, n_sent); knob; claims;
    x_only: the case still says something about s0 as a one-element message; group_local: it relies on a carry staying inside
    its 8-lane group, and `neighbour` names the case to place in the groups beside it."""

    def __init__(self, name, kind, knob, claims, msg=None, digest=None, n_sent=None, perm=0, x_only=False, group_local=False,
                 neighbour=None):
        self.name, self.kind, self.knob, self.claims = name, kind, knob, dict(claims)
        self.msg, self.digest, self.n_sent, self.perm = msg, digest, n_sent, perm
        self.x_only, self.group_local, self.neighbour = x_only, group_local, neighbour
        for v in (msg if kind == "msg" else [digest]):
            assert 0 <= v < P, name                              # canonical
        assert kind == "msg" or 0 <= n_sent < 2**32 - 1          # 2^32 - 1 wraps in the kernel's word, not in the model

    @property
    def xy(self):
        """the pair a two-element entry (hash_many at k = 2, a node's children, digest and root) takes"""
        return (self.msg[0], self.msg[1]) if self.kind == "msg" else (self.digest, self.n_sent)

    def __repr__(self):
        return f"Case({self.name})"


_rng = random.Random(0x5EED252)


def _rand():
    return _rng.randrange(P)


# ---------------------------------------------------------------- targets
def pre_targets():
    """(name, word entering cube): the limb patterns of tests/test_cpu_felt_coop.py that matter to a square and a product"""
    out = [("zero", 0), ("one", 1), ("p-1", P - 1), ("p-2", P - 2), ("R", R_MOD)]
    out += [("limb0_is_1", _rand() & ~M32 | 1), ("limb0_ones", _rand() & ~M32 | M32)]
    for i in range(8):                                          # limb 0 zero: digit 0 at step 0
        out.append((f"limb{i}_zero", _rand() & ~(M32 << (32 * i))))
    for top in (0, 1, 2**27 - 1):
        out.append((f"low7_ones_top{top}", top << 224 | (2**224 - 1)))
    out += [("2^251+2^192-1", 2**251 + 2**192 - 1), ("2^251+16*2^192+ones", 2**251 + 16 * 2**192 + (2**192 - 1))]
    for _, t in out:
        assert t < P
    return out


def ripple_operand(k, upto):
    """a canonical word whose raw sum with k generates a carry in limb 0 that limbs 1..upto pass on (each is all ones before
    the carry arrives) and limb upto + 1 takes"""
    kl = [(k >> (32 * j)) & M32 for j in range(8)]
    assert kl[0] != 0
    xl = [(2**32 - kl[0]) & M32] + [M32 - kl[j] for j in range(1, upto + 1)] + [0] * (7 - upto)
    return from_limbs(xl)


def post_targets(c, b_fixed):
    """(name, A, B, claims, group_local, neighbour) for the words that leave the S-box; B is b_fixed where the caller cannot
    choose it.  c = rep(pre2^3)."""
    c3 = 3 * c % P
    out = []

    def b_or(v):
        return b_fixed if b_fixed is not None else v

    for name, s in (("ab_is_p", P), ("ab_is_p-1", P - 1), ("ab_is_p+1", P + 1)):
        b = b_or(_rand())
        out.append((name, s - b, b, {"ab": s}, s == P, "ab_is_p+1" if s == P else None))
    b = b_or(_rand())
    out.append(("abc_is_p", (P - c - b) % P, b, {"abc": P}, True, "ab_is_p+1"))
    for name, a in (("dblA_is_p-1", (P - 1) // 2), ("dblA_is_p+1", (P + 1) // 2)):
        out.append((name, a, b_or(_rand()), {"2A": 2 * a}, False, None))
    for d in (-1, 0, 1):
        b = b_or(_rand())
        while b_fixed is None and not 0 <= 2 * b % P + d < P:
            b = _rand()
        assert 0 <= 2 * b % P + d < P
        out.append((f"t_is_2B{d:+d}", (2 * b % P + d - b - c) % P, b, {"t-2B": d}, d <= 0, "t_is_2B+1" if d <= 0 else None))
    for d in (-1, 0, 1):
        assert 0 <= c3 + d < P
        b = b_or(_rand())
        out.append((f"t_is_3c{d:+d}", (c3 + d - c - b) % P, b, {"t-3c": d}, d <= 0, "t_is_3c+1" if d <= 0 else None))
    out.append(("A0_Bmax", 0, b_or(P - 1), {}, False, None))
    if b_fixed is None:                                         # both doublings, and A + B raw p on top
        out.append(("dblA_dblB", (P - 1) // 2, (P + 1) // 2, {"2A": P - 1, "ab": P}, True, "ab_is_p+1"))
        # t = c and 2B - 1 = c: the all-borrow sub behind a raw sum of exactly p
        b = (c + 1) * pow(2, -1, P) % P
        out.append(("ab_is_p_t_is_2B-1", P - b, b, {"ab": P, "t-2B": -1}, True, "t_is_2B+1"))
    for _, a, b, *_ in out:
        assert 0 <= a < P and 0 <= b < P
    return out


# ---------------------------------------------------------------- one absorb, solved backwards
def _x_for_pre(t, prev, ark):
    return (unrep(t) - ark - prev) % P


def _x_for_post(a, prev, ark):
    return (cbrt(unrep(a)) - ark - prev) % P


def _x_for_sum(s, prev, ark):
    """rep(prev + x) + rep(ark) = s as integers"""
    w = s - rep(ark)
    assert 0 <= w < P
    return (unrep(w) - prev) % P


def _c_of(state):
    return rep(pow((state[2] + M.ARK[0][2]) % P, 3, P))


def _post1_of(state, y):
    return rep(pow((state[1] + y + M.ARK[0][1]) % P, 3, P))


def absorb_cases(prefix, state, y_fixed, select):
    """[(name, x, y, knob, claims, x_only, group_local, neighbour)] for one absorb onto `state` (integers, not Montgomery);
    y_fixed: the second element where the caller cannot choose it.  select: which of the knobs "pre", "sum", "post"."""
    a0, a1, _ = M.ARK[0]
    out = []
    yf = y_fixed
    if "pre" in select:
        tg = pre_targets()
        for i, (name, t0) in enumerate(tg):
            _, t1 = tg[(i + 7) % len(tg)]
            claims = {"pre0": t0}
            if yf is None:
                claims["pre1"] = t1
            out.append((f"{prefix}pre_{name}", _x_for_pre(t0, state[0], a0), yf if yf is not None else _x_for_pre(t1, state[1], a1),
                        "pre-cube", claims, True, False, None))
    if "sum" in select:
        k0, k1 = rep(a0), rep(a1)
        sums = [("sum_is_p", P, P + 1, True), ("sum_is_p-1", P - 1, P, False), ("sum_is_p+1", P + 1, P - 1, False),
                ("sum_ripple_to_6", ripple_operand(k0, 5) + k0, ripple_operand(k1, 6) + k1, True),
                ("sum_ripple_to_7", ripple_operand(k0, 6) + k0, ripple_operand(k1, 5) + k1, True),
                ("sum_borrow_1_5", P - 1 + 2**192, P - 1 + 3 * 2**192, False)]
        for name, s0, s1, gl in sums:
            claims = {"sum0": s0}
            if yf is None:
                claims["sum1"] = s1
            out.append((f"{prefix}{name}", _x_for_sum(s0, state[0], a0), yf if yf is not None else _x_for_sum(s1, state[1], a1),
                        "round-0 add", claims, True, gl, None if name == "sum_is_p+1" else f"{prefix}sum_is_p+1"))
    if "post" in select:
        c = _c_of(state)
        bf = None if yf is None else _post1_of(state, yf)
        for name, a, b, claims, gl, nb in post_targets(c, bf):
            claims = dict(claims, post0=a, post1=b)
            out.append((f"{prefix}post_{name}", _x_for_post(a, state[0], a0), yf if yf is not None else _x_for_post(b, state[1], a1),
                        "post-cube", claims, yf == 1, gl, None if nb is None else f"{prefix}post_{nb}"))
    return out


PRE_SUBSET = ("zero", "p-1", "limb0_is_1", "limb0_ones", "limb0_zero", "limb4_zero", "low7_ones_top134217727", "2^251+2^192-1")


def build_cases():
    cases = []
    # first absorb, both elements free: k = 2 (and the x-only ones at k = 1)
    for name, x, y, knob, claims, xo, gl, nb in absorb_cases("", [0, 0, 0], None, ("pre", "sum", "post")):
        cases.append(Case(name, "msg", knob, claims, msg=[x, y], x_only=xo, group_local=gl, neighbour=nb))
    # one-element messages: the second element is the sponge's appended 1, so B is fixed
    for name, x, y, knob, claims, xo, gl, nb in absorb_cases("k1_", [0, 0, 0], 1, ("post",)):
        cases.append(Case(name, "msg", knob, claims, msg=[x, y], x_only=True, group_local=gl, neighbour=nb))
    # later absorb: the second permutation of a 3-element (x free, y the appended 1) and a 4-element message
    for k in (3, 4):
        head = [_rand(), _rand()]
        state = M.hades([head[0], head[1], 0])
        for name, x, y, knob, claims, xo, gl, nb in absorb_cases(f"k{k}_", state, 1 if k == 3 else None, ("pre", "sum", "post")):
            if knob == "pre-cube" and name.split("pre_")[1] not in PRE_SUBSET:
                continue                                        # a subset of the limb patterns is enough the second time
            cases.append(Case(name, "msg", "later absorb", claims, msg=head + ([x] if k == 3 else [x, y]), perm=1, group_local=gl,
                              neighbour=nb))
    # channel draw: Hades(digest, n_sent, 2) with no sponge add; only the digest is free
    for n_sent in (0, 1, 2**32 - 2):
        sel = ("pre", "sum", "post") if n_sent == 1 else ("sum", "post")
        for name, x, y, knob, claims, xo, gl, nb in absorb_cases(f"draw{n_sent}_", [0, 0, 2], n_sent, sel):
            if knob == "pre-cube" and name.split("pre_")[1] not in PRE_SUBSET:
                continue
            cases.append(Case(name, "draw", "channel draw", claims, digest=x, n_sent=n_sent, group_local=gl, neighbour=nb))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert c.neighbour is None or c.neighbour in names, (c.name, c.neighbour)
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}

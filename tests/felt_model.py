"""The lane-per-hash arithmetic of csrc/felt252.cuh on Python integers, limb by limb: one variable per 32-bit limb, carry and
borrow chains written out as the header writes them, every accumulator's width checked at every step and every result checked
against Python's own arithmetic.  It shares no code with the library or with felt_coop_model.py (the 8-lane form).

Two things are optional and change nothing when unused.  EVENTS, when set to a collections.Counter, counts the named operand
situations below as they occur, so a test can prove that its inputs reach them.  `rounds` limits hades_mont to the first rounds
of the permutation, so an absorb plus round 0 runs in milliseconds.  check() is the one place a condition is asserted: a test
that deliberately breaks a line of this model replaces it to see the wrong value instead of the assertion.

Events:
  reduce.eq_p             reduce_once of exactly p (the result is 0)
  reduce.eq_p_minus_1     reduce_once of p - 1 (the largest operand that stays)
  reduce.ge_p_borrow_1_5  operand >= p whose subtraction borrows out of limb 0 and through limbs 1-5
  add.carry_into_7        the carry chain of add reaches limb 7
  sub.addback_ripple      a < b, and the carry of the add-back leaves limb 0 and ripples through limbs 1-5
  sub.zero                a == b
  mul.digit_0             a Montgomery digit of 0 (the cc = 0 branch)
  mul.digit_max           a Montgomery digit of 2^32 - 1
  mul.r6_hi               r6 >> 32 nonzero
  mul.r7_hi               r7 >> 32 nonzero
  mul.t8_nonzero          t[8] nonzero before the shift
  mul.r8_hi               r8 >> 32 nonzero: IMPOSSIBLE, see below

mul.r8_hi cannot occur.  Before a step the accumulator is T < 2p.  The step forms (T + a b_i + m p) / 2^32 with a < p and
b_i, m <= 2^32 - 1, so the new T < (2p + (2^32 - 1) p + (2^32 - 1) p) / 2^32 = 2p < 2^253.  r8 is limbs 7 and 8 of the new T
(T >> 224), so r8 < 2^29 and r8 >> 32 = 0: the new t[8] is always 0.  The model counts the event all the same, and
tests/test_cpu_poseidon_steer.py asserts the count stays 0 over its whole case set.
"""
from __future__ import annotations

import hashlib

P = 2**251 + 17 * 2**192 + 1
W = 2**32
M32 = W - 1
R = 2**256
R_INV = pow(R, -1, P)
ARK = [[int.from_bytes(hashlib.sha256(f"Hades{3 * i + j}".encode()).digest(), "big") % P for j in range(3)] for i in range(91)]
EVENT_NAMES = ("reduce.eq_p", "reduce.eq_p_minus_1", "reduce.ge_p_borrow_1_5", "add.carry_into_7", "sub.addback_ripple", "sub.zero",
               "mul.digit_0", "mul.digit_max", "mul.r6_hi", "mul.r7_hi", "mul.t8_nonzero")
IMPOSSIBLE_EVENTS = ("mul.r8_hi",)

EVENTS = None                   # a collections.Counter while a test records


def _ev(name):
    if EVENTS is not None:
        EVENTS[name] += 1


def check(cond, *info):
    assert cond, info


def limbs(x):
    check(0 <= x < R)
    return [(x >> (32 * j)) & M32 for j in range(8)]


def value(ls):
    return sum(v << (32 * j) for j, v in enumerate(ls))


P_L = limbs(P)
R2_L = limbs(R * R % P)
ONE_L = limbs(R % P)


def addc(a, b, c):
    """__builtin_addc on 32-bit words: (sum word, carry out)"""
    s = a + b + c
    return s & M32, s >> 32


def subc(a, b, bw):
    """__builtin_subc on 32-bit words: (difference word, borrow out)"""
    d = a - b - bw
    return d & M32, 1 if d < 0 else 0


def reduce_once(t):
    vt = value(t)
    check(vt < 2 * P)
    d, b, chain = [0] * 8, 0, []
    for k in range(8):
        d[k], b = subc(t[k], P_L[k], b)
        chain.append(b)
    keep = b != 0                                          # the last borrow: t < p
    r = list(t) if keep else d
    if vt == P:
        _ev("reduce.eq_p")
    if vt == P - 1:
        _ev("reduce.eq_p_minus_1")
    if not b and all(chain[:6]):
        _ev("reduce.ge_p_borrow_1_5")
    check(value(r) == vt % P, t, r)
    return r


def add(a, b):
    s, c = [0] * 8, 0
    for k in range(8):
        s[k], c = addc(a[k], b[k], c)
        if k == 6 and c:
            _ev("add.carry_into_7")
    check(c == 0)                                          # a + b < 2p < 2^256
    r = reduce_once(s)
    check(value(r) == (value(a) + value(b)) % P)
    return r


def dbl(a):
    return add(a, a)


def sub(a, b):
    d, bw = [0] * 8, 0
    for k in range(8):
        d[k], bw = subc(a[k], b[k], bw)
    m = (0 - bw) & M32
    r, c, chain = [0] * 8, 0, []
    for k in range(8):
        r[k], c = addc(d[k], P_L[k] & m, c)
        chain.append(c)
    if bw and all(chain[:6]):
        _ev("sub.addback_ripple")
    if not any(r):
        _ev("sub.zero")
    check(c == bw)                                         # the add-back carries out exactly when it was needed
    check(value(r) == (value(a) - value(b)) % P, a, b, r)
    return r


def mul(a, b):
    va, vb = value(a), value(b)
    check(va < P and vb < P)
    t = [0] * 9
    t_ref = 0
    for i in range(8):
        c = 0
        for j in range(8):
            r = a[j] * b[i] + t[j] + c
            check(r < 2**64)
            t[j] = r & M32
            c = r >> 32
        check(t[8] + c < W)                                # t[8] += (uint32_t)c does not wrap
        t[8] += c
        if t[8]:
            _ev("mul.t8_nonzero")
        m = (0 - t[0]) & M32
        if m == 0:
            _ev("mul.digit_0")
        if m == M32:
            _ev("mul.digit_max")
        cc = 1 if t[0] != 0 else 0
        for j in range(1, 6):
            t[j - 1], cc = addc(t[j], 0, cc)
        r6 = m * 17 + t[6] + cc
        check(r6 < 2**64)
        t[5] = r6 & M32
        if r6 >> 32:
            _ev("mul.r6_hi")
        r7 = (m << 27) + t[7] + (r6 >> 32)
        check(r7 < 2**64)
        t[6] = r7 & M32
        if r7 >> 32:
            _ev("mul.r7_hi")
        r8 = t[8] + (r7 >> 32)
        t[7] = r8 & M32
        t[8] = (r8 >> 32) & M32
        if r8 >> 32:
            _ev("mul.r8_hi")
        # the accumulator is what CIOS says it is, and below 2p
        t_ref = t_ref + va * b[i] + m * P
        check(t_ref % W == 0)
        t_ref //= W
        check(value(t) == t_ref and t_ref < 2 * P, i)
    r = reduce_once(t[:8])
    check(value(r) == va * vb * R_INV % P)
    return r


def cube(x):
    return mul(mul(x, x), x)


def to_mont(x):
    return mul(x, R2_L)


def from_mont(x):
    return mul(x, limbs(1))


def hades_mont(s0, s1, s2, rounds=91):
    """felt::hades on a Montgomery-form state of three limb lists; `rounds` < 91 stops after that many rounds."""
    for r in range(rounds):
        s0 = add(s0, limbs(ARK[r][0] * R % P))
        s1 = add(s1, limbs(ARK[r][1] * R % P))
        s2 = add(s2, limbs(ARK[r][2] * R % P))
        if r < 4 or r >= 87:
            s0, s1 = cube(s0), cube(s1)
        s2 = cube(s2)
        t = add(add(s0, s1), s2)
        s0, s1, s2 = add(t, dbl(s0)), sub(t, dbl(s1)), sub(t, add(dbl(s2), s2))
    return s0, s1, s2


def hades(state, rounds=91):
    """state: three canonical integers.  The permutation through the limb arithmetic, Montgomery form inside."""
    s = hades_mont(*(to_mont(limbs(x)) for x in state), rounds=rounds)
    return [value(from_mont(x)) for x in s]

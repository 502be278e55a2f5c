"""The lane algorithm of csrc/felt252_coop.cuh on Python integers: one element over 8 lanes, lane j holding limb j, one variable
per lane accumulator, and every accumulator's width asserted at every step.  It shares no code with the library; the arithmetic it
is checked against is Python's own (a * b * R^-1 mod p).

A "group" below is a list of 8 lane values.  resolve() is written for a whole wave (8 groups, 64 lanes, two 64-bit masks) because
that is where it can go wrong: a carry must not leave a group for its neighbour.

Two things are optional and change nothing when unused.  EVENTS, when set to a collections.Counter, counts the named operand
situations below as they occur, so a test can prove that its inputs reach them.  `rounds` limits hades_mont to the first rounds
of the permutation.  check() is the one place a condition is asserted: a test that deliberately breaks a line of this model
replaces it to see the wrong value instead of the assertion.

Events (resolve's are counted on the group in slot 3 of the wave, where resolve() puts its operand):
  resolve.chain6          a generating lane followed by exactly 6 lanes that propagate its carry
  resolve.chain7          the same with 7 lanes: lane 0 generates, lanes 1-7 propagate
  resolve.top_propagated  the carry out of limb 7 comes through a propagating lane 7
  sub.all_ones            the difference before the add-back is the all-ones word (a = b - 1)
  mul.h6_ge_2_27          H_6 at or above 2^27
  mul.m_carry             the (m != 0) carry into lane 0 taken
  mul.m_no_carry          ... and not taken (digit 0)
  mul.final_carry         a carry in the final L + from_lower(H)
"""
from __future__ import annotations

import hashlib

P = 2**251 + 17 * 2**192 + 1
W = 2**32
M32 = W - 1
R = 2**256
R_INV = pow(R, -1, P)
LOW7 = 0x7F7F7F7F7F7F7F7F
M64 = 2**64 - 1
EVENT_NAMES = ("resolve.chain6", "resolve.chain7", "resolve.top_propagated", "sub.all_ones", "mul.h6_ge_2_27", "mul.m_carry",
               "mul.m_no_carry", "mul.final_carry")
IMPOSSIBLE_EVENTS = ()
ARK = [[int.from_bytes(hashlib.sha256(f"Hades{3 * i + j}".encode()).digest(), "big") % P for j in range(3)] for i in range(91)]


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
NEGP_L = limbs(R - P)
Q_L = [0, 0, 0, 0, 0, 17, 1 << 27, 0]           # what lane j adds of m p after the shift: 17 m (limb 6 -> 5), 2^27 m (limb 7 -> 6)


def from_upper(g):
    return [g[j + 1] if j < 7 else 0 for j in range(8)]


def from_lower(g):
    return [g[j - 1] if j else 0 for j in range(8)]


def resolve_wave(u):
    """u: 64 lane values < 2^33.  Returns (64 resolved low words, 64 top flags): the kernel's carry-lookahead on the two masks."""
    check(len(u) == 64)
    G = Pm = 0
    for lane, x in enumerate(u):
        check(0 <= x < 2**33, (lane, x))
        G |= (x >> 32 != 0) << lane
        Pm |= ((x & M32) == M32) << lane
    a, b = (G | Pm) & LOW7, G & LOW7
    s = a + b
    check(s <= M64)                               # bits 8k + 7 of a and b are 0: the top bit of the sum never carries out
    C = s ^ a ^ b
    T = (G | (Pm & C)) & ~LOW7 & M64
    out = [((x & M32) + ((C >> lane) & 1)) & M32 for lane, x in enumerate(u)]
    top = [(T >> (lane | 7)) & 1 for lane in range(64)]
    if EVENTS is not None:
        _resolve_events(u[24:32])
    return out, top


def _resolve_events(g):
    """the group in slot 3 on its own: the longest run of lanes that pass a generated carry on, and how limb 7 carries out"""
    carry = run = best = 0
    for j in range(8):
        lo = g[j] & M32
        passes = carry and lo == M32 and g[j] >> 32 == 0
        run = run + 1 if passes else 0
        best = max(best, run)
        if j == 7 and passes:
            _ev("resolve.top_propagated")
        carry = (g[j] + carry) >> 32
    if best in (6, 7):
        _ev(f"resolve.chain{best}")


def resolve(g, others=None):
    """One group (8 lane values); `others`: what the 7 other groups of the wave hold (default: copies).  The group sits in slot 3."""
    wave = []
    for k in range(8):
        wave += list(g) if k == 3 or others is None else list(others[k if k < 3 else k - 1])
    out, top = resolve_wave(wave)
    res, t = out[24:32], top[24:32]
    check(len(set(t)) == 1)
    # what it must be: the value mod 2^256 and the carry out of bit 256
    v = value(g)
    check(value(res) == v % R and t[0] == v >> 256, (g, res, t))
    return res, t[0]


def reduce_once(t, others=None):
    check(value(t) < 2 * P)
    d, ge = resolve([t[j] + NEGP_L[j] for j in range(8)], others)
    return d if ge else list(t)


def add(a, b, others=None):
    s, top = resolve([a[j] + b[j] for j in range(8)], others)
    check(top == 0)
    return reduce_once(s, others)


def dbl(a):
    return add(a, a)


def sub(a, b, others=None):
    d, no_borrow = resolve([a[j] + (~b[j] & M32) + (1 if j == 0 else 0) for j in range(8)], others)
    if d == [M32] * 8:
        _ev("sub.all_ones")
    r, _ = resolve([d[j] + (0 if no_borrow else P_L[j]) for j in range(8)], others)
    return r


def mul(a, b, trace=None):
    """a, b: limb lists of canonical elements.  Returns the limbs of a b R^-1 mod p.  trace (a list) receives, per step, the
    Montgomery digit."""
    va, vb = value(a), value(b)
    check(va < P and vb < P)
    L, H = [0] * 8, [0] * 8
    t_ref = 0
    for i in range(8):
        bi = b[i]                                             # limb i of b on every lane
        prod = [a[j] * bi + L[j] for j in range(8)]
        check(all(x < 2**64 for x in prod))
        lo, hi = [x & M32 for x in prod], [x >> 32 for x in prod]
        m = (-lo[0]) & M32                                    # lane 0's word on every lane
        if trace is not None:
            trace.append(m)
        _ev("mul.m_carry" if m else "mul.m_no_carry")
        up = from_upper(lo)
        keep = [hi[j] + H[j] + up[j] + (1 if j == 0 and m else 0) for j in range(8)]
        check(all(x < 3 * W for x in keep))
        s = [m * Q_L[j] + keep[j] for j in range(8)]
        check(all(x < 2**59 + 3 * W for x in s))             # fits 64 bits with room
        L, H = [x & M32 for x in s], [x >> 32 for x in s]
        if H[6] >= 2**27:
            _ev("mul.h6_ge_2_27")
        check(all(h < 2**28 for h in H) and all(H[j] <= 3 for j in (0, 1, 2, 3, 4, 7)))
        # the accumulator is what CIOS says it is
        t_ref = (t_ref + va * bi + m * P)
        check(t_ref % W == 0)
        t_ref //= W
        check(sum((L[j] + (H[j] << 32)) << (32 * j) for j in range(8)) == t_ref and t_ref < 2 * P)
    check(H[7] == 0)
    last = [L[j] + from_lower(H)[j] for j in range(8)]
    t, top = resolve(last)
    if t != [x & M32 for x in last]:
        _ev("mul.final_carry")
    check(top == 0 and value(t) == t_ref)
    r = reduce_once(t)
    check(value(r) == va * vb * R_INV % P)
    return r


def cube(x):
    return mul(mul(x, x), x)


R2_L = limbs(R * R % P)
ONE_L = limbs(R % P)


def to_mont(x):
    return mul(R2_L, x)


def from_mont(x):
    return mul(x, limbs(1))


def pack_m31x8(v):
    """v[0..7] M31 words, v[0] most significant; lane j is handed v[7 - j]."""
    rev = [v[7 - j] for j in range(8)]
    up = from_upper(rev)
    return [((rev[j] >> j) | (up[j] << (31 - j))) & M32 for j in range(8)]


def hades_mont(s0, s1, s2, rounds=91):
    """feltc::hades_coop on a Montgomery-form state of three limb lists; `rounds` < 91 stops after that many rounds."""
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
    """state: three canonical integers.  The permutation through the lane arithmetic, Montgomery form inside."""
    s = hades_mont(*(to_mont(limbs(x)) for x in state), rounds=rounds)
    return [value(from_mont(x)) for x in s]


def draw_slices(h):
    """The four words a draw_felt leaves: lane k < 4 takes bits [31 k, 31 k + 31) of h from limbs (31 k) >> 5 and the next, and
    reduces as M31.reduce does (2^31 - 1 -> 0)."""
    ls = limbs(h)
    out = []
    for k in range(4):
        l0, sh = (31 * k) >> 5, (31 * k) & 31
        word = (((ls[l0 + 1] << 32) | ls[l0]) >> sh) & 0x7FFFFFFF
        out.append(0 if word == 0x7FFFFFFF else word)
    return out

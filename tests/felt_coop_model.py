"""The lane algorithm of csrc/felt252_coop.cuh on Python integers: one element over 8 lanes, lane j holding limb j, one variable
per lane accumulator, and every accumulator's width asserted at every step.  It shares no code with the library; the arithmetic it
is checked against is Python's own (a * b * R^-1 mod p).

A "group" below is a list of 8 lane values.  resolve() is written for a whole wave (8 groups, 64 lanes, two 64-bit masks) because
that is where it can go wrong: a carry must not leave a group for its neighbour.
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
ARK = [[int.from_bytes(hashlib.sha256(f"Hades{3 * i + j}".encode()).digest(), "big") % P for j in range(3)] for i in range(91)]


def limbs(x):
    assert 0 <= x < R
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
    assert len(u) == 64
    G = Pm = 0
    for lane, x in enumerate(u):
        assert 0 <= x < 2**33, (lane, x)
        G |= (x >> 32 != 0) << lane
        Pm |= ((x & M32) == M32) << lane
    a, b = (G | Pm) & LOW7, G & LOW7
    s = a + b
    assert s <= M64                               # bits 8k + 7 of a and b are 0: the top bit of the sum never carries out
    C = s ^ a ^ b
    T = (G | (Pm & C)) & ~LOW7 & M64
    out = [((x & M32) + ((C >> lane) & 1)) & M32 for lane, x in enumerate(u)]
    top = [(T >> (lane | 7)) & 1 for lane in range(64)]
    return out, top


def resolve(g, others=None):
    """One group (8 lane values); `others`: what the 7 other groups of the wave hold (default: copies).  The group sits in slot 3."""
    wave = []
    for k in range(8):
        wave += list(g) if k == 3 or others is None else list(others[k if k < 3 else k - 1])
    out, top = resolve_wave(wave)
    res, t = out[24:32], top[24:32]
    assert len(set(t)) == 1
    # what it must be: the value mod 2^256 and the carry out of bit 256
    v = value(g)
    assert value(res) == v % R and t[0] == v >> 256, (g, res, t)
    return res, t[0]


def reduce_once(t, others=None):
    assert value(t) < 2 * P
    d, ge = resolve([t[j] + NEGP_L[j] for j in range(8)], others)
    return d if ge else list(t)


def add(a, b, others=None):
    s, top = resolve([a[j] + b[j] for j in range(8)], others)
    assert top == 0
    return reduce_once(s, others)


def dbl(a):
    return add(a, a)


def sub(a, b, others=None):
    d, no_borrow = resolve([a[j] + (~b[j] & M32) + (1 if j == 0 else 0) for j in range(8)], others)
    r, _ = resolve([d[j] + (0 if no_borrow else P_L[j]) for j in range(8)], others)
    return r


def mul(a, b, trace=None):
    """a, b: limb lists of canonical elements.  Returns the limbs of a b R^-1 mod p.  trace (a list) receives, per step, the
    Montgomery digit."""
    va, vb = value(a), value(b)
    assert va < P and vb < P
    L, H = [0] * 8, [0] * 8
    t_ref = 0
    for i in range(8):
        bi = b[i]                                             # limb i of b on every lane
        prod = [a[j] * bi + L[j] for j in range(8)]
        assert all(x < 2**64 for x in prod)
        lo, hi = [x & M32 for x in prod], [x >> 32 for x in prod]
        m = (-lo[0]) & M32                                    # lane 0's word on every lane
        if trace is not None:
            trace.append(m)
        up = from_upper(lo)
        keep = [hi[j] + H[j] + up[j] + (1 if j == 0 and m else 0) for j in range(8)]
        assert all(x < 3 * W for x in keep)
        s = [m * Q_L[j] + keep[j] for j in range(8)]
        assert all(x < 2**59 + 3 * W for x in s)             # fits 64 bits with room
        L, H = [x & M32 for x in s], [x >> 32 for x in s]
        assert all(h < 2**28 for h in H) and all(H[j] <= 3 for j in (0, 1, 2, 3, 4, 7))
        # the accumulator is what CIOS says it is
        t_ref = (t_ref + va * bi + m * P)
        assert t_ref % W == 0
        t_ref //= W
        assert sum((L[j] + (H[j] << 32)) << (32 * j) for j in range(8)) == t_ref and t_ref < 2 * P
    assert H[7] == 0
    t, top = resolve([L[j] + from_lower(H)[j] for j in range(8)])
    assert top == 0 and value(t) == t_ref
    r = reduce_once(t)
    assert value(r) == va * vb * R_INV % P
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


def hades(state):
    """state: three canonical integers.  The permutation through the lane arithmetic, Montgomery form inside."""
    s0, s1, s2 = (to_mont(limbs(x)) for x in state)
    for r in range(91):
        s0 = add(s0, limbs(ARK[r][0] * R % P))
        s1 = add(s1, limbs(ARK[r][1] * R % P))
        s2 = add(s2, limbs(ARK[r][2] * R % P))
        if r < 4 or r >= 87:
            s0, s1 = cube(s0), cube(s1)
        s2 = cube(s2)
        t = add(add(s0, s1), s2)
        s0, s1, s2 = add(t, dbl(s0)), sub(t, dbl(s1)), sub(t, add(dbl(s2), s2))
    return [value(from_mont(s)) for s in (s0, s1, s2)]


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

"""The 8-lane field arithmetic of csrc/felt252_coop.cuh, as restated lane by lane in tests/felt_coop_model.py (no GPU): every
accumulator stays inside its width at operands that reach the bounds, and every result is the field's."""
import random

import pytest

import felt_coop_model as C
import poseidon_model as PM

P, R = C.P, C.R


def _all_ones_below_p():
    """limb patterns of all-ones that are still canonical: the top limb of p is 2^27, so limb 7 stays below it"""
    out = []
    for top in (0, 1, (1 << 27) - 1):
        for mask in (0b1111111, 0b1010101, 0b0101010, 0b1000000, 0b0000001, 0b0111110):
            out.append(C.value([C.M32 if (mask >> j) & 1 else 0 for j in range(7)] + [top]))
    # limb 7 = 2^27 (p's own): canonical only below 17 2^192 + 1
    out += [2**251 + 17 * 2**192, 2**251 + 16 * 2**192 + (2**192 - 1), 2**251 + 2**192 - 1]
    return out


EDGES = [0, 1, 2, P - 1, P - 2, 2**251 - 1, 2**251, 2**192 * 17, 2**192 * 17 + 1, R % P, R * R % P, 2**32 - 1, 2**32, 2**224,
         (P - 1) // 2, (P + 1) // 2] + _all_ones_below_p()


def _pairs():
    rng = random.Random(252)
    pairs = [(a, b) for a in EDGES for b in EDGES]
    # an intermediate t0 of 0 (Montgomery digit 0, the branch without the limb-0 carry): limb 0 of a is 0, or b's limb i is 0
    zero_low = [x << 32 for x in (1, 2**200 - 1, rng.randrange(2**219))] + [rng.randrange(P) & ~((1 << 96) - 1) for _ in range(3)]
    pairs += [(a, rng.randrange(P)) for a in zero_low] + [(rng.randrange(P), b) for b in zero_low]
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(300)]
    return pairs


def test_mul_at_the_bounds():
    """every pair: the model asserts each accumulator's width and the CIOS invariant at every step, and the result"""
    digits_zero = 0
    for a, b in _pairs():
        assert a < P and b < P
        trace = []
        r = C.mul(C.limbs(a), C.limbs(b), trace)
        assert C.value(r) == a * b * C.R_INV % P
        digits_zero += sum(m == 0 for m in trace)
    assert digits_zero > 50                                  # the carry-free branch of the reduction was taken


def test_mul_largest_operands():
    r = C.mul(C.limbs(P - 1), C.limbs(P - 1))
    assert C.value(r) == (P - 1) * (P - 1) * C.R_INV % P
    assert C.value(C.to_mont(C.limbs(P - 1))) == (P - 1) * R % P
    assert C.value(C.from_mont(C.limbs(P - 1))) == (P - 1) * C.R_INV % P
    assert C.value(C.cube(C.to_mont(C.limbs(P - 2)))) == pow(P - 2, 3, P) * R % P


def test_add_sub_wrap_around():
    rng = random.Random(7)
    vals = EDGES + [rng.randrange(P) for _ in range(40)]
    noise = [[rng.randrange(2**33) for _ in range(8)] for _ in range(7)]      # the other groups of the wave: any lane values
    for a in vals:
        for b in vals:
            assert C.value(C.add(C.limbs(a), C.limbs(b))) == (a + b) % P
            assert C.value(C.sub(C.limbs(a), C.limbs(b))) == (a - b) % P
    for a, b in [(P - 1, 1), (P - 1, P - 1), (0, 1), (0, P - 1), (1, 2), (2**224 - 1, 1), (2**251, 17 * 2**192 + 1)]:
        assert C.value(C.add(C.limbs(a), C.limbs(b), noise)) == (a + b) % P
        assert C.value(C.sub(C.limbs(a), C.limbs(b), noise)) == (a - b) % P
        assert C.value(C.dbl(C.limbs(a))) == 2 * a % P


def test_carries_stay_inside_a_group():
    """a group of all-ones words (every lane propagates) next to a group that generates in limb 7's neighbour: the carry that
    enters lane 0 of the next group would change its result"""
    ones = [C.M32] * 7 + [0]
    gen = [0] * 6 + [2**32, 0]                               # carry into limb 7
    out, top = C.resolve_wave(gen + ones + ones + gen + ones + gen + gen + ones)
    assert out[:8] == [0] * 7 + [1] and out[8:16] == ones and top == [0] * 64
    full = [C.M32] * 8
    out, top = C.resolve_wave([1 + C.M32] + [C.M32] * 7 + full * 7)      # 2^256 exactly in group 0: top set there only
    assert out[:8] == [0] * 8 and top[:8] == [1] * 8 and top[8:] == [0] * 56 and out[8:] == full * 7


def test_pack_m31x8():
    m = 2**31 - 1
    rng = random.Random(3)
    for v in ([m] * 8, [0] * 8, [m, 0] * 4, [0, m] * 4, [1] + [0] * 7, [0] * 7 + [1], [rng.randrange(m + 1) for _ in range(8)]):
        assert C.value(C.pack_m31x8(v)) == PM.pack8(v)
    assert C.value(C.pack_m31x8([m] * 8)) == 2**248 - 1


@pytest.mark.parametrize("state", [[0, 0, 0], [1, 2, 3], [P - 1, P - 2, P - 1], [2**251 - 1, 2**192 * 17, R % P]])
def test_hades(state):
    assert C.hades(state) == PM.hades(state)


def test_draw_slices():
    """the 31-bit slicing of a draw, against the channel model's division; a slice of 2^31 - 1, which no hash will give on the
    device, reduces to 0"""
    rng = random.Random(11)
    m = 2**31 - 1
    for h in [0, P - 1, m, m << 31, m << 62, m << 93, (m << 31) | 5, (1 << 124) - 1, 2**251] + [rng.randrange(P) for _ in range(50)]:
        cur, want = h, []
        for _ in range(4):
            want.append((cur % 2**31) % m)
            cur //= 2**31
        assert C.draw_slices(h) == want
    assert C.draw_slices(m << 62) == [0, 0, 0, 0] and C.draw_slices((m << 62) | 1) == [1, 0, 0, 0]

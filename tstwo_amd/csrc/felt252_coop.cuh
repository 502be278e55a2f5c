// felt252_coop.cuh — the arithmetic of felt252.cuh with ONE element spread over 8 consecutive lanes: lane j of a group holds limb j
// (little-endian, canonical at rest, Montgomery form inside a kernel), a wave holds 8 groups.  A lone Hades permutation on
// felt252.cuh is one lane's instruction stream of ~1.2e5 VALU; here the eight a_j · b_i products of a CIOS step are one
// instruction of the group, so the stream a permutation waits for is a fraction as long.  tests/felt_coop_model.py
// restates every function below on Python integers, one variable per lane, with each accumulator's width asserted.
//
// Every operation takes canonical operands (< p) and returns a canonical result, bit-identical to felt::.  EVERY function here
// moves data across lanes: all 64 lanes of the wave must be active when it is called.  A kernel clamps the index of a tail group
// and masks its store; it never returns early from part of a wave.
//
// Cross-lane traffic: a neighbour's word travels by DPP (row_shl:1, no LDS), the word of one lane of a group to the whole group
// by two DPP row broadcasts (a DPP row is 16 lanes = 2 groups) and a select, carries by a carry-lookahead over the two
// wave-wide compare masks (generate / propagate) in scalar registers: no carry ripples lane by lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poseidon_constants.h"

namespace tstwo {
namespace feltc {

using felt::kArk;
using felt::kHadesRounds;

// What a lane knows about itself: its limb index and its limb of each constant.
struct Lane {
    uint32_t j;          // limb index, lane & 7
    uint32_t lane;       // lane of the wave
    uint32_t negp;       // limb j of 2^256 - p
    uint32_t p;          // limb j of p
    uint32_t q;          // the factor of the Montgomery digit m this lane adds after the shift: 17 (j = 5), 2^27 (j = 6), else 0
    uint32_t r2;         // limb j of R^2 mod p
    uint32_t one;        // limb j of R mod p
};

// v[j] of eight compile-time words for a lane-varying j: seven selects, no table in memory
__device__ __forceinline__ uint32_t pick8(uint32_t j, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4, uint32_t v5, uint32_t v6,
                                          uint32_t v7) {
    const uint32_t a = (j & 1) ? v1 : v0, b = (j & 1) ? v3 : v2, c = (j & 1) ? v5 : v4, d = (j & 1) ? v7 : v6;
    const uint32_t e = (j & 2) ? b : a, f = (j & 2) ? d : c;
    return (j & 4) ? f : e;
}

__device__ __forceinline__ Lane lane_info() {
    Lane l;
    l.lane = __lane_id();
    l.j = l.lane & 7u;
    const uint32_t j = l.j;
    l.p = j == 0 ? 1u : j == 6 ? 17u : j == 7 ? (1u << 27) : 0u;
    l.negp = j == 6 ? 0xffffffeeu : j == 7 ? 0xf7ffffffu : 0xffffffffu;      // 2^256 - p = ~p + 1, and limb 0 of ~p is 2^32 - 2
    l.q = j == 5 ? 17u : j == 6 ? (1u << 27) : 0u;
    l.r2 = pick8(j, felt::kR2[0], felt::kR2[1], felt::kR2[2], felt::kR2[3], felt::kR2[4], felt::kR2[5], felt::kR2[6], felt::kR2[7]);
    l.one = pick8(j, felt::kOneMont[0], felt::kOneMont[1], felt::kOneMont[2], felt::kOneMont[3], felt::kOneMont[4], felt::kOneMont[5],
                  felt::kOneMont[6], felt::kOneMont[7]);
    return l;
}

// the word of lane j + 1 of the group; 0 for limb 7
__device__ __forceinline__ uint32_t from_upper(const Lane &l, uint32_t x) {
    const uint32_t v = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101 /* row_shl:1 */, 0xf, 0xf, true);
    return l.j == 7u ? 0u : v;
}
// the word of lane j - 1 of the group; 0 for limb 0
__device__ __forceinline__ uint32_t from_lower(const Lane &l, uint32_t x) {
    const uint32_t v = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
    return l.j == 0u ? 0u : v;
}
// limb I of the group's element on every lane of the group
template <int I>
__device__ __forceinline__ uint32_t bcast(const Lane &l, uint32_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x150 + I /* row_newbcast:I */, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x158 + I /* row_newbcast:I+8 */, 0xf, 0xf, true);
    return (l.lane & 8u) ? hi : lo;
}

// Carry resolution of a group whose lane j holds u_j < 2^33, the value being Σ u_j 2^(32 j): returns limb j of the value mod 2^256
// and, in *top, the carry out of limb 7 (bit 256), the same on every lane of the group.  A lane generates a carry (u_j >= 2^32:
// its low word is then < 2^32 - 1, so a carry coming in does not add a second one) or propagates one (low word all ones); with
// G and P the wave's two masks, the carries INTO each lane are the carry bits of the 64-bit addition (G | P) + G.  Limb 7's bits
// are taken out of both masks, so no carry leaves a group for the next; its own carry out is g_7 | (p_7 & c_7).
__device__ __forceinline__ uint32_t resolve(const Lane &l, uint64_t u, uint32_t *top) {
    const uint32_t lo = (uint32_t)u;
    const uint64_t G = __ballot((uint32_t)(u >> 32) != 0u), P = __ballot(lo == 0xffffffffu);
    const uint64_t kLow7 = 0x7f7f7f7f7f7f7f7full;
    const uint64_t a = (G | P) & kLow7, b = G & kLow7;
    const uint64_t C = (a + b) ^ a ^ b;                            // bit l: the carry into lane l
    const uint64_t T = (G | (P & C)) & ~kLow7;                     // bit 8k + 7: the carry out of group k
    if (top) *top = (uint32_t)(T >> (l.lane | 7u)) & 1u;
    return lo + ((uint32_t)(C >> l.lane) & 1u);
}

// r = t - p if t >= p, else t; t < 2p, limb j of t per lane.  t - p = t + (2^256 - p) mod 2^256, and the carry out says t >= p.
__device__ __forceinline__ uint32_t reduce_once(const Lane &l, uint32_t t) {
    uint32_t ge;
    const uint32_t d = resolve(l, (uint64_t)t + l.negp, &ge);
    return ge ? d : t;
}

__device__ __forceinline__ uint32_t add(const Lane &l, uint32_t a, uint32_t b) {
    return reduce_once(l, resolve(l, (uint64_t)a + b, nullptr));    // a + b < 2p < 2^253: no carry out of limb 7
}
__device__ __forceinline__ uint32_t dbl(const Lane &l, uint32_t a) { return add(l, a, a); }

// a - b = a + ~b + 1 mod 2^256; no carry out means a < b: add p back
__device__ __forceinline__ uint32_t sub(const Lane &l, uint32_t a, uint32_t b) {
    uint32_t no_borrow;
    const uint32_t d = resolve(l, (uint64_t)a + (uint32_t)~b + (l.j == 0u ? 1u : 0u), &no_borrow);
    return resolve(l, (uint64_t)d + (no_borrow ? 0u : l.p), nullptr);
}

// The eight limbs of an element on every lane of its group: the b operand of mul (cube uses one for both products).
struct Bcast { uint32_t b[8]; };
__device__ __forceinline__ Bcast bcast_all(const Lane &l, uint32_t x) {
    Bcast r;
    r.b[0] = bcast<0>(l, x); r.b[1] = bcast<1>(l, x); r.b[2] = bcast<2>(l, x); r.b[3] = bcast<3>(l, x);
    r.b[4] = bcast<4>(l, x); r.b[5] = bcast<5>(l, x); r.b[6] = bcast<6>(l, x); r.b[7] = bcast<7>(l, x);
    return r;
}

// Montgomery product a·b·R^-1 mod p (CIOS).  The accumulator is T = Σ (L_j + H_j 2^32) 2^(32 j): lane j keeps a word L_j and a
// deferred carry H_j < 2^28.  Step i: every lane forms a_j b_i + L_j < 2^64 (low word lo_j, high word hi_j); the Montgomery digit is
// m = -lo_0, and T + a b_i + m p is divisible by 2^32 — limb 0 becomes 0 with a carry of (m != 0).  Dividing by 2^32 moves every
// limb one lane down: lane j takes lo_(j+1) from above and keeps hi_j + H_j (which stood one limb higher already), lane 0 adds
// the carry, and m p = m + 17 m 2^192 + m 2^251 lands as m · 17 in lane 5 and m · 2^27 in lane 6.  The sum is < 3 · 2^32 + 2^59:
// its low word is the new L_j, the rest the new H_j < 2^28.  T < 2p after every step, as in felt::mul.
__device__ __forceinline__ uint32_t mul(const Lane &l, uint32_t a, const Bcast &b) {
    uint32_t L = 0u, H = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t prod = (uint64_t)a * b.b[i] + L;
        const uint32_t lo = (uint32_t)prod, hi = (uint32_t)(prod >> 32);
        const uint32_t m = 0u - bcast<0>(l, lo);
        const uint64_t keep = (uint64_t)hi + H + from_upper(l, lo) + ((l.j == 0u && m != 0u) ? 1u : 0u);
        const uint64_t s = (uint64_t)m * l.q + keep;
        L = (uint32_t)s;
        H = (uint32_t)(s >> 32);
    }
    // T < 2p < 2^253: H_7 = 0; limb j of T is L_j + H_(j-1) plus carries
    const uint32_t t = resolve(l, (uint64_t)L + from_lower(l, H), nullptr);
    return reduce_once(l, t);
}
__device__ __forceinline__ uint32_t mul(const Lane &l, uint32_t a, uint32_t b) { return mul(l, a, bcast_all(l, b)); }

__device__ __forceinline__ uint32_t cube(const Lane &l, uint32_t x) {
    const Bcast b = bcast_all(l, x);
    return mul(l, mul(l, x, b), b);
}

__device__ __forceinline__ uint32_t to_mont(const Lane &l, uint32_t x) { return mul(l, l.r2, x); }   // commutative: broadcast x
__device__ __forceinline__ uint32_t from_mont(const Lane &l, uint32_t x) {
    Bcast one;
    one.b[0] = 1u;
#pragma unroll
    for (int k = 1; k < 8; k++) one.b[k] = 0u;
    return mul(l, x, one);
}

// felt::pack_m31x8 of eight M31 values v[0..7] (v[0] most significant): lane j passes v[7 - j], which stands at bit 31 j = 32 j - j:
// limb j is its bits from j upwards and, on top, the low bits of the value of lane j + 1.
__device__ __forceinline__ uint32_t pack_m31x8(const Lane &l, uint32_t v_rev) {
    const uint32_t up = from_upper(l, v_rev);                       // 0 for limb 7
    return (v_rev >> l.j) | (uint32_t)((uint64_t)up << (31u - l.j));
}

// The Hades permutation (felt::hades) on a Montgomery-form state.  Limb j of a round constant is a vector load from the table.
__device__ __forceinline__ void hades_coop(const Lane &l, uint32_t &s0, uint32_t &s1, uint32_t &s2) {
#pragma unroll 1
    for (int r = 0; r < kHadesRounds; r++) {
        s0 = add(l, s0, kArk[3 * r][l.j]);
        s1 = add(l, s1, kArk[3 * r + 1][l.j]);
        s2 = add(l, s2, kArk[3 * r + 2][l.j]);
        if (r < 4 || r >= kHadesRounds - 4) {
            s0 = cube(l, s0);
            s1 = cube(l, s1);
        }
        s2 = cube(l, s2);
        // (3a + b + c, a - b + c, a + b - 2c) = (t + 2a, t - 2b, t - 3c) with t = a + b + c
        const uint32_t t = add(l, add(l, s0, s1), s2);
        const uint32_t n0 = add(l, t, dbl(l, s0));
        const uint32_t n1 = sub(l, t, dbl(l, s1));
        const uint32_t n2 = sub(l, t, add(l, dbl(l, s2), s2));
        s0 = n0;
        s1 = n1;
        s2 = n2;
    }
}

}  // namespace feltc
}  // namespace tstwo

// felt252.cuh — arithmetic in the Starknet field F_p, p = 2^251 + 17·2^192 + 1, for the Poseidon252 kernels (poseidon.hip).
//
// An element is 8 little-endian 32-bit limbs.  Every loop below is fully unrolled, so each limb index is a compile-time
// constant and the limbs live in VGPRs (a runtime index would put the array in scratch).  Multiplication is Montgomery's with
// R = 2^256 (CIOS, one 32-bit digit per step).  p is sparse — limbs 0, 6 and 7 are 1, 17 and 2^27, the others 0 — and
// p ≡ 1 (mod 2^32), so the Montgomery digit is m = -t0 (mod 2^32) and adding m·p touches three limbs: the reduction of a step
// costs two v_mad_u64_u32 and a carry chain instead of eight products.
//
// Ranges: every operation takes canonical operands (< p) and returns a canonical result.  Values in device memory and across
// the C ABI are canonical and NOT in Montgomery form; to_mont / from_mont convert at the edges of a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poseidon_constants.h"

namespace tstwo {
namespace felt {

struct F {
    uint32_t v[8];
};

constexpr uint32_t kP[8] = {1u, 0u, 0u, 0u, 0u, 0u, 17u, 1u << 27};

__device__ __forceinline__ F from_limbs(const uint32_t (&x)[8]) {
    F r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = x[k];
    return r;
}

__device__ __forceinline__ F zero() {
    F r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = 0u;
    return r;
}

// r = t - p if t >= p, else t; t < 2p (so t < 2^253: no ninth limb)
__device__ __forceinline__ F reduce_once(const F &t) {
    F d;
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) d.v[k] = __builtin_subc(t.v[k], kP[k], b, &b);
    F r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = b ? t.v[k] : d.v[k];
    return r;
}

__device__ __forceinline__ F add(const F &a, const F &b) {
    F s;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s.v[k] = __builtin_addc(a.v[k], b.v[k], c, &c);
    return reduce_once(s);              // a + b < 2p < 2^256: the last carry is 0
}

__device__ __forceinline__ F dbl(const F &a) { return add(a, a); }

__device__ __forceinline__ F sub(const F &a, const F &b) {
    F d;
    uint32_t bw = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) d.v[k] = __builtin_subc(a.v[k], b.v[k], bw, &bw);
    // a < b: add p back (only limbs 0, 6 and 7 of p are nonzero; the carry ripples through the others)
    const uint32_t m = 0u - bw;
    F r;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = __builtin_addc(d.v[k], kP[k] & m, c, &c);
    return r;
}

// Montgomery product a·b·R^-1 mod p (CIOS).  After step i the accumulator t < 2p < 2^253, so it fits 8 limbs plus the ninth that
// the step's products spill into.
__device__ __forceinline__ F mul(const F &a, const F &b) {
    uint32_t t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        // t += a · b[i]
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t r = (uint64_t)a.v[j] * b.v[i] + t[j] + c;      // <= (2^32-1)^2 + 2 (2^32-1) = 2^64 - 1
            t[j] = (uint32_t)r;
            c = r >> 32;
        }
        t[8] += (uint32_t)c;
        // t = (t + m·p) / 2^32 with m = -t[0]: m·p = m + 17m·2^192 + m·2^251
        const uint32_t m = 0u - t[0];
        uint32_t cc = t[0] != 0u;                                          // t[0] + m = 2^32 (or 0 when t[0] = 0)
#pragma unroll
        for (int j = 1; j < 6; j++) t[j - 1] = __builtin_addc(t[j], 0u, cc, &cc);
        const uint64_t r6 = (uint64_t)m * 17u + t[6] + cc;
        t[5] = (uint32_t)r6;
        const uint64_t r7 = ((uint64_t)m << 27) + t[7] + (r6 >> 32);
        t[6] = (uint32_t)r7;
        const uint64_t r8 = (uint64_t)t[8] + (r7 >> 32);
        t[7] = (uint32_t)r8;
        t[8] = (uint32_t)(r8 >> 32);
    }
    F r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = t[k];
    return reduce_once(r);
}

__device__ __forceinline__ F cube(const F &x) { return mul(mul(x, x), x); }

__device__ __forceinline__ F to_mont(const F &x) { return mul(x, from_limbs(kR2)); }

__device__ __forceinline__ F from_mont(const F &x) {
    F one = zero();
    one.v[0] = 1u;
    return mul(x, one);
}

__device__ __forceinline__ F one_mont() { return from_limbs(kOneMont); }

// The column block of hashNode (vcs/poseidon252_merkle.ts:86-122): eight M31 values v[0..7] (each < 2^31) as
// Σ v[k] · 2^(31·(7-k)), the first column most significant.  248 bits, so canonical without a reduction.
__device__ __forceinline__ F pack_m31x8(const uint32_t (&w)[8]) {
    F r = zero();
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int bit = 31 * (7 - k);
        const int limb = bit / 32, sh = bit % 32;
        r.v[limb] |= w[k] << sh;
        if (sh > 1 && limb + 1 < 8) r.v[limb + 1] |= w[k] >> (32 - sh);   // sh <= 1: a 31-bit value does not reach the next limb
    }
    return r;
}

// Channel.trailing_zeros of a Poseidon252 digest (channel/poseidon.ts:209-229): the first 16 bytes of the 32-byte big-endian
// encoding read as a little-endian u128 — byte-reversed limbs 7, 6, 5, 4 — so the count starts at bit 248 of the element.
__device__ __forceinline__ uint32_t trailing_zeros(const F &x) {
    const uint32_t w0 = __builtin_bswap32(x.v[7]), w1 = __builtin_bswap32(x.v[6]);
    const uint32_t w2 = __builtin_bswap32(x.v[5]), w3 = __builtin_bswap32(x.v[4]);
    if (w0) return __builtin_ctz(w0);
    if (w1) return 32u + __builtin_ctz(w1);
    if (w2) return 64u + __builtin_ctz(w2);
    if (w3) return 96u + __builtin_ctz(w3);
    return 128u;
}

// The Hades permutation of Starknet's Poseidon on a Montgomery-form state: 91 rounds, 4 full, 83 partial, 4 full; a round adds
// its constants, cubes all three elements (full) or s2 only (partial), and multiplies by the MDS matrix
// [[3,1,1],[1,-1,1],[1,1,-2]].  The round index is wave-uniform, so kArk[3r + j] comes in through scalar loads.
__device__ __forceinline__ void hades(F &s0, F &s1, F &s2) {
#pragma unroll 1
    for (int r = 0; r < kHadesRounds; r++) {
        s0 = add(s0, from_limbs(kArk[3 * r]));
        s1 = add(s1, from_limbs(kArk[3 * r + 1]));
        s2 = add(s2, from_limbs(kArk[3 * r + 2]));
        if (r < 4 || r >= kHadesRounds - 4) {
            s0 = cube(s0);
            s1 = cube(s1);
        }
        s2 = cube(s2);
        // (3a + b + c, a - b + c, a + b - 2c) = (t + 2a, t - 2b, t - 3c) with t = a + b + c
        const F t = add(add(s0, s1), s2);
        const F n0 = add(t, dbl(s0));
        const F n1 = sub(t, dbl(s1));
        const F n2 = sub(t, add(dbl(s2), s2));
        s0 = n0;
        s1 = n1;
        s2 = n2;
    }
}

}  // namespace felt
}  // namespace tstwo

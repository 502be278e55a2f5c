// coset_order.cuh — where a coset row lives in a stored column (device; logup.hip and lookup.hip).
//
// Rows are stored bit-reversed on the circle domain; "previous row" (mask offset -1) is the coset order.  With L = log_size - 1,
// j = k >> 1 and rev = bit reversal over L bits, coset row k lives at
//   2 rev(j)                       for even k  (the A part of j)
//   2 (2^L - 1 - rev(j)) + 1       for odd k   (the B part of j; 2^L - 1 - rev(j) = ~rev(j) over L bits)
// (tstwo_amd/constraint_framework.py _coset_positions is the same closed form in numpy).
#pragma once
#include "m31.cuh"

namespace tstwo {

__device__ __forceinline__ u32 rev_bits(u32 x, u32 bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// storage position of coset row k; L = log_size - 1
__device__ __forceinline__ u32 coset_pos(u32 k, u32 L) {
    const u32 r = rev_bits(k >> 1, L);
    return (k & 1u) ? 2u * (((1u << L) - 1u) - r) + 1u : 2u * r;
}

// its inverse: the coset row stored at position p (an even p is the A part of rev(p / 2), an odd one the B part of rev(~(p / 2)))
__device__ __forceinline__ u32 coset_row(u32 p, u32 L) {
    const u32 h = p >> 1;
    return (p & 1u) ? 2u * rev_bits(((1u << L) - 1u) - h, L) + 1u : 2u * rev_bits(h, L);
}

}  // namespace tstwo

// eval_sum.cuh — what the two evaluate-at-a-point reductions share (poly_eval.hip: circle polynomials; mle_eval.hip: multilinear
// extensions): the reduction of a lazy 64-bit sum and the sum of one QM31 per lane over a workgroup.
#pragma once
#include "m31.cuh"

namespace tstwo {

__device__ __forceinline__ u32 red64(u64 x) {          // x < 2^64: canonical x mod P
    u64 f = (x & M31_P) + (x >> 31);                     // < 2^31 + 2^33
    return m31_reduce64(f);
}
// sum of one QM31 per lane over the workgroup (256 lanes); the result is valid in lane 0
__device__ __forceinline__ qm31 eval_wg_sum(qm31 v, qm31 *scratch /* >= 4 entries */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        qm31 o = {(u32)__shfl_down((int)v.a, off, 64), (u32)__shfl_down((int)v.b, off, 64), (u32)__shfl_down((int)v.c, off, 64),
                  (u32)__shfl_down((int)v.d, off, 64)};
        v = qm31_add(v, o);
    }
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = qm31_add(qm31_add(scratch[0], scratch[1]), qm31_add(scratch[2], scratch[3]));
    return v;
}

}  // namespace tstwo

// poly_eval.hip — PolyOps.eval_at_point: one polynomial, or every polynomial of one size, at one out-of-domain point; and groups of
// polynomials, each group at several points, in one call (tstwo_eval_at_points).
#include <string.h>

#include <vector>

#include "common.h"
#include "eval_sum.cuh"
#include "poly_eval_plan.h"

using namespace tstwo;

namespace {

// PolyOps.eval_at_point (backend/cpu/circle.ts:52-69) = fold(coeffs, [y, x, pi(x), pi^2(x), ...] reversed)
// (poly/utils.ts:36-59).  Unrolled, the fold is the multilinear form
//     value = sum_i coeffs[i] * prod_{s : bit s of i is set} fac[s],      fac = [y, x, pi(x), pi^2(x), ...],
// and the product splits over any partition of the index bits.  One pass over the coefficients (kernel E1), then one tiny
// kernel per further 12 index bits (E2):
//   E1  a workgroup of 256 lanes owns 4096 consecutive coefficients.  Lane t reads four 16-byte vectors, a KiB apart per
//       wave (fully coalesced): coefficient (r, t, j) = base + 1024 r + 4 t + j.  Bits {0,1} (j) and {10,11} (r) are the same
//       for every lane, so their 16 factor products W[r][j] arrive as kernel arguments (SGPRs) and the lane's 16 terms are
//       16 x 4 v_mad_u64_u32 (M31 x QM31 = 4 multiplications, accumulated lazily in 64 bits).  Bits 2..9 (t) give a
//       per-lane factor A[t & 15] * B[t >> 4] from two 16-entry tables that 32 lanes build in LDS while the loads are in
//       flight.  After that the workgroup's partial is a plain sum over lanes (DPP-free shuffles + one LDS hop).
//   E2  folds up to 4096 QM31 partials per workgroup the same way (QM31 x QM31 terms), bits 8..11 through a 16-entry
//       argument table, bits 0..7 through the lane factor.
// log 22: 1024 workgroups + one; the result is read back with one 16-byte copy.  Algorithmic bytes: 4 per coefficient.
struct EvalW { qm31 w[16]; };        // products over the 4 "uniform" bits of a level (entry 0 = 1)
struct EvalF { qm31 f[8]; };         // factors of the 8 lane bits of a level (A: f[0..3], B: f[4..7])

// lane factor tables: entry e < 16 = prod_{i<4, bit i of e} f[i]; entry 16 + e = the same over f[4..7]
__device__ __forceinline__ void eval_build_tables(qm31 *tab, const EvalF &ff) {
    const u32 t = threadIdx.x;
    if (t < 32) {
        const u32 e = t & 15;
        const int o = t < 16 ? 0 : 4;
        qm31 v = {1u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const qm31 f = (o == 0) ? ff.f[i] : ff.f[4 + i];
            const qm31 p = qm31_mul(v, f);
            if ((e >> i) & 1) v = p;
        }
        tab[t] = v;
    }
}

// Fold of up to 4096 QM31 partials by one workgroup (R = 16 per lane; fewer when `left` < 4096): entry i lives at
// in[i * elem_stride].  The result is valid in lane 0.
__device__ __forceinline__ qm31 eval_fold_partials(const qm31 *__restrict__ in, size_t elem_stride, size_t left, const EvalW &W, const EvalF &F,
                                                   qm31 *tab) {
    const u32 t = threadIdx.x;
    eval_build_tables(tab, F);
    __syncthreads();
    const qm31 ft = qm31_mul(tab[t & 15], tab[16 + (t >> 4)]);
    qm31 acc = {0u, 0u, 0u, 0u};
#pragma unroll 4
    for (int r = 0; r < 16; r++) {
        const size_t i = (size_t)r * 256 + t;
        if (i < left) acc = qm31_add(acc, qm31_mul(in[i * elem_stride], W.w[r]));
    }
    const qm31 v = qm31_mul(acc, ft);
    return eval_wg_sum(v, tab + 32);
}

// E1: coefficients -> one partial per chunk of 4096 * G coefficients.  grid = (chunks, columns).  G = 4 (64 coefficients
// per lane: the per-lane fixed work — lane factor, workgroup sum — is paid once per 64 instead of once per 16) when that still
// leaves >= 2 workgroups per CU, else G = 1.  Group g of a chunk (index bits 12, 13) is folded with the uniform factors H[g].
// n_coeffs < 4096 or unaligned columns take the guarded scalar loads (coefficients beyond the polynomial count as zero).
struct EvalH { qm31 h[4]; };         // h[g] = prod_{bit of g} fac[12 + bit]  (h[0] = 1)
// (A one-launch variant — the workgroup that arrives last on an agent-scope counter folds the partials itself, hand-off by the
// CDNA guide's release / acquire recipe — was built and measured: 28.7 us instead of 25.5 for one column of 2^22, 93 instead
// of 50 for 32 columns of 2^20: a release fence (L2 write-back) in every one of the 256 .. 2048 workgroups costs more than
// the second launch it saves.  Removed.)
template <bool FAST, int G>
__global__ void __launch_bounds__(256) k_eval_coeffs(ColPtrs cols, size_t n_coeffs, EvalW W, EvalF F, EvalH H, qm31 *__restrict__ partial_out,
                                                    size_t out_stride) {
    __shared__ qm31 tab[32 + 4];
    const u32 t = threadIdx.x;
    const u32 *__restrict__ c = colp_u(cols, blockIdx.y);
    const size_t base = (size_t)blockIdx.x * (4096 * G) + 4 * t;
    auto load_group = [&](uint4 (&x)[4], int g) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t i = base + 4096 * (size_t)g + 1024 * (size_t)r;
            if (FAST) {
                x[r] = gload4(c + i);
            } else {
                x[r].x = i + 0 < n_coeffs ? gload1(c + i + 0) : 0u; x[r].y = i + 1 < n_coeffs ? gload1(c + i + 1) : 0u;
                x[r].z = i + 2 < n_coeffs ? gload1(c + i + 2) : 0u; x[r].w = i + 3 < n_coeffs ? gload1(c + i + 3) : 0u;
            }
        }
    };
    uint4 x[4];
    load_group(x, 0);
    eval_build_tables(tab, F);               // overlaps the loads above
    __syncthreads();
    const qm31 ft = qm31_mul(tab[t & 15], tab[16 + (t >> 4)]);
    qm31 total = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < G; g++) {
        uint4 y[4];
        if (g + 1 < G) load_group(y, g + 1);       // next group's loads fly while this one is multiplied
        u32 ua = 0, ub = 0, uc = 0, ud = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const u32 v[4] = {x[r].x, x[r].y, x[r].z, x[r].w};
            u64 a = ua, b = ub, cc = uc, d = ud;     // 4 products < 2^62 each + carry-in < 2^31: no overflow
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const qm31 w = W.w[4 * r + j];
                a += (u64)v[j] * w.a; b += (u64)v[j] * w.b; cc += (u64)v[j] * w.c; d += (u64)v[j] * w.d;
            }
            ua = red64(a); ub = red64(b); uc = red64(cc); ud = red64(d);
        }
        const qm31 u = {ua, ub, uc, ud};
        total = g == 0 ? u : qm31_add(total, qm31_mul(u, H.h[g]));
        if (g + 1 < G) {
#pragma unroll
            for (int r = 0; r < 4; r++) x[r] = y[r];
        }
    }
    qm31 v = qm31_mul(total, ft);
    v = eval_wg_sum(v, tab + 32);
    if (t == 0) partial_out[(size_t)blockIdx.y * out_stride + blockIdx.x] = v;
}

// E2: QM31 partials -> one partial per 4096 of them.  grid = (groups, columns).
__global__ void __launch_bounds__(256) k_eval_partials(const qm31 *__restrict__ partial_in, size_t in_stride, size_t m_in, EvalW W, EvalF F,
                                                      qm31 *__restrict__ partial_out, size_t out_stride) {
    __shared__ qm31 tab[32 + 4];
    const qm31 *__restrict__ in = partial_in + (size_t)blockIdx.y * in_stride + (size_t)blockIdx.x * 4096;
    const size_t left = m_in - (size_t)blockIdx.x * 4096;      // entries of this group (>= 1)
    const qm31 v = eval_fold_partials(in, 1, left, W, F, tab);
    if (threadIdx.x == 0) partial_out[(size_t)blockIdx.y * out_stride + blockIdx.x] = v;
}

// ---- The same two kernels for K points in one sweep (tstwo_eval_at_points): every coefficient is loaded once and multiplied
// into the accumulators of K points.  The tables of point k are member k of the kernel's one by-value argument, and the kernels
// read them where they already are, in the kernel-argument segment, through the constant address space (scalar loads, as
// colp_u does for the pointer table): indexing a by-value argument with the point or group index would have the compiler copy
// the whole argument into scratch memory, and so does handing it to a lambda once it holds 3 or 4 points' tables.
template <int K> struct EvalPts { EvalW W[K]; EvalF F[K]; EvalH H[K]; };
template <int K> struct EvalPtsFold { EvalW W[K]; EvalF F[K]; };
template <int K> struct EvalCoeffsArgs {       // ColPtrs first: colp_u reads the pointer table at kernel-argument offset 0
    ColPtrs cols; size_t n_coeffs; EvalPts<K> T; qm31 *partial_out; size_t col_stride, pt_stride;
};
template <int K> struct EvalPartialsArgs { const qm31 *partial_in; size_t m_in; EvalPtsFold<K> T; qm31 *partial_out; size_t col_stride, pt_stride; };
template <class A>
__device__ __forceinline__ const __attribute__((address_space(4))) A *eval_kernarg() {
    return (const __attribute__((address_space(4))) A *)__builtin_amdgcn_kernarg_segment_ptr();
}
__device__ __forceinline__ qm31 ldq(const __attribute__((address_space(4))) qm31 &q) { return qm31{q.a, q.b, q.c, q.d}; }

#define TSTWO_KARG __attribute__((address_space(4)))
// lane factor tables of K points, 32 entries each (layout of eval_build_tables), built by 32 K lanes
template <int K>
__device__ __forceinline__ void eval_build_tables_pts(qm31 *tab, const TSTWO_KARG EvalF *F) {
    const u32 t = threadIdx.x;
    if (t < 32u * K) {
        const u32 e = t & 15, k = t >> 5;
        const bool hi = (t & 16) != 0;
        qm31 v = {1u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            qm31 f = hi ? ldq(F[0].f[4 + i]) : ldq(F[0].f[i]);
#pragma unroll
            for (int kk = 1; kk < K; kk++) {
                const qm31 o = hi ? ldq(F[kk].f[4 + i]) : ldq(F[kk].f[i]);
                if (k == (u32)kk) f = o;
            }
            const qm31 p = qm31_mul(v, f);
            if ((e >> i) & 1) v = p;
        }
        tab[t] = v;
    }
}
// eval_fold_partials (contiguous entries) with the tables in the kernel-argument segment
__device__ __forceinline__ qm31 eval_fold_partials_karg(const qm31 *__restrict__ in, size_t left, const TSTWO_KARG EvalW *W, const TSTWO_KARG EvalF *F,
                                                        qm31 *tab) {
    const u32 t = threadIdx.x;
    eval_build_tables_pts<1>(tab, F);
    __syncthreads();
    const qm31 ft = qm31_mul(tab[t & 15], tab[16 + (t >> 4)]);
    qm31 acc = {0u, 0u, 0u, 0u};
#pragma unroll 4
    for (int r = 0; r < 16; r++) {
        const size_t i = (size_t)r * 256 + t;
        if (i < left) acc = qm31_add(acc, qm31_mul(in[i], ldq(W->w[r])));
    }
    const qm31 v = qm31_mul(acc, ft);
    return eval_wg_sum(v, tab + 32);
}
// eval_wg_sum for K values at once (one barrier); the results are valid in lane 0
template <int K>
__device__ __forceinline__ void eval_wg_sum_pts(qm31 (&v)[K], qm31 *scratch /* >= 4 K entries */) {
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            qm31 o = {(u32)__shfl_down((int)v[k].a, off, 64), (u32)__shfl_down((int)v[k].b, off, 64), (u32)__shfl_down((int)v[k].c, off, 64),
                      (u32)__shfl_down((int)v[k].d, off, 64)};
            v[k] = qm31_add(v[k], o);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) scratch[4 * k + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++)
            v[k] = qm31_add(qm31_add(scratch[4 * k], scratch[4 * k + 1]), qm31_add(scratch[4 * k + 2], scratch[4 * k + 3]));
    }
}

// E1 for K points: tile geometry, load pipeline and FAST / guarded paths of k_eval_coeffs.  grid = (chunks, columns); the
// partial of (chunk x, column y, point k) goes to partial_out[y * col_stride + k * pt_stride + x].
template <bool FAST, int G, int K>
__global__ void __launch_bounds__(256) k_eval_coeffs_pts(EvalCoeffsArgs<K> args) {
    __shared__ qm31 tab[(32 + 4) * K];
    const TSTWO_KARG EvalCoeffsArgs<K> *A = eval_kernarg<EvalCoeffsArgs<K>>();
    const u32 t = threadIdx.x;
    const size_t n_coeffs = A->n_coeffs;
    const u32 *__restrict__ c = colp_u(args.cols, blockIdx.y);
    const size_t base = (size_t)blockIdx.x * (4096 * G) + 4 * t;
    auto load_group = [&](uint4 (&x)[4], int g) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t i = base + 4096 * (size_t)g + 1024 * (size_t)r;
            if (FAST) {
                x[r] = gload4(c + i);
            } else {
                x[r].x = i + 0 < n_coeffs ? gload1(c + i + 0) : 0u; x[r].y = i + 1 < n_coeffs ? gload1(c + i + 1) : 0u;
                x[r].z = i + 2 < n_coeffs ? gload1(c + i + 2) : 0u; x[r].w = i + 3 < n_coeffs ? gload1(c + i + 3) : 0u;
            }
        }
    };
    uint4 x[4];
    load_group(x, 0);
    eval_build_tables_pts<K>(tab, A->T.F);   // overlaps the loads above
    qm31 total[K];
#pragma unroll
    for (int k = 0; k < K; k++) total[k] = qm31{0u, 0u, 0u, 0u};
    for (int g = 0; g < G; g++) {            // (left to the compiler: H is read with a run-time g where it keeps the loop)
        uint4 y[4];
        if (g + 1 < G) load_group(y, g + 1);       // next group's loads fly while this one is multiplied
        u32 u[K][4];
#pragma unroll
        for (int k = 0; k < K; k++) u[k][0] = u[k][1] = u[k][2] = u[k][3] = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const u32 v[4] = {x[r].x, x[r].y, x[r].z, x[r].w};
#pragma unroll
            for (int k = 0; k < K; k++) {
                u64 a = u[k][0], b = u[k][1], cc = u[k][2], d = u[k][3];     // 4 products < 2^62 each + carry-in < 2^31: no overflow
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const qm31 w = ldq(A->T.W[k].w[4 * r + j]);
                    a += (u64)v[j] * w.a; b += (u64)v[j] * w.b; cc += (u64)v[j] * w.c; d += (u64)v[j] * w.d;
                }
                u[k][0] = red64(a); u[k][1] = red64(b); u[k][2] = red64(cc); u[k][3] = red64(d);
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const qm31 uk = {u[k][0], u[k][1], u[k][2], u[k][3]};
            total[k] = G == 1 ? uk : qm31_add(total[k], qm31_mul(uk, ldq(A->T.H[k].h[g])));     // h[0] = 1
        }
        if (g + 1 < G) {
#pragma unroll
            for (int r = 0; r < 4; r++) x[r] = y[r];
        }
    }
    __syncthreads();                         // the tables are complete
#pragma unroll
    for (int k = 0; k < K; k++) total[k] = qm31_mul(total[k], qm31_mul(tab[32 * k + (t & 15)], tab[32 * k + 16 + (t >> 4)]));
    eval_wg_sum_pts<K>(total, tab + 32 * K);
    if (t == 0) {
        qm31 *out = A->partial_out + (size_t)blockIdx.y * A->col_stride + blockIdx.x;
#pragma unroll
        for (int k = 0; k < K; k++) out[(size_t)k * A->pt_stride] = total[k];
    }
}

// E2 for K points: grid = (groups, columns, K).  Row (column y, point z) of the input holds m_in partials at
// partial_in[(y K + z) m_in ..]; it is folded with the tables of point z.
template <int K>
__global__ void __launch_bounds__(256) k_eval_partials_pts(EvalPartialsArgs<K> args) {
    __shared__ qm31 tab[32 + 4];
    const TSTWO_KARG EvalPartialsArgs<K> *A = eval_kernarg<EvalPartialsArgs<K>>();
    const u32 z = blockIdx.z;
    const size_t m_in = A->m_in;
    const qm31 *__restrict__ in = A->partial_in + ((size_t)blockIdx.y * K + z) * m_in + (size_t)blockIdx.x * 4096;
    const size_t left = m_in - (size_t)blockIdx.x * 4096;      // entries of this group (>= 1)
    const qm31 v = eval_fold_partials_karg(in, left, &A->T.W[z], &A->T.F[z], tab);
    if (threadIdx.x == 0) A->partial_out[(size_t)blockIdx.y * A->col_stride + (size_t)z * A->pt_stride + blockIdx.x] = v;
}
#undef TSTWO_KARG

}  // namespace

// eval_at_point of n_cols polynomials of one size at one point: kernels E1/E2 above, one read-back of 16 bytes per column.
static int eval_at_point_impl(const u32 *const *coeffs, size_t n_cols, u32 log_size, const u32 px[4], const u32 py[4], u32 *out) {
    Context &c = ctx();
    if (log_size == 0) {   // circle.ts:53-59: the constant polynomial
        for (size_t i = 0; i < n_cols; i++) {
            u32 v;
            { int rc2 = small_d2h(&v, coeffs[i], 4); if (rc2) return rc2; }
            out[4 * i] = v; out[4 * i + 1] = out[4 * i + 2] = out[4 * i + 3] = 0;
        }
        return TSTWO_OK;
    }
    // fac[s] multiplies every coefficient whose index has bit s set: y, x, pi(x), ... (circle.ts:61-67 before the reverse)
    const host::Q one = {{1, 0, 0, 0}}, zero = {{0, 0, 0, 0}};
    host::Q fac[44];
    fac[0] = to_hq(py);
    {
        host::Q x = to_hq(px);
        for (u32 i = 1; i < log_size; i++) {
            fac[i] = x;
            host::Q sx = host::qmul(x, x);
            x = host::qsub(host::qadd(sx, sx), one);   // circle.ts:37-40
        }
        for (u32 i = log_size; i < 44; i++) fac[i] = zero;   // bits the polynomial does not have: those coefficients are zero
    }
    auto level_tables = [&](const int (&wbits)[4], u32 lane_bit0, EvalW &W, EvalF &F) {
        for (int e = 0; e < 16; e++) {
            host::Q v = one;
            for (int i = 0; i < 4; i++)
                if ((e >> i) & 1) v = host::qmul(v, fac[wbits[i]]);
            W.w[e] = to_q(v);
        }
        for (int i = 0; i < 8; i++) F.f[i] = to_q(fac[lane_bit0 + i]);
    };
    const size_t n_coeffs = (size_t)1 << log_size;
    // 64 coefficients per lane (G = 4) when the grid still has a workgroup per CU, else 16 (G = 1)
    const u32 glog = (log_size >= 14 && (((size_t)1 << (log_size - 14)) * n_cols >= (size_t)c.n_cus)) ? 2u : 0u;
    const u32 chunk_log = 12 + glog;
    const size_t chunks = log_size > chunk_log ? (size_t)1 << (log_size - chunk_log) : 1;
    const size_t groups1 = chunks > 4096 ? chunks / 4096 : 1;
    bool aligned = true;
    for (size_t i = 0; i < n_cols; i++) aligned = aligned && ((((uintptr_t)coeffs[i]) & 15) == 0);
    const bool fast = log_size >= chunk_log && aligned;
    const size_t kChunkCols = 32768;                       // gridDim.y limit
    for (size_t col0 = 0; col0 < n_cols; col0 += kChunkCols) {
        const size_t g = n_cols - col0 < kChunkCols ? n_cols - col0 : kChunkCols;
        int rc = ensure_scratch((g * (chunks + groups1) + 8) * sizeof(qm31));
        if (rc) return rc;
        qm31 *bufA = (qm31 *)c.scratch, *bufB = bufA + g * chunks;
        // the last level stores its g results straight into the page-locked host buffer (device-visible): the call then ends
        // with one stream synchronisation instead of a copy + synchronisation
        qm31 *host_dst = (c.pinned && g * sizeof(qm31) <= kPinnedBytes) ? (qm31 *)c.pinned : nullptr;
        ColPtrs cp;
        rc = fill_col_table(cp, coeffs + col0, g, 0);
        if (rc) return rc;
        EvalW W;
        EvalF F;
        qm31 *src = bufA, *dst = bufB;
        size_t m_in = chunks;
        u32 bit0 = chunk_log;
        {   // E1: bits 0,1 (j) and 10,11 (r) through W[4 r + j]; bits 2..9 are the lane bits; bits 12,13 the groups of a chunk
            const int wb[4] = {0, 1, 10, 11};
            level_tables(wb, 2, W, F);
            EvalH H;
            H.h[0] = to_q(one); H.h[1] = to_q(fac[12]); H.h[2] = to_q(fac[13]); H.h[3] = to_q(host::qmul(fac[12], fac[13]));
            const size_t stride = chunks == 1 ? 1 : chunks;
            qm31 *o = (chunks == 1 && host_dst) ? host_dst : bufA;
            const dim3 grid((unsigned)chunks, (unsigned)g);
            if (glog) {
                if (fast) hipLaunchKernelGGL((k_eval_coeffs<true, 4>), grid, dim3(256), 0, c.stream, cp, n_coeffs, W, F, H, o, stride);
                else hipLaunchKernelGGL((k_eval_coeffs<false, 4>), grid, dim3(256), 0, c.stream, cp, n_coeffs, W, F, H, o, stride);
            } else {
                if (fast) hipLaunchKernelGGL((k_eval_coeffs<true, 1>), grid, dim3(256), 0, c.stream, cp, n_coeffs, W, F, H, o, stride);
                else hipLaunchKernelGGL((k_eval_coeffs<false, 1>), grid, dim3(256), 0, c.stream, cp, n_coeffs, W, F, H, o, stride);
            }
        }
        while (m_in > 1) {   // E2: 12 more bits per level (lane bits bit0..bit0+7, W over bit0+8..bit0+11)
            const int wb[4] = {(int)bit0 + 8, (int)bit0 + 9, (int)bit0 + 10, (int)bit0 + 11};
            level_tables(wb, bit0, W, F);
            const size_t groups = m_in > 4096 ? m_in / 4096 : 1;
            hipLaunchKernelGGL(k_eval_partials, dim3((unsigned)groups, (unsigned)g), dim3(256), 0, c.stream, (const qm31 *)src, m_in, m_in, W, F,
                               (groups == 1 && host_dst) ? host_dst : dst, groups);
            qm31 *tmp = src; src = dst; dst = tmp;
            m_in = groups;
            bit0 += 12;
        }
        TSTWO_LAUNCH_CHECK();
        // one QM31 per column, contiguous (the last level has stride 1)
        if (host_dst) {
            if (int rcw = wait_stream()) return rcw;
            memcpy(out + 4 * col0, host_dst, g * sizeof(qm31));
        } else {
            rc = small_d2h(out + 4 * col0, src, g * sizeof(qm31));
            if (rc) return rc;
        }
    }
    return TSTWO_OK;
}

// ---- tstwo_eval_at_points: groups of columns, each group at its own points (plan: poly_eval_plan.h)
namespace {

static_assert(kEvalPtsPinnedBytes == kPinnedBytes, "poly_eval_plan.h restates kPinnedBytes");
static_assert(kEvalPtsMaxPoints == TSTWO_EVAL_MAX_POINTS, "poly_eval_plan.h restates TSTWO_EVAL_MAX_POINTS");

struct PointFactors { host::Q fac[44]; };      // fac[s] multiplies every coefficient whose index has bit s set; zero beyond the polynomial

PointFactors point_factors(u32 log_size, const u32 *point /* x[4], y[4] */) {
    const host::Q one = {{1, 0, 0, 0}}, zero = {{0, 0, 0, 0}};
    PointFactors pf;
    pf.fac[0] = to_hq(point + 4);
    host::Q x = to_hq(point);
    for (u32 i = 1; i < log_size; i++) {
        pf.fac[i] = x;
        host::Q sx = host::qmul(x, x);
        x = host::qsub(host::qadd(sx, sx), one);   // circle.ts:37-40
    }
    for (u32 i = log_size; i < 44; i++) pf.fac[i] = zero;   // log 0: every factor is zero, the value is coefficient 0
    return pf;
}
void level_tables(const PointFactors &pf, int wbit0, int wbit1, int wbit2, int wbit3, u32 lane_bit0, EvalW &W, EvalF &F) {
    const int wbits[4] = {wbit0, wbit1, wbit2, wbit3};
    for (int e = 0; e < 16; e++) {
        host::Q v = {{1, 0, 0, 0}};
        for (int i = 0; i < 4; i++)
            if ((e >> i) & 1) v = host::qmul(v, pf.fac[wbits[i]]);
        W.w[e] = to_q(v);
    }
    for (int i = 0; i < 8; i++) F.f[i] = to_q(pf.fac[lane_bit0 + i]);
}

// One sweep: `cols` columns (table cp) at the K points pf[0..K); the last level stores the value of (column i, point k) at
// result[i * result_col_stride + k].  Enqueues only.
template <int K>
void enqueue_sweep(const ColPtrs &cp, size_t cols, u32 log_size, const EvalPointsPlan &p, const PointFactors *pf, qm31 *partials, qm31 *result,
                   size_t result_col_stride) {
    Context &c = ctx();
    const size_t n_coeffs = (size_t)1 << log_size;
    const size_t chunks = (size_t)p.chunks;
    {   // E1: bits 0,1 (j) and 10,11 (r) through W[4 r + j]; bits 2..9 are the lane bits; bits 12,13 the groups of a chunk
        EvalCoeffsArgs<K> A;
        EvalPts<K> &T = A.T;
        for (int k = 0; k < K; k++) {
            level_tables(pf[k], 0, 1, 10, 11, 2, T.W[k], T.F[k]);
            T.H[k].h[0] = to_q(host::Q{{1, 0, 0, 0}}); T.H[k].h[1] = to_q(pf[k].fac[12]); T.H[k].h[2] = to_q(pf[k].fac[13]);
            T.H[k].h[3] = to_q(host::qmul(pf[k].fac[12], pf[k].fac[13]));
        }
        const bool last = p.levels == 1;
        A.cols = cp; A.n_coeffs = n_coeffs;
        A.partial_out = last ? result : partials;
        A.col_stride = last ? result_col_stride : (size_t)K * chunks; A.pt_stride = last ? 1 : chunks;
        const dim3 grid((unsigned)chunks, (unsigned)cols);
        if (p.g == 4) {
            if (p.fast) hipLaunchKernelGGL((k_eval_coeffs_pts<true, 4, K>), grid, dim3(256), 0, c.stream, A);
            else hipLaunchKernelGGL((k_eval_coeffs_pts<false, 4, K>), grid, dim3(256), 0, c.stream, A);
        } else {
            if (p.fast) hipLaunchKernelGGL((k_eval_coeffs_pts<true, 1, K>), grid, dim3(256), 0, c.stream, A);
            else hipLaunchKernelGGL((k_eval_coeffs_pts<false, 1, K>), grid, dim3(256), 0, c.stream, A);
        }
    }
    qm31 *src = partials, *dst = partials + cols * K * chunks;
    size_t m_in = chunks;
    u32 bit0 = p.chunk_log;
    while (m_in > 1) {   // E2: 12 more bits per level (lane bits bit0..bit0+7, W over bit0+8..bit0+11)
        EvalPartialsArgs<K> A;
        for (int k = 0; k < K; k++) level_tables(pf[k], (int)bit0 + 8, (int)bit0 + 9, (int)bit0 + 10, (int)bit0 + 11, bit0, A.T.W[k], A.T.F[k]);
        const size_t groups = m_in > 4096 ? m_in / 4096 : 1;
        const bool last = groups == 1;
        A.partial_in = src; A.m_in = m_in;
        A.partial_out = last ? result : dst;
        A.col_stride = last ? result_col_stride : (size_t)K * groups; A.pt_stride = last ? 1 : groups;
        hipLaunchKernelGGL((k_eval_partials_pts<K>), dim3((unsigned)groups, (unsigned)cols, K), dim3(256), 0, c.stream, A);
        src = dst;
        m_in = groups;
        bit0 += 12;
    }
}

int eval_at_points_impl(const u32 *const *coeffs, const u32 *group_cols, const u32 *group_logs, const u32 *group_points, size_t n_groups,
                        const u32 *points, u32 *out) {
    Context &c = ctx();
    std::vector<EvalPointsPlan> plans(n_groups);
    size_t results = 0, partial_qm31 = 0, col0 = 0;
    for (size_t g = 0; g < n_groups; g++) {
        bool aligned = true;
        for (size_t i = 0; i < group_cols[g]; i++) aligned = aligned && aligned16(coeffs[col0 + i]);
        if (const char *why = eval_points_plan(group_logs[g], group_cols[g], group_points[g], aligned, plans[g]))
            return set_error(TSTWO_ERR_BAD_ARG, std::string("eval_at_points: ") + why);
        if (plans[g].scratch_qm31 > partial_qm31) partial_qm31 = plans[g].scratch_qm31;
        results += (size_t)group_cols[g] * group_points[g];
        col0 += group_cols[g];
    }
    // One scratch block for the whole call, taken before the first launch.  Launches of one stream run in order, so every sweep
    // uses the same partial slots; the results of all groups form one contiguous region: the page-locked page (device-visible)
    // when they fit, else device scratch behind the partials and one copy.
    const bool pinned = c.pinned && eval_points_result_pinned(results);
    if (int rc = ensure_scratch((partial_qm31 + (pinned ? 0 : results) + 8) * sizeof(qm31))) return rc;
    qm31 *partials = (qm31 *)c.scratch;
    qm31 *result = pinned ? (qm31 *)c.pinned : partials + partial_qm31;
    // What a group's launches read stays valid until they have run, however many groups are in flight before the single wait:
    // factor tables and up to 64 column pointers travel by value in the kernel arguments; a longer pointer table goes into a
    // device slot of fill_col_table, whose upload is ordered on the stream behind the kernels still reading the slot's previous
    // content (small_h2d), and a slot is only ever freed after a stream synchronisation (context.hip: fill_col_table).
    size_t res0 = 0, pt0 = 0;
    col0 = 0;
    for (size_t g = 0; g < n_groups; g++) {
        const EvalPointsPlan &p = plans[g];
        const u32 n_pts = group_points[g], log_size = group_logs[g];
        PointFactors pf[TSTWO_EVAL_MAX_POINTS];
        for (u32 k = 0; k < n_pts; k++) pf[k] = point_factors(log_size, points + 8 * (pt0 + k));
        for (size_t s0 = 0; s0 < group_cols[g]; s0 += kEvalPtsSlabCols) {
            const size_t cols = group_cols[g] - s0 < kEvalPtsSlabCols ? group_cols[g] - s0 : kEvalPtsSlabCols;
            ColPtrs cp;
            if (int rc = fill_col_table(cp, coeffs + col0 + s0, cols, 0)) return rc;
            for (u32 k0 = 0; k0 < n_pts; k0 += kEvalPtsMaxK) {
                const u32 K = n_pts - k0 < kEvalPtsMaxK ? n_pts - k0 : kEvalPtsMaxK;
                qm31 *r = result + res0 + s0 * n_pts + k0;
                switch (K) {
                    case 1: enqueue_sweep<1>(cp, cols, log_size, p, pf + k0, partials, r, n_pts); break;
                    case 2: enqueue_sweep<2>(cp, cols, log_size, p, pf + k0, partials, r, n_pts); break;
                    case 3: enqueue_sweep<3>(cp, cols, log_size, p, pf + k0, partials, r, n_pts); break;
                    default: enqueue_sweep<4>(cp, cols, log_size, p, pf + k0, partials, r, n_pts); break;
                }
            }
        }
        res0 += (size_t)group_cols[g] * n_pts;
        pt0 += n_pts;
        col0 += group_cols[g];
    }
    TSTWO_LAUNCH_CHECK();
    if (pinned) {
        if (int rc = wait_stream()) return rc;
        memcpy(out, c.pinned, results * sizeof(qm31));
        return TSTWO_OK;
    }
    return small_d2h(out, result, results * sizeof(qm31));
}

}  // namespace

extern "C" {

// PolyOps.eval_at_point (backend/cpu/circle.ts:52-69) for every (column, point) pair CommitmentSchemeProver.prove_values asks for
// (packages/core/src/pcs/prover.ts:94-106 loops per column over that column's points): groups of columns, each group at its own
// points, every coefficient loaded once per sweep of up to 4 points, one read-back for the call.
int tstwo_eval_at_points(const u32 *const *coeffs, const u32 *group_cols, const u32 *group_logs, const u32 *group_points, size_t n_groups,
                         const u32 *points, u32 *out) {
    TSTWO_REQUIRE_READY();
    if (n_groups == 0) return TSTWO_OK;
    auto bad = [](const char *why) { return set_error(TSTWO_ERR_BAD_ARG, std::string("eval_at_points: ") + why); };
    if (!coeffs || !group_cols || !group_logs || !group_points || !points || !out) return bad("null argument");
    size_t n_cols = 0, n_points = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (group_cols[g] == 0) return bad("a group without columns");
        if (group_points[g] < 1 || group_points[g] > TSTWO_EVAL_MAX_POINTS) return bad("1 to 16 points per group");
        if (group_logs[g] > kEvalPtsMaxLog) return bad("log size out of range");
        n_cols += group_cols[g];
        n_points += group_points[g];
    }
    for (size_t i = 0; i < n_cols; i++)
        if (!coeffs[i]) return bad("null argument");
    for (size_t k = 0; k < 8 * n_points; k++)
        if (points[k] >= M31_P) return bad("point word out of range");
    if (stream_is_capturing()) return bad("host read-back during graph capture (the values cannot be recorded)");
    return eval_at_points_impl(coeffs, group_cols, group_logs, group_points, n_groups, points, out);
}

int tstwo_eval_at_point(const u32 *coeffs, u32 log_size, const u32 px[4], const u32 py[4], u32 out[4]) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(coeffs, px, py, out);
    if (log_size > 31) return set_error(TSTWO_ERR_BAD_ARG, "eval_at_point: log size out of range");
    return eval_at_point_impl(&coeffs, 1, log_size, px, py, out);
}

// eval_at_point of n_cols polynomials of one size at one point (CommitmentSchemeProver.prove_values samples every
// column of a tree at the same out-of-domain point, pcs/prover.ts Rust text :93-110): one launch sequence and one
// read-back for all of them.  out = 4 words per column.
int tstwo_eval_at_point_batch(const u32 *const *coeffs, size_t n_cols, u32 log_size, const u32 px[4], const u32 py[4], u32 *out) {
    TSTWO_REQUIRE_READY();
    if (n_cols == 0) return TSTWO_OK;
    if (!coeffs || !out) return set_error(TSTWO_ERR_BAD_ARG, "eval_at_point: null argument");
    TSTWO_REQUIRE_TABLE(coeffs, n_cols); TSTWO_REQUIRE_PTRS(px, py);
    if (log_size > 31) return set_error(TSTWO_ERR_BAD_ARG, "eval_at_point: log size out of range");
    return eval_at_point_impl(coeffs, n_cols, log_size, px, py, out);
}

}  // extern "C"

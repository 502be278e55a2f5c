// poly_eval.hip — PolyOps.eval_at_point: one polynomial, or every polynomial of one size, at one out-of-domain point.
#include <string.h>

#include "common.h"
#include "eval_sum.cuh"

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

extern "C" {

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

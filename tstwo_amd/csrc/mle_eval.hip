// mle_eval.hip — Mle.evalAtPoint (lookups/mle.ts:81-114): every MLE of one size, base or secure, at one point.
//
//     value = sum_i f[i] * prod_j (bit_{n-1-j}(i) ? p_j : 1 - p_j)            (the first variable is the most significant bit)
//
// The reference fixes one variable after the other (n passes, 2x the input in all).  Unrolled it is the multilinear form of
// poly_eval.hip's eval_at_point with the factor pair (1 - p, p) per index bit in place of (1, fac), and the product splits over
// any partition of the index bits in the same way.  Index bit s belongs to p_{n-1-s}; a bit the MLE does not have takes p = 0,
// i.e. the pair (1, 0).  One pass over the input, no eq table, no launch per variable (plan: mle_eval_plan.h):
//   pass 1  k_mle_first: a workgroup of 256 lanes owns a chunk of 4096 G consecutive values.  Lane t reads four 16-byte vectors
//           per group, a KiB apart per wave: value (g, r, t, j) = chunk + 4096 g + 1024 r + 4 t + j.  Bits {0,1} (j) and {10,11}
//           (r) are wave-uniform: their 16 products W[4r + j] are kernel arguments (SGPRs) and a lane's 16 terms are 16 x 4
//           v_mad_u64_u32.  Bits 2..9 (t) give the lane factor A[t & 15] * B[t >> 4] from two 16-entry LDS tables that 32 lanes
//           build while the loads are in flight.  Bits 12, 13 (g) are the uniform H[g].
//           A secure MLE is f = f_0 + i f_1 + u f_2 + iu f_3 over its 4 coordinate columns, so a QM31 x QM31 term is
//           f[i] w = sum_k f_k[i] (e_k w): the 4 groups of the workgroup are the 4 coordinate columns at the SAME 4096 positions,
//           each summed against W like a base column (M31 x QM31, all terms positive, lazy), and group k's sum is multiplied by
//           the basis element e_k (negations and one (2 + i): no field multiplication) where a base chunk multiplies by H[g].
//           16 multiplications per QM31 value, as many as ONE qm31_mul, and no reduction per term.
//           Lazy accumulation: the 4 products of a row r (< (P - 1)^2 each) plus the canonical carry-in stay below
//           4 (2^31 - 2)^2 + 2^31 < 2^64, then one reduction.  tests/test_gpu_mle_eval.py runs the all-(P - 1) case.
//   pass 2  k_mle_partials, when an MLE has more than one chunk: one workgroup per MLE folds its partials (at most 2^16), 256
//           per block: the lane factor over the block's 8 bits, a per-block factor over the next 8 from a second table pair.
// Both passes end in a plain sum over the workgroup (M31 addition is exact: the order changes nothing).  The last pass stores one
// QM31 per MLE into page-locked host memory, so the batch costs one stream synchronisation.
// Algorithmic bytes: 4 per value of a base MLE, 16 per value of a secure one.
#include <string.h>
#include <string>
#include <type_traits>

#include "common.h"
#include "eval_sum.cuh"
#include "mle_eval_plan.h"

using namespace tstwo;

namespace {

struct MleW { qm31 w[16]; };         // products over the 4 wave-uniform bits of pass 1
struct MleF { qm31 p[8]; };          // the point's coordinate for 8 consecutive index bits (0: a bit the MLE does not have)
struct MleH { qm31 h[4]; };          // base, 4 groups: products over bits 12, 13

// lanes [lane0, lane0 + 32) build tab[0 .. 32): entry e < 16 = prod_{i<4} (bit i of e ? p[i] : 1 - p[i]); entry 16 + e = the
// same over p[4..7]
__device__ __forceinline__ void mle_build_tables(qm31 *tab, const MleF &ff, u32 lane0) {
    const u32 t = threadIdx.x - lane0;
    if (t < 32) {
        const u32 e = t & 15;
        const int o = t < 16 ? 0 : 4;
        const qm31 one = {1u, 0u, 0u, 0u};
        qm31 v = one;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const qm31 p = (o == 0) ? ff.p[i] : ff.p[4 + i];
            v = qm31_mul(v, ((e >> i) & 1) ? p : qm31_sub(one, p));
        }
        tab[t] = v;
    }
}
// x e_k for the basis 1, i, u, iu of QM31 over M31 (i^2 = -1, u^2 = 2 + i)
template <int K>
__device__ __forceinline__ qm31 mle_mul_basis(qm31 x) {
    if constexpr (K == 0) return x;
    else if constexpr (K == 1) return {m31_neg(x.b), x.a, m31_neg(x.d), x.c};
    else if constexpr (K == 2) return {m31_sub(m31_double(x.c), x.d), m31_add(x.c, m31_double(x.d)), x.a, x.b};
    else return mle_mul_basis<1>(mle_mul_basis<2>(x));
}

// Pass 1.  grid = (chunks, MLEs).  SECURE: G = 4 and group g is coordinate column 4 y + g; base: group g is index bits 12, 13.
// FAST = false: guarded word loads (an MLE smaller than a chunk, or a column that is not 16-byte aligned).
template <bool SECURE, bool FAST, int G>
__global__ void __launch_bounds__(256) k_mle_first(ColPtrs cols, u32 n_vals, MleW W, MleF F, MleH H, qm31 *__restrict__ out, u32 out_stride) {
    static_assert(!SECURE || G == 4, "a secure MLE has 4 coordinate columns");
    __shared__ qm31 tab[32 + 4];
    const u32 t = threadIdx.x;
    const u32 base = blockIdx.x * (SECURE ? 4096u : 4096u * G) + 4 * t;
    auto load_group = [&](uint4 (&x)[4], int g) {
        // (a secure group's pointer is fetched here, one scalar load per group, not all four up front: fewer live SGPRs)
        const u32 *__restrict__ c = colp_u(cols, SECURE ? 4 * blockIdx.y + (u32)g : blockIdx.y);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const u32 i = base + (SECURE ? 0u : 4096u * (u32)g) + 1024u * (u32)r;
            if (FAST) {
                x[r] = gload4(c, i);
            } else {
                // Nothing past the MLE is read: the address is clamped to its last value.  The word read for a position
                // i >= n_vals needs no masking: such an i has an index bit the MLE does not have, whose factor pair is (1, 0), so
                // its term is a canonical word times zero.  (Masking it cost 16 live lane masks and SGPR spills.)
                x[r] = make_uint4(gload1(c, min(i + 0, n_vals - 1)), gload1(c, min(i + 1, n_vals - 1)),
                                  gload1(c, min(i + 2, n_vals - 1)), gload1(c, min(i + 3, n_vals - 1)));
            }
        }
    };
    uint4 x[4];
    load_group(x, 0);
    mle_build_tables(tab, F, 0);             // overlaps the loads above
    __syncthreads();
    const qm31 ft = qm31_mul(tab[t & 15], tab[16 + (t >> 4)]);
    qm31 total = {0u, 0u, 0u, 0u};
    auto group = [&](auto gc) {
        constexpr int g = decltype(gc)::value;
        uint4 y[4];
        if (g + 1 < G) load_group(y, g + 1);       // the next group's loads fly while this one is multiplied
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
        if (SECURE) total = g == 0 ? u : qm31_add(total, mle_mul_basis<g>(u));
        else if (G == 1) total = u;
        else total = g == 0 ? qm31_mul(u, H.h[0]) : qm31_add(total, qm31_mul(u, H.h[g]));      // H[0] = (1 - p)(1 - p'), not 1
        if (g + 1 < G) {
#pragma unroll
            for (int r = 0; r < 4; r++) x[r] = y[r];
        }
    };
    group(std::integral_constant<int, 0>{});
    if constexpr (G == 4) {
        group(std::integral_constant<int, 1>{});
        group(std::integral_constant<int, 2>{});
        group(std::integral_constant<int, 3>{});
    }
    qm31 v = qm31_mul(total, ft);
    v = eval_wg_sum(v, tab + 32);
    if (t == 0) out[(size_t)blockIdx.y * out_stride + blockIdx.x] = v;
}

// Pass 2.  grid = (1, MLEs): partial q of MLE y is in[y * chunks + q]; lane t takes q = 256 b + t for every block b.
// F: the 8 index bits above the chunk (q's bits 0..7, the lane), F2: the 8 above those (q's bits 8..15, the block).
__global__ void __launch_bounds__(256) k_mle_partials(const qm31 *__restrict__ partials, u32 chunks, MleF F, MleF F2, qm31 *__restrict__ out) {
    __shared__ qm31 tab[64 + 4];
    const u32 t = threadIdx.x;
    const qm31 *__restrict__ in = partials + (size_t)blockIdx.y * chunks;
    const u32 blocks = (chunks + kMleFoldBlock - 1) / kMleFoldBlock;
    const qm31 zero = {0u, 0u, 0u, 0u};
    qm31 x = t < chunks ? in[t] : zero;
    mle_build_tables(tab, F, 0);
    mle_build_tables(tab + 32, F2, 32);
    __syncthreads();
    const qm31 ft = qm31_mul(tab[t & 15], tab[16 + (t >> 4)]);
    qm31 acc = zero;
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        const u32 qn = (b + 1) * kMleFoldBlock + t;
        const qm31 nx = qn < chunks ? in[qn] : zero;          // the next block's load flies while this one is multiplied
        const qm31 bf = qm31_mul(tab[32 + (b & 15)], tab[48 + (b >> 4)]);
        acc = qm31_add(acc, qm31_mul(x, bf));
        x = nx;
    }
    qm31 v = qm31_mul(acc, ft);
    v = eval_wg_sum(v, tab + 64);
    if (t == 0) out[blockIdx.y] = v;
}

int bad(const std::string &msg) { return set_error(TSTWO_ERR_BAD_ARG, "mle eval_at_point: " + msg); }

template <bool SECURE>
void launch_first(const MleEvalPlan &p, const ColPtrs &cp, u32 n_vals, const MleW &W, const MleF &F, const MleH &H, qm31 *out, u32 stride) {
    const dim3 grid(p.chunks, p.grid_y), wg(256);
    hipStream_t s = ctx().stream;
    if (SECURE || p.groups == 4) {
        if (p.fast) hipLaunchKernelGGL((k_mle_first<SECURE, true, 4>), grid, wg, 0, s, cp, n_vals, W, F, H, out, stride);
        else hipLaunchKernelGGL((k_mle_first<SECURE, false, 4>), grid, wg, 0, s, cp, n_vals, W, F, H, out, stride);
    } else {
        if (p.fast) hipLaunchKernelGGL((k_mle_first<false, true, 1>), grid, wg, 0, s, cp, n_vals, W, F, H, out, stride);
        else hipLaunchKernelGGL((k_mle_first<false, false, 1>), grid, wg, 0, s, cp, n_vals, W, F, H, out, stride);
    }
}

// cols: n_mles columns (base) or 4 n_mles (secure: MLE k = cols[4k .. 4k + 4)).  Every check comes before the first enqueue.
int mle_eval_at_point(const u32 *const *cols, size_t n_mles, u32 log_n, const u32 *point, u32 *out, bool secure) {
    if (n_mles == 0) return bad("no MLE given");
    if (log_n > kMleEvalMaxLog) return bad("more than 28 variables");
    if (n_mles > kMleEvalMaxMles) return bad("more than 32768 MLEs in one call");
    if (!cols || !out || (log_n && !point)) return bad("null argument");
    const size_t n_cols = secure ? 4 * n_mles : n_mles;
    bool aligned = true;
    for (size_t i = 0; i < n_cols; i++) {
        if (!cols[i]) return bad("null device pointer in table");
        aligned = aligned && aligned16(cols[i]);
    }
    for (u32 k = 0; k < 4 * log_n; k++)
        if (point[k] >= M31_P) return bad("point word out of range");
    if (stream_is_capturing()) return bad("host read-back during graph capture (the values cannot be recorded)");
    MleEvalPlan p;
    if (const char *why = mle_eval_plan(log_n, n_mles, secure, aligned, p)) return bad(why);

    // fac[s]: the point's coordinate for index bit s (variable n - 1 - s); zero for a bit the MLE does not have
    const host::Q one = {{1, 0, 0, 0}}, zero = {{0, 0, 0, 0}};
    host::Q fac[kMleEvalMaxLog + 16];
    for (u32 s = 0; s < kMleEvalMaxLog + 16; s++) fac[s] = s < log_n ? to_hq(point + 4 * (log_n - 1 - s)) : zero;
    auto pick = [&](u32 s, u32 bit) { return bit ? fac[s] : host::qsub(one, fac[s]); };
    MleW W;
    MleF F, F2;
    MleH H;
    const u32 wbits[4] = {0, 1, 10, 11};
    for (u32 e = 0; e < 16; e++) {
        host::Q v = one;
        for (int i = 0; i < 4; i++) v = host::qmul(v, pick(wbits[i], (e >> i) & 1));
        W.w[e] = to_q(v);
    }
    for (u32 g = 0; g < 4; g++) H.h[g] = to_q(host::qmul(pick(12, g & 1), pick(13, g >> 1)));
    for (u32 i = 0; i < 8; i++) F.p[i] = to_q(fac[2 + i]);

    if (int rc = ensure_scratch((p.scratch_qm31 + 8) * sizeof(qm31))) return rc;
    Context &c = ctx();
    qm31 *partials = (qm31 *)c.scratch, *results = partials + (p.scratch_qm31 - n_mles);
    // the last pass stores its results straight into the page-locked host buffer (device-visible): the call then ends with one
    // stream synchronisation instead of a copy + synchronisation
    qm31 *host_dst = (c.pinned && n_mles * sizeof(qm31) <= kPinnedBytes) ? (qm31 *)c.pinned : nullptr;
    qm31 *dst = host_dst ? host_dst : results;
    ColPtrs cp;
    if (int rc = fill_col_table(cp, cols, n_cols, 0)) return rc;
    const u32 n_vals = 1u << log_n;
    qm31 *o1 = p.passes == 1 ? dst : partials;
    const u32 stride = p.passes == 1 ? 1u : p.chunks;
    if (secure) launch_first<true>(p, cp, n_vals, W, F, H, o1, stride);
    else launch_first<false>(p, cp, n_vals, W, F, H, o1, stride);
    if (p.passes == 2) {
        for (u32 i = 0; i < 8; i++) { F.p[i] = to_q(fac[p.chunk_log + i]); F2.p[i] = to_q(fac[p.chunk_log + 8 + i]); }
        hipLaunchKernelGGL(k_mle_partials, dim3(1, p.grid_y), dim3(256), 0, c.stream, (const qm31 *)partials, p.chunks, F, F2, dst);
    }
    TSTWO_LAUNCH_CHECK();
    if (host_dst) {
        if (int rc = wait_stream()) return rc;
        memcpy(out, host_dst, n_mles * sizeof(qm31));
        return TSTWO_OK;
    }
    return small_d2h(out, results, n_mles * sizeof(qm31));
}

}  // namespace

extern "C" {

int tstwo_mle_eval_at_point_base(const u32 *const *mles, size_t n_mles, u32 log_n, const u32 *point, u32 *out) {
    TSTWO_REQUIRE_READY();
    return mle_eval_at_point(mles, n_mles, log_n, point, out, false);
}

int tstwo_mle_eval_at_point_secure(const u32 *const *cols, size_t n_mles, u32 log_n, const u32 *point, u32 *out) {
    TSTWO_REQUIRE_READY();
    return mle_eval_at_point(cols, n_mles, log_n, point, out, true);
}

}  // extern "C"

// gkr.hip — GkrOps / MleOps of the reference (backend/cpu/lookups/gkr.ts:84-358, backend/cpu/lookups/mle.ts:60-130) on
// multilinear extensions held as SoA QM31 columns (4 u32 columns, SecureColumnByCoords layout) or one M31 column.
//
// Index order: the first variable is the most significant bit of the index, so fix_first_variable pairs i with i + n/2 and
// next_layer pairs 2i with 2i + 1.  Every op is a streaming pass over 2^n values:
//   eq table        k_eq_tables (two tables of 2^(n/2) entries) + k_eq_expand (one QM31 product per output: HBM writes)
//   next_layer      k_next_layer<KIND>: pairwise product or fraction addition, nothing is inverted
//   fold            k_fold<BASE>: out[i] = lhs[i] + r (rhs[i] - lhs[i]); the secure form may run in place
//   sums            k_sum<KIND, FOLD>: (f(0), f(2)) of the round polynomial, block partials + a last-block ticket (one launch).
//                   FOLD = the fused sumcheck round of prove_batch: the layer is first folded by the previous round's challenge
//                   (written back, in place for secure columns) and the sum is taken over the folded values.
//                   Fold and FOLD take their challenge by value or from 4 device words an earlier launch wrote (the _dev entries).
//   round finish    k_gkr_round_finish: the O(instances) end of a sum-check round by one wave — round polynomials, combination,
//                   Blake2s channel mix + draw, new claims — so that a layer of prove_batch is enqueued without a read-back.
//   one-call proof  tstwo_gkr_prove_batch: the schedule of gkr_plan.h with every protocol scalar left in device words — the _dev /
//                   _ldev forms of the kernels above read y, v, lambda, inv_eq0 and alpha from memory, and two single-wave
//                   transcript kernels (k_gkr_layer_begin, k_gkr_layer_end) do what the host does around a layer's sum-check — so
//                   that the whole proof is enqueued without a read-back and one block comes back at the end.
// M31 addition is exact, so the reduction order does not change a bit of the result.
#include <vector>

#include "common.h"
#include "blake2s.cuh"
#include "gkr_plan.h"

using namespace tstwo;

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxSumBlocks = 1024;     // slab = kMaxSumBlocks x 8 words
constexpr u32 kMaxLog = 28;                  // word offsets of gload*/gstore* stay below 2^30
// gkr scratch layout (context scratch, >= 1 MiB): ticket word | result words (no result page) | slab | eq tables
constexpr size_t kTicketOff = 0, kResultOff = 256, kSlabOff = 1024, kTabOff = kSlabOff + kMaxSumBlocks * 8 * 4;

unsigned grid_for(size_t work, unsigned cap_per_cu) {
    unsigned b = ceil_div(work, kThreads);
    unsigned cap = (unsigned)ctx().n_cus * cap_per_cu;
    if (b > cap) b = cap;
    return b ? b : 1;
}
template <class T>
bool all_aligned16(const T &s) {
    for (int k = 0; k < 4; k++) if (!aligned16(s.p[k])) return false;
    return true;
}

struct EqY { qm31 y[kMaxLog]; };

__device__ __forceinline__ qm31 ld_q(const CSoa4 &c, u32 i) { return {gload1(c.p[0], i), gload1(c.p[1], i), gload1(c.p[2], i), gload1(c.p[3], i)}; }
__device__ __forceinline__ void st_q(const Soa4 &c, u32 i, qm31 v) {
    gstore1(c.p[0], i, v.a); gstore1(c.p[1], i, v.b); gstore1(c.p[2], i, v.c); gstore1(c.p[3], i, v.d);
}
__device__ __forceinline__ qm31 q_double(qm31 x) { return qm31_add(x, x); }
// foldMleEvals (lookups/utils.ts:256): eval0 + r (eval1 - eval0)
__device__ __forceinline__ qm31 fold_q(qm31 r, qm31 lhs, qm31 rhs) { return qm31_add(lhs, qm31_mul(r, qm31_sub(rhs, lhs))); }
__device__ __forceinline__ qm31 fold_b(qm31 r, u32 lhs, u32 rhs) {
    qm31 t = qm31_mul_m31(r, m31_sub(rhs, lhs));
    t.a = m31_add(t.a, lhs);
    return t;
}

// ---------------------------------------------------------------- eq table (gkr.ts:90-104)
// out[x] = v * prod_k eq(bit_k(x), y[k]), bit 0 of that product = the MOST significant bit of x.  hi = the first n - lo variables
// (high bits of x), lo = the last lo variables.  tab[0 .. 2^hi) = v * eq(high bits, y[0..hi)), tab[2^hi .. 2^hi + 2^lo) =
// eq(low bits, y[hi..n)).  eq(0, y) = 1 - y, eq(1, y) = y.
__global__ void __launch_bounds__(kThreads) k_eq_tables(EqY y, qm31 v, u32 hi, u32 lo, qm31 *tab) {
    const u32 t = blockIdx.x * kThreads + threadIdx.x;
    const u32 nh = 1u << hi, nl = 1u << lo;
    if (t >= nh + nl) return;
    const bool high = t < nh;
    const u32 idx = high ? t : t - nh, nb = high ? hi : lo, y0 = high ? 0 : hi;
    qm31 acc = high ? v : qm31{1u, 0u, 0u, 0u};
    const qm31 one = {1u, 0u, 0u, 0u};
#pragma unroll 1
    for (u32 k = 0; k < nb; k++) {
        const qm31 yk = y.y[y0 + k];
        acc = qm31_mul(acc, ((idx >> (nb - 1 - k)) & 1u) ? yk : qm31_sub(one, yk));
    }
    tab[t] = acc;
}
// The same with the point (4 hi + 4 lo words) and v (4 words) in device memory, left there by an earlier launch on the stream
// (tstwo_gkr_layer_end / _begin).  Lane t reads y[y0 + k] for k = 0 .. nb: one address per wave wherever a wave lies within one of
// the two tables (always from 2^6 high entries on), so the loads are broadcasts out of one cache line.
__global__ void __launch_bounds__(kThreads) k_eq_tables_dev(const u32 *__restrict__ y, const u32 *__restrict__ v, u32 hi, u32 lo, qm31 *tab) {
    const u32 t = blockIdx.x * kThreads + threadIdx.x;
    const u32 nh = 1u << hi, nl = 1u << lo;
    if (t >= nh + nl) return;
    const bool high = t < nh;
    const u32 idx = high ? t : t - nh, nb = high ? hi : lo, y0 = high ? 0 : hi;
    const qm31 one = {1u, 0u, 0u, 0u};
    qm31 acc = one;
    if (high) { const uint4 w = gload4(v); acc = {w.x, w.y, w.z, w.w}; }
#pragma unroll 1
    for (u32 k = 0; k < nb; k++) {
        const uint4 w = gload4(y, 4 * (y0 + k));
        const qm31 yk = {w.x, w.y, w.z, w.w};
        acc = qm31_mul(acc, ((idx >> (nb - 1 - k)) & 1u) ? yk : qm31_sub(one, yk));
    }
    tab[t] = acc;
}
// W consecutive outputs per lane (W = 4: 16-byte stores; lo >= 2 so the W outputs share one high-table entry)
template <int W>
__global__ void __launch_bounds__(kThreads) k_eq_expand(const qm31 *__restrict__ tab, u32 hi, u32 lo, Soa4 out) {
    const u32 n = 1u << (hi + lo), nh = 1u << hi, lmask = (1u << lo) - 1;
    const u32 stride = gridDim.x * kThreads;
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < n / W; t += stride) {
        const u32 x = t * W;
        const qm31 h = tab[x >> lo];
        if (W == 4) {
            qm31 r[4];
#pragma unroll
            for (int e = 0; e < 4; e++) r[e] = qm31_mul(h, tab[nh + ((x + e) & lmask)]);
            gstore4(out.p[0], x, make_uint4(r[0].a, r[1].a, r[2].a, r[3].a));
            gstore4(out.p[1], x, make_uint4(r[0].b, r[1].b, r[2].b, r[3].b));
            gstore4(out.p[2], x, make_uint4(r[0].c, r[1].c, r[2].c, r[3].c));
            gstore4(out.p[3], x, make_uint4(r[0].d, r[1].d, r[2].d, r[3].d));
        } else {
            st_q(out, x, qm31_mul(h, tab[nh + (x & lmask)]));
        }
    }
}

// ---------------------------------------------------------------- next_layer (gkr.ts:109-137, 317-358)
// KIND: the input layer's kind (TSTWO_GKR_GRAND_PRODUCT: `den` is the product column, `num` unused).  Output i from inputs
// 2i, 2i+1.  Fraction addition: (n0 d1 + n1 d0, d0 d1); LogUpSingles numerators are 1: (d0 + d1, d0 d1).
template <int KIND>
__device__ __forceinline__ void next_one(const CSoa4 &num, const CSoa4 &den, u32 i, qm31 &on, qm31 &od) {
    const qm31 d0 = ld_q(den, 2 * i), d1 = ld_q(den, 2 * i + 1);
    od = qm31_mul(d0, d1);
    if (KIND == TSTWO_GKR_LOGUP_GENERIC) {
        on = qm31_add(qm31_mul(ld_q(num, 2 * i), d1), qm31_mul(ld_q(num, 2 * i + 1), d0));
    } else if (KIND == TSTWO_GKR_LOGUP_MULTIPLICITIES) {
        on = qm31_add(qm31_mul_m31(d1, gload1(num.p[0], 2 * i)), qm31_mul_m31(d0, gload1(num.p[0], 2 * i + 1)));
    } else if (KIND == TSTWO_GKR_LOGUP_SINGLES) {
        on = qm31_add(d0, d1);
    }
}
template <int KIND>
__global__ void __launch_bounds__(kThreads) k_next_layer(CSoa4 num, CSoa4 den, Soa4 onum, Soa4 oden, u32 n_out) {
    const u32 stride = gridDim.x * kThreads;
    for (u32 i = blockIdx.x * kThreads + threadIdx.x; i < n_out; i += stride) {
        qm31 on, od;
        next_one<KIND>(num, den, i, on, od);
        st_q(oden, i, od);
        if (KIND != TSTWO_GKR_GRAND_PRODUCT) st_q(onum, i, on);
    }
}

// A QM31 that an earlier launch on the stream left in device memory (16-byte aligned), the same for every lane: one load, then
// scalar registers, so a kernel that takes its challenge this way keeps the register budget of the by-value form.
__device__ __forceinline__ qm31 ld_uniform_q(const u32 *p) {
    const uint4 v = gload4(p);
    return {(u32)__builtin_amdgcn_readfirstlane((int)v.x), (u32)__builtin_amdgcn_readfirstlane((int)v.y),
            (u32)__builtin_amdgcn_readfirstlane((int)v.z), (u32)__builtin_amdgcn_readfirstlane((int)v.w)};
}

// ---------------------------------------------------------------- fix_first_variable (mle.ts:68-130)
// out[i] = in[i] + r (in[i + half] - in[i]); W = 4: 16-byte accesses.  In place (out == in) is safe: lane i reads i and
// i + half and writes i only.
template <bool BASE, int W>
__global__ void __launch_bounds__(kThreads) k_fold(CSoa4 in, qm31 r, const u32 *__restrict__ r_dev, Soa4 out, u32 half) {
    if (r_dev) r = ld_uniform_q(r_dev);         // the challenge an earlier launch drew (tstwo_gkr_round_finish)
    const u32 stride = gridDim.x * kThreads;
    for (u32 t = blockIdx.x * kThreads + threadIdx.x; t < half / W; t += stride) {
        const u32 i = t * W;
        if (W == 4) {
            qm31 v[4];
            if (BASE) {
                const uint4 l = gload4(in.p[0], i), h = gload4(in.p[0], i + half);
                v[0] = fold_b(r, l.x, h.x); v[1] = fold_b(r, l.y, h.y); v[2] = fold_b(r, l.z, h.z); v[3] = fold_b(r, l.w, h.w);
            } else {
                uint4 l[4], h[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { l[k] = gload4(in.p[k], i); h[k] = gload4(in.p[k], i + half); }
                v[0] = fold_q(r, {l[0].x, l[1].x, l[2].x, l[3].x}, {h[0].x, h[1].x, h[2].x, h[3].x});
                v[1] = fold_q(r, {l[0].y, l[1].y, l[2].y, l[3].y}, {h[0].y, h[1].y, h[2].y, h[3].y});
                v[2] = fold_q(r, {l[0].z, l[1].z, l[2].z, l[3].z}, {h[0].z, h[1].z, h[2].z, h[3].z});
                v[3] = fold_q(r, {l[0].w, l[1].w, l[2].w, l[3].w}, {h[0].w, h[1].w, h[2].w, h[3].w});
            }
            gstore4(out.p[0], i, make_uint4(v[0].a, v[1].a, v[2].a, v[3].a));
            gstore4(out.p[1], i, make_uint4(v[0].b, v[1].b, v[2].b, v[3].b));
            gstore4(out.p[2], i, make_uint4(v[0].c, v[1].c, v[2].c, v[3].c));
            gstore4(out.p[3], i, make_uint4(v[0].d, v[1].d, v[2].d, v[3].d));
        } else {
            const qm31 v = BASE ? fold_b(r, gload1(in.p[0], i), gload1(in.p[0], i + half)) : fold_q(r, ld_q(in, i), ld_q(in, i + half));
            st_q(out, i, v);
        }
    }
}

// ---------------------------------------------------------------- sum_as_poly_in_first_variable (gkr.ts:142-311)
// Term i (i < n_terms) reads the layer at 2i, 2i+1 (t = 0 half) and 2(n_terms + i), 2(n_terms + i) + 1 (t = 1 half) and
// eq_evals[i]; the value at t = 2 of a column is 2 x(1) - x(0).
//   grand product: eq (x0 x1)
//   LogUp:         eq (n0 d1 + n1 d0 + lambda d0 d1)           (singles: n = 1)
// FOLD: the layer passed is the one BEFORE fixing its first variable to r (2x the entries); each lane folds the 4 positions it
// reads (position p from p and p + 4 n_terms of the unfolded layer), writes them to the output columns and sums them.
struct SumArgs {
    CSoa4 eq;
    CSoa4 num, den;      // GP: den = the product column
    Soa4 onum, oden;     // FOLD: where the folded layer goes (may alias num / den for secure columns)
    qm31 lambda, r;
    const u32 *r_dev;    // FOLD: non-null = r is read from these 4 device words instead (tstwo_gkr_round_dev)
    u32 n_terms;
    u32 *slab, *ticket, *out;
};

template <int KIND, bool FOLD>
__device__ __forceinline__ qm31 num_at(const SumArgs &a, u32 p) {
    if (KIND == TSTWO_GKR_LOGUP_SINGLES || KIND == TSTWO_GKR_GRAND_PRODUCT) return qm31{1u, 0u, 0u, 0u};
    const u32 full = 4 * a.n_terms;    // folded-layer length
    if (KIND == TSTWO_GKR_LOGUP_MULTIPLICITIES) {
        if (FOLD) {
            const qm31 v = fold_b(a.r, gload1(a.num.p[0], p), gload1(a.num.p[0], p + full));
            st_q(a.onum, p, v);
            return v;
        }
        return qm31_from_m31(gload1(a.num.p[0], p));
    }
    if (FOLD) {
        const qm31 v = fold_q(a.r, ld_q(a.num, p), ld_q(a.num, p + full));
        st_q(a.onum, p, v);
        return v;
    }
    return ld_q(a.num, p);
}
template <bool FOLD>
__device__ __forceinline__ qm31 den_at(const SumArgs &a, u32 p) {
    if (FOLD) {
        const qm31 v = fold_q(a.r, ld_q(a.den, p), ld_q(a.den, p + 4 * a.n_terms));
        st_q(a.oden, p, v);
        return v;
    }
    return ld_q(a.den, p);
}
template <int KIND>
__device__ __forceinline__ qm31 gate(const SumArgs &a, qm31 n0, qm31 d0, qm31 n1, qm31 d1) {
    if (KIND == TSTWO_GKR_GRAND_PRODUCT) return qm31_mul(d0, d1);
    const qm31 dd = qm31_mul(d0, d1);
    qm31 nn;
    if (KIND == TSTWO_GKR_LOGUP_SINGLES) nn = qm31_add(d0, d1);
    else nn = qm31_add(qm31_mul(n0, d1), qm31_mul(n1, d0));
    return qm31_add(nn, qm31_mul(a.lambda, dd));
}

__device__ __forceinline__ void wave_sum8(u32 (&v)[8]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = m31_add(v[k], (u32)__shfl_xor((int)v[k], off, 64));
}

template <int KIND, bool FOLD>
__global__ void __launch_bounds__(kThreads) k_sum(SumArgs a) {
#include "gkr_sum_body.inc"
}
// The same with lambda left in device memory by an earlier launch (tstwo_gkr_layer_begin): one load, then scalar registers.  The
// pointer is a kernel parameter of its own: SumArgs, and with it the argument segment and the code of k_sum, stay as they were.
template <int KIND, bool FOLD>
__global__ void __launch_bounds__(kThreads) k_sum_ldev(SumArgs a, const u32 *lambda_dev) {
    a.lambda = ld_uniform_q(lambda_dev);
#include "gkr_sum_body.inc"
}

template <int KIND>
int launch_sum_kind(const SumArgs &a, const u32 *lambda_dev, bool fold, unsigned grid) {
    const dim3 g(grid), b(kThreads);
    if constexpr (KIND != TSTWO_GKR_GRAND_PRODUCT) {                    // a grand product has no lambda
        if (lambda_dev) {
            if (fold) hipLaunchKernelGGL((k_sum_ldev<KIND, true>), g, b, 0, ctx().stream, a, lambda_dev);
            else hipLaunchKernelGGL((k_sum_ldev<KIND, false>), g, b, 0, ctx().stream, a, lambda_dev);
            TSTWO_LAUNCH_CHECK();
            return TSTWO_OK;
        }
    }
    if (fold) hipLaunchKernelGGL((k_sum<KIND, true>), g, b, 0, ctx().stream, a);
    else hipLaunchKernelGGL((k_sum<KIND, false>), g, b, 0, ctx().stream, a);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

bool valid_kind(u32 kind) { return kind <= TSTWO_GKR_LOGUP_SINGLES; }
qm31 qarg(const u32 v[4]) { return {v[0], v[1], v[2], v[3]}; }
CSoa4 csoa(const u32 *const c[4]) { return {{c[0], c[1], c[2], c[3]}}; }
Soa4 soa(u32 *const c[4]) { return {{c[0], c[1], c[2], c[3]}}; }
CSoa4 csoa1(const u32 *c) { return {{c, c, c, c}}; }

// Checks and launches one sum (fold: the fused round); `out` = 8 device-visible words.
// The fold's challenge is r (host words) or, when r_dev is given, 4 words of device memory written earlier on the stream; lambda
// likewise: host words, or (lambda null) the 4 device words at lambda_dev.
int gkr_sum(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const onum[4],
            u32 *const oden[4], u32 n_vars, const u32 r[4], const u32 *r_dev, const u32 lambda[4], u32 *out, bool fold,
            const u32 *lambda_dev = nullptr) {
    if (!valid_kind(kind)) return set_error(TSTWO_ERR_BAD_ARG, "unknown GKR layer kind");
    if (n_vars == 0) return set_error(TSTWO_ERR_ZERO_VARIABLES, "Number of variables must not be zero");
    if (n_vars + 1 + (fold ? 1 : 0) > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "GKR layer too large");
    TSTWO_REQUIRE_TABLE(eq, 4); TSTWO_REQUIRE_TABLE(den, 4);
    if (!lambda && !lambda_dev) return set_error(TSTWO_ERR_BAD_ARG, "null lambda");
    if (!lambda && !aligned16(lambda_dev)) return set_error(TSTWO_ERR_BAD_ARG, "device lambda is not 16-byte aligned");
    SumArgs a{};
    a.eq = csoa(eq);
    a.den = csoa(den);
    a.n_terms = 1u << (n_vars - 1);
    if (lambda) { a.lambda = qarg(lambda); lambda_dev = nullptr; }
    if (kind == TSTWO_GKR_LOGUP_GENERIC) { TSTWO_REQUIRE_TABLE(num, 4); a.num = csoa(num); }
    if (kind == TSTWO_GKR_LOGUP_MULTIPLICITIES) { TSTWO_REQUIRE_TABLE(num, 1); a.num = csoa1(num[0]); }
    if (fold) {
        if (!r && !r_dev) return set_error(TSTWO_ERR_BAD_ARG, "null challenge");
        if (!aligned16(r_dev)) return set_error(TSTWO_ERR_BAD_ARG, "device challenge is not 16-byte aligned");
        if (r) a.r = qarg(r);
        a.r_dev = r ? nullptr : r_dev;
        TSTWO_REQUIRE_TABLE(oden, 4);
        a.oden = soa(oden);
        if (kind == TSTWO_GKR_LOGUP_GENERIC || kind == TSTWO_GKR_LOGUP_MULTIPLICITIES) { TSTWO_REQUIRE_TABLE(onum, 4); a.onum = soa(onum); }
        if (kind == TSTWO_GKR_LOGUP_MULTIPLICITIES)
            for (int k = 0; k < 4; k++)
                if ((const void *)onum[k] == (const void *)num[0]) return set_error(TSTWO_ERR_BAD_ARG, "base numerators cannot be folded in place");
    }
    if (int rc = ensure_scratch(kTabOff)) return rc;
    uint8_t *const s = (uint8_t *)ctx().scratch;
    a.ticket = (u32 *)(s + kTicketOff);
    a.slab = (u32 *)(s + kSlabOff);
    a.out = out;
    const unsigned grid = grid_for(a.n_terms, 4) < kMaxSumBlocks ? grid_for(a.n_terms, 4) : kMaxSumBlocks;
    TSTWO_HIP(hipMemsetAsync(a.ticket, 0, 4, ctx().stream));
    switch (kind) {
        case TSTWO_GKR_GRAND_PRODUCT: return launch_sum_kind<TSTWO_GKR_GRAND_PRODUCT>(a, lambda_dev, fold, grid);
        case TSTWO_GKR_LOGUP_GENERIC: return launch_sum_kind<TSTWO_GKR_LOGUP_GENERIC>(a, lambda_dev, fold, grid);
        case TSTWO_GKR_LOGUP_MULTIPLICITIES: return launch_sum_kind<TSTWO_GKR_LOGUP_MULTIPLICITIES>(a, lambda_dev, fold, grid);
        default: return launch_sum_kind<TSTWO_GKR_LOGUP_SINGLES>(a, lambda_dev, fold, grid);
    }
}

// Checks and launches one fold; base: in[0] is the one M31 column.  The challenge is r (host words) or, when r is null, the 4
// device words at r_dev.
int mle_fold(bool base, const u32 *const in[4], u32 log_n, const u32 r[4], const u32 *r_dev, u32 *const out[4]) {
    if (log_n == 0) return TSTWO_OK;                 // a constant: midpoint 0, nothing to write (mle.ts:68-80)
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "MLE too large");
    if (!r && !r_dev) return set_error(TSTWO_ERR_BAD_ARG, "null assignment");
    if (!r && !aligned16(r_dev)) return set_error(TSTWO_ERR_BAD_ARG, "device challenge is not 16-byte aligned");
    if (base) TSTWO_REQUIRE_PTRS(in[0]);
    else TSTWO_REQUIRE_TABLE(in, 4);
    TSTWO_REQUIRE_TABLE(out, 4);
    const u32 half = 1u << (log_n - 1);
    const CSoa4 i4 = csoa(in);
    const Soa4 o = soa(out);
    const qm31 rv = r ? qarg(r) : qm31{0u, 0u, 0u, 0u};
    const u32 *rd = r ? nullptr : r_dev;
    const bool wide = half % 4 == 0 && all_aligned16(i4) && all_aligned16(o);
    const dim3 g(wide ? grid_for(half / 4, 32) : grid_for(half, 32)), b(kThreads);
    if (base && wide) hipLaunchKernelGGL((k_fold<true, 4>), g, b, 0, ctx().stream, i4, rv, rd, o, half);
    else if (base) hipLaunchKernelGGL((k_fold<true, 1>), g, b, 0, ctx().stream, i4, rv, rd, o, half);
    else if (wide) hipLaunchKernelGGL((k_fold<false, 4>), g, b, 0, ctx().stream, i4, rv, rd, o, half);
    else hipLaunchKernelGGL((k_fold<false, 1>), g, b, 0, ctx().stream, i4, rv, rd, o, half);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// ---------------------------------------------------------------- the end of a sum-check round (gkr_prover.ts:609-660, sumcheck.ts:99-227)
// Everything prove_batch's host loop does between the sums of one round and the launches of the next, by ONE wave: lane i owns
// instance i (its claim, its eq correction, its round polynomial p_i); the combined polynomial, the channel and the challenge are
// wave-uniform.
//
// An active instance's p_i is the cubic through (0, r0), (1, r1), (2, r2), (b, 0) with r0 = f0 c (1 - y) a, r1 = claim - r0,
// r2 = f2 c (3y - 1) a, b = (1 - y) / (1 - 2y) (c = the instance's correction, a = inv_eq0, y = y_k).  Written as
// p_i(x) = (x - b) (w0 (x-1)(x-2) + w1 x(x-2) + w2 x(x-1)) the Lagrange weights are w0 = r0 / (-2b), w1 = -r1 / (1 - b),
// w2 = r2 / (2 (2 - b)); with D = 1 - 2y: 1/b = D / (1 - y), 1/(1 - b) = -D / y, 1/(2 - b) = D / (1 - 3y), so the factors
// (1 - y) and (3y - 1) of r0 and r2 cancel and, with g0 = f0 c a D and g2 = f2 c a D,
//     w0 = -g0 / 2,   w1 = (claim D - g0 (1 - y)) / y,   w2 = -g2 / 2.
// Only y and D are inverted — wave-uniform, one qm31_inv for both (Montgomery) — and nothing per instance.  The field is exact, so
// the coefficients are the host path's bit for bit.  The entry point refuses the y for which the host path divides by zero.
struct FinishArgs {
    u32 *chan;
    const u32 *sums;
    u32 *state;
    u32 n;
    u64 mask;
    qm31 y, a, alpha;
    u32 *poly_out, *ch_out;
};
// k_gkr_round_finish_dev: y, a and alpha are read from 4 device words each; a degenerate y is reported in *status.  A parameter of
// its own, so that FinishArgs, the argument segment and the code of k_gkr_round_finish stay as they were.
struct FinishDev {
    const u32 *y, *a, *alpha;
    u32 *status;
};
constexpr u32 kStatusDegenerate = 1u;        // the status word: an eq point at which the host path divides by zero
__device__ __forceinline__ bool q_eq_m31(qm31 v, u32 a) { return v.a == a && (v.b | v.c | v.d) == 0u; }
// y = 1/2: b is undefined; y = 1, 0, 1/3: b = 0, 1, 2 collides with an interpolation point
__device__ __forceinline__ bool degenerate_y(qm31 y) { return q_eq_m31(y, 0u) || q_eq_m31(y, 1u) || q_eq_m31(y, 1u << 30) || q_eq_m31(y, 0x55555555u); }
__device__ __forceinline__ qm31 q_of(uint4 v) { return {v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ uint4 u4_of(qm31 v) { return make_uint4(v.a, v.b, v.c, v.d); }

__global__ void __launch_bounds__(64) k_gkr_round_finish(FinishArgs f) {
#include "gkr_finish_body.inc"
}
__global__ void __launch_bounds__(64) k_gkr_round_finish_dev(FinishArgs f, FinishDev dev) {
    f.y = ld_uniform_q(dev.y); f.a = ld_uniform_q(dev.a); f.alpha = ld_uniform_q(dev.alpha);
    // the round still finishes (every loop of the body is bounded and the inversion is a fixed power chain); its outputs mean nothing
    if (threadIdx.x == 0 && degenerate_y(f.y)) __hip_atomic_fetch_or(dev.status, kStatusDegenerate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#include "gkr_finish_body.inc"
}

// ---------------------------------------------------------------- the top and the bottom of a layer (gkr_prover.ts:452-500, 540-575)
// What prove_batch's host loop does around a layer's sum-check, by ONE wave each: lane j owns the j-th active instance (a
// tstwo_gkr_lane in device memory); the channel is wave-uniform.  The mixes of a layer are a serial hash chain by the definition
// of the transcript: lane j's felts are broadcast and every lane runs the same compression, as k_gkr_round_finish does.
typedef const TSTWO_GLOBAL tstwo_gkr_lane *lane_ptr;
__device__ __forceinline__ qm31 bcast_q(qm31 v, u32 j) {
    return {(u32)__shfl((int)v.a, (int)j, 64), (u32)__shfl((int)v.b, (int)j, 64), (u32)__shfl((int)v.c, (int)j, 64), (u32)__shfl((int)v.d, (int)j, 64)};
}
// mix_felts (channel/blake2.ts:113-118) of the first n_felts (1 .. 4) of f: Blake2s over digest || 16 n_felts bytes.  The felts
// beyond n_felts are zero, which is the padding of the last block.  FOUR = false: at most 2 felts, always one compression.
template <bool FOUR>
__device__ __forceinline__ void chan_mix_felts(u32 (&d)[8], u32 &n_chal, u32 &n_sent, const qm31 (&f)[4], u32 n_felts) {
    using namespace b2s;
    u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
    u32 m[16];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = d[k];
    m[8] = f[0].a; m[9] = f[0].b; m[10] = f[0].c; m[11] = f[0].d; m[12] = f[1].a; m[13] = f[1].b; m[14] = f[1].c; m[15] = f[1].d;
    const u32 len = 32u + 16u * n_felts;
    if (!FOUR || n_felts <= 2) {
        b2s_compress(h, m, len, true);
    } else {
        b2s_compress(h, m, 64u, false);
        m[0] = f[2].a; m[1] = f[2].b; m[2] = f[2].c; m[3] = f[2].d; m[4] = f[3].a; m[5] = f[3].b; m[6] = f[3].c; m[7] = f[3].d;
#pragma unroll
        for (int k = 8; k < 16; k++) m[k] = 0u;
        b2s_compress(h, m, len, true);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = h[k];
    n_chal += 1;
    n_sent = 0;
}
__device__ __forceinline__ qm31 ld_col0(const u32 *const *c, int first, u32 word) {
    return {gload1(c[first], word), gload1(c[first + 1], word), gload1(c[first + 2], word), gload1(c[first + 3], word)};
}
__device__ __forceinline__ void load_lane_ptrs(const u32 *const TSTWO_GLOBAL *p, const u32 *(&out)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = p[k];
}

struct BeginArgs {
    u32 *chan;
    const tstwo_gkr_lane *lanes;
    u32 n;
    const u32 *claims;
    u32 *out_claims, *state, *scalars;
    const u32 *y;
    u32 n_y;
    u32 *inv, *status;
};
__global__ void __launch_bounds__(64) k_gkr_layer_begin(BeginArgs t) {
    using namespace b2s;
    const u32 lane = threadIdx.x;
    const bool in = lane < t.n;
    const qm31 zero = {0u, 0u, 0u, 0u}, one = {1u, 0u, 0u, 0u};
    u32 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = gload1(t.chan, k);
    u32 n_chal = gload1(t.chan, 8), n_sent = gload1(t.chan, 9);
    // lane j: its claims to verify — the output values where it enters, else what the layer below left
    qm31 c0 = zero, c1 = zero;
    u32 n_felts = 0, shift = 0;
    if (in) {
        const lane_ptr me = (lane_ptr)t.lanes + lane;
        const u32 inst = me->inst;
        const bool gp = me->kind == TSTWO_GKR_GRAND_PRODUCT;
        n_felts = gp ? 1u : 2u;
        shift = me->shift;
        if (me->enter) {
            const u32 *src[8];
            load_lane_ptrs(me->out_src, src);
            const qm31 den = {gload1(src[4]), gload1(src[5]), gload1(src[6]), gload1(src[7])};
            if (gp) {
                c0 = den;
            } else {
                c0 = {gload1(src[0]), gload1(src[1]), gload1(src[2]), gload1(src[3])};
                c1 = den;
            }
            gstore4(t.out_claims, 8 * inst, u4_of(c0));
            gstore4(t.out_claims, 8 * inst + 4, u4_of(c1));
        } else {
            c0 = q_of(gload4(t.claims, 8 * inst));
            c1 = q_of(gload4(t.claims, 8 * inst + 4));
        }
    }
    // one mix per lane, in lane order
#pragma unroll 1
    for (u32 j = 0; j < t.n; j++) {
        const qm31 f[4] = {bcast_q(c0, j), bcast_q(c1, j), zero, zero};
        const u32 nf = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)n_felts, (int)j, 64));
        chan_mix_felts<false>(d, n_chal, n_sent, f, nf);
    }
    u32 fa[4] = {0u, 0u, 0u, 0u}, fl[4] = {0u, 0u, 0u, 0u};
    chan_mix_draw(d, n_chal, n_sent, nullptr, false, true, fa);
    chan_mix_draw(d, n_chal, n_sent, nullptr, false, true, fl);
    const qm31 lambda = {fl[0], fl[1], fl[2], fl[3]};
    if (in) {
        // random_linear_combination(claims, lambda) 2^shift (sumcheck.ts proveBatch doubles the claims of the shorter oracles)
        const qm31 claim = qm31_mul_m31(qm31_add(c0, qm31_mul(c1, lambda)), 1u << (shift % 31u));      // 2^31 = 1 in M31: any shift gives a reduced factor
        gstore4(t.state, 8 * lane, u4_of(claim));
        gstore4(t.state, 8 * lane + 4, u4_of(one));
    }
    // inv_eq0 of round r: 1 / prod_{j <= r} (1 - y_j).  Lane r holds y_r; an inclusive scan gives the prefix products, and every
    // lane inverts its own in the same instruction stream (one inversion step for the layer).
    qm31 y = zero;
    if (lane < t.n_y) y = q_of(gload4(t.y, 4 * lane));
    qm31 pre = lane < t.n_y ? qm31_sub(one, y) : one;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const qm31 up = {(u32)__shfl_up((int)pre.a, off, 64), (u32)__shfl_up((int)pre.b, off, 64), (u32)__shfl_up((int)pre.c, off, 64),
                         (u32)__shfl_up((int)pre.d, off, 64)};
        if (lane >= (u32)off) pre = qm31_mul(pre, up);
    }
    const qm31 inv = qm31_inv(pre);                     // a fixed power chain: zero in, zero out (and the status bit below)
    const bool bad = lane < t.n_y && (degenerate_y(y) || qm31_is_zero(pre));
    if (lane < t.n_y) gstore4(t.inv, 4 * lane, u4_of(inv));
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        if (any_bad) __hip_atomic_fetch_or(t.status, kStatusDegenerate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gstore4(t.scalars, 0, make_uint4(fa[0], fa[1], fa[2], fa[3]));
        gstore4(t.scalars, 4, u4_of(lambda));
        if (t.n_y) gstore4(t.scalars, 8, u4_of(qm31_sub(one, y)));      // eq([0], [y_0]): the v of EqEvals.generate
#pragma unroll
        for (int k = 0; k < 8; k++) gstore1(t.chan, k, d[k]);
        gstore1(t.chan, 8, n_chal);
        gstore1(t.chan, 9, n_sent);
    }
}

struct EndArgs {
    u32 *chan;
    const tstwo_gkr_lane *lanes;
    u32 n;
    u32 *masks, *claims, *ch_out;
};
__global__ void __launch_bounds__(64) k_gkr_layer_end(EndArgs t) {
    using namespace b2s;
    const u32 lane = threadIdx.x;
    const bool in = lane < t.n;
    const qm31 zero = {0u, 0u, 0u, 0u}, one = {1u, 0u, 0u, 0u};
    u32 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = gload1(t.chan, k);
    u32 n_chal = gload1(t.chan, 8), n_sent = gload1(t.chan, 9);
    // lane j: its mask (tryIntoMask, gkr_prover.ts:353-395) — column 0 at 0 and 1, column 1 at 0 and 1
    qm31 a0 = zero, b0 = zero, a1 = zero, b1 = zero;
    u32 n_felts = 0, inst = 0;
    bool gp = false;
    if (in) {
        const lane_ptr me = (lane_ptr)t.lanes + lane;
        const u32 kind = me->kind;
        inst = me->inst;
        gp = kind == TSTWO_GKR_GRAND_PRODUCT;
        n_felts = gp ? 2u : 4u;
        const u32 *src[8];
        load_lane_ptrs(me->src, src);
        const qm31 den0 = ld_col0(src, 4, 0), den1 = ld_col0(src, 4, 1);
        if (gp) {
            a0 = den0; b0 = den1;
        } else {
            a1 = den0; b1 = den1;
            if (kind == TSTWO_GKR_LOGUP_SINGLES) { a0 = one; b0 = one; }
            else { a0 = ld_col0(src, 0, 0); b0 = ld_col0(src, 0, 1); }
        }
        gstore4(t.masks, 16 * lane, u4_of(a0));
        gstore4(t.masks, 16 * lane + 4, u4_of(b0));
        gstore4(t.masks, 16 * lane + 8, u4_of(a1));
        gstore4(t.masks, 16 * lane + 12, u4_of(b1));
    }
#pragma unroll 1
    for (u32 j = 0; j < t.n; j++) {
        const qm31 f[4] = {bcast_q(a0, j), bcast_q(b0, j), bcast_q(a1, j), bcast_q(b1, j)};
        const u32 nf = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)n_felts, (int)j, 64));
        chan_mix_felts<true>(d, n_chal, n_sent, f, nf);
    }
    u32 felt[4] = {0u, 0u, 0u, 0u};
    chan_mix_draw(d, n_chal, n_sent, nullptr, false, true, felt);
    const qm31 ch = {felt[0], felt[1], felt[2], felt[3]};
    if (in) {                                           // reduceAtPoint: foldMleEvals of each column
        gstore4(t.claims, 8 * inst, u4_of(fold_q(ch, a0, b0)));
        gstore4(t.claims, 8 * inst + 4, u4_of(gp ? zero : fold_q(ch, a1, b1)));
    }
    if (lane == 0) {
        gstore4(t.ch_out, 0, u4_of(ch));
#pragma unroll
        for (int k = 0; k < 8; k++) gstore1(t.chan, k, d[k]);
        gstore1(t.chan, 8, n_chal);
        gstore1(t.chan, 9, n_sent);
    }
}

bool q_is(const u32 v[4], u32 a) { return v[0] == a && v[1] == 0 && v[2] == 0 && v[3] == 0; }

// ---- checks + launches of the entries that take their scalars from device memory (the public entries and tstwo_gkr_prove_batch)
bool dev_scalar_ok(const void *p) { return p && aligned16(p); }

int eq_evals_dev(const u32 *y_dev, u32 n_y, const u32 *v_dev, u32 *const out[4]) {
    if (n_y > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "eq table too large");
    if (!dev_scalar_ok(v_dev) || (n_y && !dev_scalar_ok(y_dev))) return set_error(TSTWO_ERR_BAD_ARG, "eq table: null or misaligned device scalar");
    TSTWO_REQUIRE_TABLE(out, 4);
    const u32 lo = n_y / 2, hi = n_y - lo, nt = (1u << hi) + (1u << lo);
    if (int rc = ensure_scratch(kTabOff + (size_t)nt * sizeof(qm31))) return rc;
    qm31 *tab = (qm31 *)((uint8_t *)ctx().scratch + kTabOff);
    hipLaunchKernelGGL(k_eq_tables_dev, dim3(ceil_div(nt, kThreads)), dim3(kThreads), 0, ctx().stream, y_dev, v_dev, hi, lo, tab);
    TSTWO_LAUNCH_CHECK();
    const Soa4 o = soa(out);
    const u32 n = 1u << n_y;
    if (lo >= 2 && all_aligned16(o)) hipLaunchKernelGGL(k_eq_expand<4>, dim3(grid_for(n / 4, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    else hipLaunchKernelGGL(k_eq_expand<1>, dim3(grid_for(n, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int round_finish_dev(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 *y_dev, const u32 *a_dev,
                     const u32 *alpha_dev, u32 *round_poly_out, u32 *challenge_out, u32 *status) {
    TSTWO_REQUIRE_PTRS(chan, sums, state, round_poly_out, challenge_out, status);
    if (n_instances == 0 || n_instances > 64) return set_error(TSTWO_ERR_BAD_ARG, "sum-check: 1 to 64 instances per round");
    if (((uintptr_t)chan & 3) || ((uintptr_t)status & 3) || !aligned16(sums) || !aligned16(state) || !aligned16(round_poly_out) ||
        !aligned16(challenge_out))
        return set_error(TSTWO_ERR_BAD_ARG, "sum-check: misaligned device pointer");
    if (!dev_scalar_ok(y_dev) || !dev_scalar_ok(a_dev) || !dev_scalar_ok(alpha_dev))
        return set_error(TSTWO_ERR_BAD_ARG, "sum-check: null or misaligned device scalar");
    FinishArgs f{};
    f.chan = chan; f.sums = sums; f.state = state; f.n = n_instances;
    f.mask = n_instances == 64 ? active_mask : active_mask & ((1ull << n_instances) - 1);
    f.poly_out = round_poly_out; f.ch_out = challenge_out;
    const FinishDev d{y_dev, a_dev, alpha_dev, status};
    hipLaunchKernelGGL(k_gkr_round_finish_dev, dim3(1), dim3(64), 0, ctx().stream, f, d);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int layer_begin(u32 *chan, const tstwo_gkr_lane *lanes, u32 n, const u32 *claims, u32 *out_claims, u32 *state, u32 *scalars, const u32 *y_dev,
                u32 n_y, u32 *inv, u32 *status) {
    TSTWO_REQUIRE_PTRS(chan, lanes, claims, out_claims, state, scalars, inv, status);
    if (n == 0 || n > 64) return set_error(TSTWO_ERR_BAD_ARG, "layer begin: 1 to 64 lanes");
    if (n_y > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "layer begin: more than 28 coordinates");
    if (n_y && !dev_scalar_ok(y_dev)) return set_error(TSTWO_ERR_BAD_ARG, "layer begin: null or misaligned device scalar");
    if (((uintptr_t)chan & 3) || ((uintptr_t)status & 3) || ((uintptr_t)lanes & 7) || !aligned16(claims) || !aligned16(out_claims) ||
        !aligned16(state) || !aligned16(scalars) || !aligned16(inv))
        return set_error(TSTWO_ERR_BAD_ARG, "layer begin: misaligned device pointer");
    const BeginArgs t{chan, lanes, n, claims, out_claims, state, scalars, y_dev, n_y, inv, status};
    hipLaunchKernelGGL(k_gkr_layer_begin, dim3(1), dim3(64), 0, ctx().stream, t);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int layer_end(u32 *chan, const tstwo_gkr_lane *lanes, u32 n, u32 *masks, u32 *claims, u32 *ch_out) {
    TSTWO_REQUIRE_PTRS(chan, lanes, masks, claims, ch_out);
    if (n == 0 || n > 64) return set_error(TSTWO_ERR_BAD_ARG, "layer end: 1 to 64 lanes");
    if (((uintptr_t)chan & 3) || ((uintptr_t)lanes & 7) || !aligned16(masks) || !aligned16(claims) || !aligned16(ch_out))
        return set_error(TSTWO_ERR_BAD_ARG, "layer end: misaligned device pointer");
    const EndArgs t{chan, lanes, n, masks, claims, ch_out};
    hipLaunchKernelGGL(k_gkr_layer_end, dim3(1), dim3(64), 0, ctx().stream, t);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// ---------------------------------------------------------------- prove_batch in one call (gkr_prover.ts:440-580)
// One instance's layer as the kernels see it: 4 numerator pointers (a base column repeats its one pointer; null without
// numerators) and 4 denominator pointers.
struct LayerView {
    u32 kind;
    u32 *num[4], *den[4];
};
// generated layer k of instance p inside the pool: all LogUp kinds generate LogUpGeneric layers (numerators, then denominators)
LayerView generated_layer(u32 *pool, const GkrPlanInst &p, u32 k) {
    LayerView v{};
    v.kind = p.kind == kGkrGrandProduct ? kGkrGrandProduct : kGkrGeneric;
    u32 *base = pool + gkr_layer_off(p, k);
    const uint64_t w = gkr_col_words(k);
    for (int c = 0; c < 4; c++) {
        v.num[c] = p.gen_cols == 8 ? base + c * w : nullptr;
        v.den[c] = base + (p.gen_cols == 8 ? 4 + c : c) * w;
    }
    return v;
}
LayerView input_layer(const tstwo_gkr_instance &in) {
    LayerView v{};
    v.kind = in.kind;
    for (int c = 0; c < 4; c++) {
        // never written: the plan folds an input into the instance's own buffers (GKR_FOLD_NEW)
        v.num[c] = in.kind == kGkrGeneric ? (u32 *)in.num[c] : in.kind == kGkrMultiplicities ? (u32 *)in.num[0] : nullptr;
        v.den[c] = (u32 *)in.den[c];
    }
    return v;
}
int launch_next_layer(const LayerView &in, u32 log_n, const LayerView &out) {
    const u32 n_out = 1u << (log_n - 1);
    const dim3 g(grid_for(n_out, 32)), b(kThreads);
    const CSoa4 num = csoa(in.num), den = csoa(in.den);
    const Soa4 onum = soa(out.num), oden = soa(out.den);
    hipStream_t st = ctx().stream;
    switch (in.kind) {
        case kGkrGrandProduct: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_GRAND_PRODUCT>, g, b, 0, st, CSoa4{}, den, Soa4{}, oden, n_out); break;
        case kGkrGeneric: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_GENERIC>, g, b, 0, st, num, den, onum, oden, n_out); break;
        case kGkrMultiplicities: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_MULTIPLICITIES>, g, b, 0, st, num, den, onum, oden, n_out); break;
        default: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_SINGLES>, g, b, 0, st, CSoa4{}, den, onum, oden, n_out); break;
    }
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}
void fill_lane_ptrs(const u32 *(&dst)[8], const LayerView &v) {
    for (int c = 0; c < 4; c++) { dst[c] = v.num[c]; dst[4 + c] = v.den[c]; }
}

int plan_of(const tstwo_gkr_instance *instances, size_t n, GkrPlan &pl) {
    if (n && !instances) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    u32 kinds[kGkrMaxInstances], logs[kGkrMaxInstances];
    for (size_t i = 0; i < n && i < kGkrMaxInstances; i++) { kinds[i] = instances[i].kind; logs[i] = instances[i].log_n; }
    if (const char *why = gkr_plan(kinds, logs, n, pl)) return set_error(TSTWO_ERR_BAD_ARG, why);
    return TSTWO_OK;
}

// Everything the call allocated goes back to the allocator on every way out, behind a synchronisation (launches may be in flight).
struct ProveBuffers {
    void *pool = nullptr, *block = nullptr, *lanes = nullptr;
    ~ProveBuffers() {
        (void)hipStreamSynchronize(ctx().stream);
        for (void *p : {pool, block, lanes}) if (p) tstwo_free(p);
    }
};

int prove_batch_run(const u32 chan[10], const tstwo_gkr_instance *instances, const GkrPlan &pl, u32 *block_host) {
    const u32 n = pl.n_inst, n_layers = pl.n_layers;
    ProveBuffers mem;
    if (int rc = tstwo_malloc(&mem.pool, pl.pool_words * 4)) return rc;
    if (int rc = tstwo_malloc(&mem.block, (size_t)pl.block_words * 4)) return rc;
    size_t n_lanes_total = 0;
    for (const GkrPlanLayer &l : pl.layers) n_lanes_total += l.n_active;
    if (int rc = tstwo_malloc(&mem.lanes, n_lanes_total * sizeof(tstwo_gkr_lane))) return rc;
    if (int rc = ensure_scratch(kTabOff + ((size_t)2 << (kMaxLog / 2 + 1)) * sizeof(qm31))) return rc;
    u32 *const pool = (u32 *)mem.pool, *const blk = (u32 *)mem.block;
    hipStream_t st = ctx().stream;

    // the layers of every instance: [0 .. log_n) generated, [log_n] the caller's
    std::vector<std::vector<LayerView>> lay(n);
    u32 widest = 0;                                      // an instance with n_layers variables: its dead layers hold the eq tables
    for (u32 i = 0; i < n; i++) {
        const GkrPlanInst &p = pl.inst[i];
        for (u32 k = 0; k < p.log_n; k++) lay[i].push_back(generated_layer(pool, p, k));
        lay[i].push_back(input_layer(instances[i]));
        if (p.log_n == n_layers && pl.inst[widest].log_n != n_layers) widest = i;
        for (u32 k = p.log_n; k >= 1; k--)
            if (int rc = launch_next_layer(lay[i][k], k, lay[i][k - 1])) return rc;
    }
    TSTWO_HIP(hipMemsetAsync(blk, 0, (size_t)pl.block_words * 4, st));
    TSTWO_HIP(hipMemcpyAsync(blk + pl.chan_off, chan, 10 * sizeof(u32), hipMemcpyHostToDevice, st));

    // the lanes of every layer, known before anything runs: where each mask will lie once the layer's folds are done
    std::vector<tstwo_gkr_lane> lanes(n_lanes_total);
    std::vector<size_t> lane0(n_layers);
    {
        size_t at = 0;
        for (u32 L = 0; L < n_layers; L++) {
            lane0[L] = at;
            for (u32 i = 0; i < n; i++) {
                const GkrPlanInst &p = pl.inst[i];
                const int n_v = gkr_n_v(p, L);
                if (n_v < 0) continue;
                tstwo_gkr_lane &ln = lanes[at++];
                ln = tstwo_gkr_lane{};
                const bool input = (u32)n_v + 1 == p.log_n;
                // the reduced layer ends as 2 points: in place for a generated layer, in the dead layer below for an input that
                // was folded (n_v >= 1), the input itself where it has one variable
                const LayerView &src = input && n_v >= 1 ? lay[i][p.log_n - 1] : lay[i][n_v + 1];
                const u32 kind = input ? (p.kind == kGkrMultiplicities ? kGkrGeneric : p.kind) : src.kind;
                fill_lane_ptrs(ln.src, src);
                ln.inst = i; ln.kind = kind; ln.shift = L - (u32)n_v; ln.enter = n_v == 0;
                fill_lane_ptrs(ln.out_src, lay[i][0]);
            }
        }
    }
    TSTWO_HIP(hipMemcpyAsync(mem.lanes, lanes.data(), n_lanes_total * sizeof(tstwo_gkr_lane), hipMemcpyHostToDevice, st));
    const tstwo_gkr_lane *lanes_dev = (const tstwo_gkr_lane *)mem.lanes;

    u32 *const status = blk + pl.status_off, *const chan_dev = blk + pl.chan_off;
    for (u32 L = 0; L < n_layers; L++) {
        const GkrPlanLayer &gl = pl.layers[L];
        u32 *const ood_cur = blk + pl.ood_off[L & 1], *const ood_next = blk + pl.ood_off[(L + 1) & 1];
        const tstwo_gkr_lane *ld = lanes_dev + lane0[L];
        if (int rc = layer_begin(chan_dev, ld, gl.n_active, blk + pl.ctv_off, blk + pl.out_off, blk + pl.state_off, blk + pl.alpha_off, ood_cur,
                                 L, blk + pl.inv_off, status))
            return rc;
        // EqEvals.generate(ood): eq((0, x), y) = genEqEvals(y[1:], 1 - y[0]), into the widest instance's dead layer of L - 1 variables
        const LayerView eqv = L ? lay[widest][L - 1] : LayerView{};
        if (L)
            if (int rc = eq_evals_dev(ood_cur + 4, L - 1, blk + pl.eqv_off, eqv.den)) return rc;
        // per lane: the layer being reduced, and the challenge not yet applied to it
        struct Cur { LayerView v; u32 n_vars; const u32 *pending; u32 inst; };
        std::vector<Cur> cur;
        for (u32 j = 0; j < gl.n_active; j++) {
            const u32 i = lanes[lane0[L] + j].inst;
            const u32 n_v = (u32)gkr_n_v(pl.inst[i], L);
            cur.push_back({lay[i][n_v + 1], n_v + 1, nullptr, i});
        }
        auto target = [&](const Cur &c, GkrFold how) {
            return how == GKR_FOLD_IN_PLACE ? c.v : lay[c.inst][pl.inst[c.inst].log_n - 1];
        };
        for (u32 rnd = 0; rnd < L; rnd++) {
            const u32 rem = L - rnd;
            const uint64_t mask = gkr_round_lanes(pl, L, rem);
            for (u32 j = 0; j < gl.n_active; j++) {
                if (!((mask >> j) & 1)) continue;
                Cur &c = cur[j];
                const GkrFold how = gkr_round_fold(pl, pl.inst[c.inst], L, rem);
                u32 *const slot = blk + pl.sums_off + 8 * j;
                if (how == GKR_NO_FOLD) {
                    if (int rc = gkr_sum(c.v.kind, eqv.den, c.v.num, c.v.den, nullptr, nullptr, rem, nullptr, nullptr, nullptr, slot, false,
                                         blk + pl.lambda_off))
                        return rc;
                } else {
                    const LayerView to = target(c, how);
                    if (int rc = gkr_sum(c.v.kind, eqv.den, c.v.num, c.v.den, to.num, to.den, rem, nullptr, c.pending, nullptr, slot, true,
                                         blk + pl.lambda_off))
                        return rc;
                    const bool had_num = c.v.kind == kGkrGeneric || c.v.kind == kGkrMultiplicities;
                    const u32 kind = c.v.kind == kGkrMultiplicities ? kGkrGeneric : c.v.kind;
                    c.v = to;
                    c.v.kind = kind;
                    if (!had_num) for (int k = 0; k < 4; k++) c.v.num[k] = nullptr;
                    c.n_vars--;
                }
                c.pending = ood_next + 4 * rnd;              // the challenge this round is about to draw
            }
            if (int rc = round_finish_dev(chan_dev, blk + pl.sums_off, blk + pl.state_off, gl.n_active, mask, ood_cur + 4 * rnd,
                                          blk + pl.inv_off + 4 * rnd, blk + pl.alpha_off, blk + gl.poly_off + 20 * rnd, ood_next + 4 * rnd, status))
                return rc;
        }
        // the last challenge of the layer: a plain fold leaves the 2-point layer the mask is read from
        for (Cur &c : cur) {
            if (!c.pending) continue;
            const LayerView to = target(c, gkr_last_fold(pl, pl.inst[c.inst], L));
            if (c.v.kind == kGkrGeneric || c.v.kind == kGkrMultiplicities)
                if (int rc = mle_fold(c.v.kind == kGkrMultiplicities, c.v.num, c.n_vars, nullptr, c.pending, to.num)) return rc;
            if (int rc = mle_fold(false, c.v.den, c.n_vars, nullptr, c.pending, to.den)) return rc;
        }
        if (int rc = layer_end(chan_dev, ld, gl.n_active, blk + gl.mask_off, blk + pl.ctv_off, ood_next + 4 * L)) return rc;
    }
    TSTWO_HIP(hipMemcpyAsync(block_host, blk, (size_t)pl.block_words * 4, hipMemcpyDeviceToHost, st));
    TSTWO_HIP(hipStreamSynchronize(st));
    if (block_host[pl.status_off] & kStatusDegenerate) return set_error(TSTWO_ERR_BAD_ARG, "sum-check: degenerate eq point");
    return TSTWO_OK;
}

}  // namespace

extern "C" {

int tstwo_gkr_round_finish(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 y_k[4],
                           const u32 inv_eq0[4], const u32 alpha[4], u32 *round_poly_out, u32 *challenge_out) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(chan, sums, state, round_poly_out, challenge_out);
    if (!y_k || !inv_eq0 || !alpha) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    if (n_instances == 0 || n_instances > 64) return set_error(TSTWO_ERR_BAD_ARG, "sum-check: 1 to 64 instances per round");
    if (((uintptr_t)chan & 3) || !aligned16(sums) || !aligned16(state) || !aligned16(round_poly_out) || !aligned16(challenge_out))
        return set_error(TSTWO_ERR_BAD_ARG, "sum-check: misaligned device pointer");
    // y_k = 1/2: b is undefined; y_k = 1, 0, 1/3: b = 0, 1, 2 collides with an interpolation point
    if (q_is(y_k, 0u) || q_is(y_k, 1u) || q_is(y_k, 1u << 30) || q_is(y_k, 0x55555555u))
        return set_error(TSTWO_ERR_BAD_ARG, "sum-check: degenerate eq point");
    FinishArgs f{};
    f.chan = chan; f.sums = sums; f.state = state; f.n = n_instances;
    f.mask = n_instances == 64 ? active_mask : active_mask & ((1ull << n_instances) - 1);
    f.y = qarg(y_k); f.a = qarg(inv_eq0); f.alpha = qarg(alpha);
    f.poly_out = round_poly_out; f.ch_out = challenge_out;
    hipLaunchKernelGGL(k_gkr_round_finish, dim3(1), dim3(64), 0, ctx().stream, f);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}


int tstwo_gkr_gen_eq_evals(const u32 *y, u32 n_y, const u32 v[4], u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    if (n_y > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "eq table too large");
    if (!v || (n_y && !y)) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    TSTWO_REQUIRE_TABLE(out, 4);
    EqY ys{};
    for (u32 k = 0; k < n_y; k++) ys.y[k] = {y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]};
    const u32 lo = n_y / 2, hi = n_y - lo, nt = (1u << hi) + (1u << lo);
    if (int rc = ensure_scratch(kTabOff + (size_t)nt * sizeof(qm31))) return rc;
    qm31 *tab = (qm31 *)((uint8_t *)ctx().scratch + kTabOff);
    hipLaunchKernelGGL(k_eq_tables, dim3(ceil_div(nt, kThreads)), dim3(kThreads), 0, ctx().stream, ys, qarg(v), hi, lo, tab);
    TSTWO_LAUNCH_CHECK();
    const Soa4 o = soa(out);
    const u32 n = 1u << n_y;
    if (lo >= 2 && all_aligned16(o)) hipLaunchKernelGGL(k_eq_expand<4>, dim3(grid_for(n / 4, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    else hipLaunchKernelGGL(k_eq_expand<1>, dim3(grid_for(n, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_gkr_next_layer_grand_product(const u32 *const in[4], u32 log_n, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    if (log_n == 0) return set_error(TSTWO_ERR_BAD_ARG, "next_layer of an output layer");
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "GKR layer too large");
    TSTWO_REQUIRE_TABLE(in, 4); TSTWO_REQUIRE_TABLE(out, 4);
    const u32 n_out = 1u << (log_n - 1);
    hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_GRAND_PRODUCT>, dim3(grid_for(n_out, 32)), dim3(kThreads), 0, ctx().stream, CSoa4{},
                       csoa(in), Soa4{}, soa(out), n_out);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_gkr_next_layer_logup(u32 kind, const u32 *const num[4], const u32 *const den[4], u32 log_n, u32 *const out_num[4],
                               u32 *const out_den[4]) {
    TSTWO_REQUIRE_READY();
    if (kind < TSTWO_GKR_LOGUP_GENERIC || kind > TSTWO_GKR_LOGUP_SINGLES) return set_error(TSTWO_ERR_BAD_ARG, "unknown LogUp numerator kind");
    if (log_n == 0) return set_error(TSTWO_ERR_BAD_ARG, "next_layer of an output layer");
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "GKR layer too large");
    TSTWO_REQUIRE_TABLE(den, 4); TSTWO_REQUIRE_TABLE(out_num, 4); TSTWO_REQUIRE_TABLE(out_den, 4);
    const u32 n_out = 1u << (log_n - 1);
    const dim3 g(grid_for(n_out, 32)), b(kThreads);
    if (kind == TSTWO_GKR_LOGUP_GENERIC) {
        TSTWO_REQUIRE_TABLE(num, 4);
        hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_GENERIC>, g, b, 0, ctx().stream, csoa(num), csoa(den), soa(out_num), soa(out_den), n_out);
    } else if (kind == TSTWO_GKR_LOGUP_MULTIPLICITIES) {
        TSTWO_REQUIRE_TABLE(num, 1);
        hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_MULTIPLICITIES>, g, b, 0, ctx().stream, csoa1(num[0]), csoa(den), soa(out_num), soa(out_den), n_out);
    } else {
        hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_SINGLES>, g, b, 0, ctx().stream, CSoa4{}, csoa(den), soa(out_num), soa(out_den), n_out);
    }
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int tstwo_gkr_sum_poly(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 n_vars,
                       const u32 lambda[4], u32 out[8]) {
    TSTWO_REQUIRE_READY();
    if (!out) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    u32 *page = (u32 *)result_target(8 * sizeof(u32));
    u32 *dst = page ? page : (u32 *)nullptr;
    if (!page) {
        if (int rc = ensure_scratch(kTabOff)) return rc;
        dst = (u32 *)((uint8_t *)ctx().scratch + kResultOff);
    }
    if (int rc = gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, lambda, dst, false)) return rc;
    if (page) {
        const void *view = nullptr;
        if (int rc = result_wait(&view)) return rc;
        for (int k = 0; k < 8; k++) out[k] = ((const volatile u32 *)view)[k];
        return TSTWO_OK;
    }
    return small_d2h(out, dst, 8 * sizeof(u32));
}

int tstwo_gkr_sum_poly_async(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 n_vars,
                             const u32 lambda[4], u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev);
    return gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, lambda, out_dev, false);
}

int tstwo_gkr_round(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const out_num[4],
                    u32 *const out_den[4], u32 n_vars, const u32 r[4], const u32 lambda[4], u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev);
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, r, nullptr, lambda, out_dev, true);
}

int tstwo_mle_fix_first_variable_base(const u32 *in, u32 log_n, const u32 r[4], u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    const u32 *const in4[4] = {in, in, in, in};
    return mle_fold(true, in4, log_n, r, nullptr, out);
}

int tstwo_mle_fix_first_variable_secure(const u32 *const in[4], u32 log_n, const u32 r[4], u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    return mle_fold(false, in, log_n, r, nullptr, out);
}

int tstwo_gkr_round_dev(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const out_num[4],
                        u32 *const out_den[4], u32 n_vars, const u32 *r_dev, const u32 lambda[4], u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev, r_dev);
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, nullptr, r_dev, lambda, out_dev, true);
}

int tstwo_mle_fix_first_variable_base_dev(const u32 *in, u32 log_n, const u32 *r_dev, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    const u32 *const in4[4] = {in, in, in, in};
    return mle_fold(true, in4, log_n, nullptr, r_dev, out);
}

int tstwo_mle_fix_first_variable_secure_dev(const u32 *const in[4], u32 log_n, const u32 *r_dev, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    return mle_fold(false, in, log_n, nullptr, r_dev, out);
}

int tstwo_gkr_gen_eq_evals_dev(const u32 *y_dev, u32 n_y, const u32 *v_dev, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    return eq_evals_dev(y_dev, n_y, v_dev, out);
}

int tstwo_gkr_sum_poly_async_ldev(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 n_vars,
                                  const u32 *lambda_dev, u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev, lambda_dev);
    return gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, nullptr, out_dev, false, lambda_dev);
}

int tstwo_gkr_round_dev_ldev(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const out_num[4],
                             u32 *const out_den[4], u32 n_vars, const u32 *r_dev, const u32 *lambda_dev, u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev, r_dev, lambda_dev);
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, nullptr, r_dev, nullptr, out_dev, true, lambda_dev);
}

int tstwo_gkr_round_finish_dev(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 *y_k_dev,
                               const u32 *inv_eq0_dev, const u32 *alpha_dev, u32 *round_poly_out, u32 *challenge_out, u32 *status) {
    TSTWO_REQUIRE_READY();
    return round_finish_dev(chan, sums, state, n_instances, active_mask, y_k_dev, inv_eq0_dev, alpha_dev, round_poly_out, challenge_out, status);
}

int tstwo_gkr_layer_begin(u32 *chan, const tstwo_gkr_lane *lanes_dev, u32 n_lanes, const u32 *claims, u32 *output_claims, u32 *state,
                          u32 *scalars_out, const u32 *y_dev, u32 n_y, u32 *inv_eq0_out, u32 *status) {
    TSTWO_REQUIRE_READY();
    return layer_begin(chan, lanes_dev, n_lanes, claims, output_claims, state, scalars_out, y_dev, n_y, inv_eq0_out, status);
}

int tstwo_gkr_layer_end(u32 *chan, const tstwo_gkr_lane *lanes_dev, u32 n_lanes, u32 *masks_out, u32 *claims, u32 *challenge_out) {
    TSTWO_REQUIRE_READY();
    return layer_end(chan, lanes_dev, n_lanes, masks_out, claims, challenge_out);
}

int tstwo_gkr_prove_batch_words(const tstwo_gkr_instance *instances, size_t n_instances, size_t *block_words) {
    if (!block_words) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    GkrPlan pl;
    if (int rc = plan_of(instances, n_instances, pl)) return rc;
    *block_words = pl.block_words;
    return TSTWO_OK;
}

int tstwo_gkr_prove_batch(const u32 chan[10], const tstwo_gkr_instance *instances, size_t n_instances, u32 *block, size_t block_words) {
    TSTWO_REQUIRE_READY();
    if (!chan || !block) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    GkrPlan pl;
    if (int rc = plan_of(instances, n_instances, pl)) return rc;
    if (block_words < pl.block_words) return set_error(TSTWO_ERR_BAD_ARG, "prove_batch: the block is too small (tstwo_gkr_prove_batch_words)");
    for (size_t i = 0; i < n_instances; i++) {
        const tstwo_gkr_instance &in = instances[i];
        const int n_num = in.kind == kGkrGeneric ? 4 : in.kind == kGkrMultiplicities ? 1 : 0;
        TSTWO_REQUIRE_TABLE(in.den, 4);
        TSTWO_REQUIRE_TABLE(in.num, (size_t)n_num);
        for (int c = 0; c < 4; c++)
            if (((uintptr_t)in.den[c] & 3) || (c < n_num && ((uintptr_t)in.num[c] & 3)))
                return set_error(TSTWO_ERR_BAD_ARG, "prove_batch: misaligned device pointer");
    }
    if (stream_is_capturing()) return set_error(TSTWO_ERR_BAD_ARG, "prove_batch during graph capture (it reads its result back)");
    return prove_batch_run(chan, instances, pl, block);
}

}  // extern "C"

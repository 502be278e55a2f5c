// gkr_ops.hip — GkrOps / MleOps of the reference (backend/cpu/lookups/gkr.ts:84-358, backend/cpu/lookups/mle.ts:60-130) on
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
// A protocol scalar (the eq point and v, the fold's challenge, lambda) comes by value or from 4 device words an earlier launch on
// the stream wrote (the _dev / _ldev entries and tstwo_gkr_prove_batch): the same kernel either way.
// M31 addition is exact, so the reduction order does not change a bit of the result.
// The single-wave transcript kernels are in gkr_transcript.hip, the one-call proof in gkr_prove.hip.
#include "gkr_internal.h"

using namespace tstwo;

namespace {

constexpr int kThreads = 256;

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
__device__ __forceinline__ qm31 fold_b(qm31 r, u32 lhs, u32 rhs) {
    qm31 t = qm31_mul_m31(r, m31_sub(rhs, lhs));
    t.a = m31_add(t.a, lhs);
    return t;
}

// ---------------------------------------------------------------- eq table (gkr.ts:90-104)
// out[x] = v * prod_k eq(bit_k(x), y[k]), bit 0 of that product = the MOST significant bit of x.  hi = the first n - lo variables
// (high bits of x), lo = the last lo variables.  tab[0 .. 2^hi) = v * eq(high bits, y[0..hi)), tab[2^hi .. 2^hi + 2^lo) =
// eq(low bits, y[hi..n)).  eq(0, y) = 1 - y, eq(1, y) = y.
// The point and v come by value, or (y_dev / v_dev non-null) from device words an earlier launch on the stream left there
// (tstwo_gkr_layer_end / _begin).  Lane t then reads y[y0 + k] for k = 0 .. nb: one address per wave wherever a wave lies within
// one of the two tables (always from 2^6 high entries on), so the loads are broadcasts out of one cache line.
__global__ void __launch_bounds__(kThreads) k_eq_tables(EqY y, qm31 v, const u32 *__restrict__ y_dev, const u32 *__restrict__ v_dev, u32 hi,
                                                        u32 lo, qm31 *tab) {
    const u32 t = blockIdx.x * kThreads + threadIdx.x;
    const u32 nh = 1u << hi, nl = 1u << lo;
    if (t >= nh + nl) return;
    const bool high = t < nh;
    const u32 idx = high ? t : t - nh, nb = high ? hi : lo, y0 = high ? 0 : hi;
    const qm31 one = {1u, 0u, 0u, 0u};
    qm31 acc = one;
    if (high) acc = v_dev ? q_of(gload4(v_dev)) : v;
#pragma unroll 1
    for (u32 k = 0; k < nb; k++) {
        const qm31 yk = y_dev ? q_of(gload4(y_dev, 4 * (y0 + k))) : y.y[y0 + k];
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

// ---------------------------------------------------------------- fix_first_variable (mle.ts:68-130)
// out[i] = in[i] + r (in[i + half] - in[i]); W = 4: 16-byte accesses.  In place (out == in) is safe: lane i reads i and
// i + half and writes i only.
template <bool BASE, int W>
__global__ void __launch_bounds__(kThreads) k_fold(CSoa4 in, qm31 r, const u32 *__restrict__ r_dev, Soa4 out, u32 half) {
    r = scalar_q(r, r_dev);                     // r_dev: the challenge an earlier launch drew (tstwo_gkr_round_finish)
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
    const u32 *r_dev, *lambda_dev;   // non-null = r (FOLD) / lambda is read from these 4 device words instead (scalar_q)
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
    __shared__ u32 lds[8 * (kThreads / 64) + 1];       // wave partials; [last] = "this block is the last arriver"
    u32 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const u32 nt = a.n_terms, stride = gridDim.x * kThreads;
    if (FOLD) a.r = scalar_q(a.r, a.r_dev);
    if (KIND != TSTWO_GKR_GRAND_PRODUCT) a.lambda = scalar_q(a.lambda, a.lambda_dev);      // a grand product has no lambda
    for (u32 i = blockIdx.x * kThreads + threadIdx.x; i < nt; i += stride) {
        const u32 p0 = 2 * i, p1 = 2 * (nt + i);
        const qm31 n00 = num_at<KIND, FOLD>(a, p0), n01 = num_at<KIND, FOLD>(a, p0 + 1);
        const qm31 n10 = num_at<KIND, FOLD>(a, p1), n11 = num_at<KIND, FOLD>(a, p1 + 1);
        const qm31 d00 = den_at<FOLD>(a, p0), d01 = den_at<FOLD>(a, p0 + 1);
        const qm31 d10 = den_at<FOLD>(a, p1), d11 = den_at<FOLD>(a, p1 + 1);
        const qm31 n20 = qm31_sub(q_double(n10), n00), n21 = qm31_sub(q_double(n11), n01);
        const qm31 d20 = qm31_sub(q_double(d10), d00), d21 = qm31_sub(q_double(d11), d01);
        const qm31 e = ld_q(a.eq, i);
        const qm31 at0 = qm31_mul(e, gate<KIND>(a, n00, d00, n01, d01));
        const qm31 at2 = qm31_mul(e, gate<KIND>(a, n20, d20, n21, d21));
        acc[0] = m31_add(acc[0], at0.a); acc[1] = m31_add(acc[1], at0.b); acc[2] = m31_add(acc[2], at0.c); acc[3] = m31_add(acc[3], at0.d);
        acc[4] = m31_add(acc[4], at2.a); acc[5] = m31_add(acc[5], at2.b); acc[6] = m31_add(acc[6], at2.c); acc[7] = m31_add(acc[7], at2.d);
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u32 kWaves = kThreads / 64, kLast = 8 * kWaves;
    wave_sum8(acc);
    if (lane == 0)
        for (int k = 0; k < 8; k++) lds[8 * wave + k] = acc[k];
    __syncthreads();
    // block partial -> slab[block]; then the in-launch hand-off of a split reduction: stores drained, agent-scope release, drained
    // again (the release's own wait can be dropped by the compiler), relaxed agent-scope ticket; the block that draws the last
    // ticket acquires at agent scope and reduces every slab row.  Correct for any placement of the blocks over XCDs; the ticket is
    // zeroed by a memset ahead of every launch.
    if (threadIdx.x < 8) {
        u32 s = 0;
        for (u32 w = 0; w < kWaves; w++) s = m31_add(s, lds[8 * w + threadIdx.x]);
        gstore1(a.slab, blockIdx.x * 8 + threadIdx.x, s);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u32 t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u32 last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds[kLast] = last;
    }
    __syncthreads();
    if (!lds[kLast]) return;
    u32 tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (u32 b = threadIdx.x; b < gridDim.x; b += kThreads)
#pragma unroll
        for (int k = 0; k < 8; k++) tot[k] = m31_add(tot[k], gload1(a.slab, b * 8 + k));
    wave_sum8(tot);
    __syncthreads();                         // every wave has read lds[kLast] before it is overwritten below
    if (lane == 0)
        for (int k = 0; k < 8; k++) lds[8 * wave + k] = tot[k];
    __syncthreads();
    if (threadIdx.x < 8) {
        u32 s = 0;
        for (u32 w = 0; w < kWaves; w++) s = m31_add(s, lds[8 * w + threadIdx.x]);
        *(volatile TSTWO_GLOBAL u32 *)(a.out + threadIdx.x) = s;
    }
}

template <int KIND>
int launch_sum_kind(const SumArgs &a, bool fold, unsigned grid) {
    const dim3 g(grid), b(kThreads);
    if (fold) hipLaunchKernelGGL((k_sum<KIND, true>), g, b, 0, ctx().stream, a);
    else hipLaunchKernelGGL((k_sum<KIND, false>), g, b, 0, ctx().stream, a);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

bool valid_kind(u32 kind) { return kind <= TSTWO_GKR_LOGUP_SINGLES; }
CSoa4 csoa(const u32 *const c[4]) { return {{c[0], c[1], c[2], c[3]}}; }
Soa4 soa(u32 *const c[4]) { return {{c[0], c[1], c[2], c[3]}}; }
CSoa4 csoa1(const u32 *c) { return {{c, c, c, c}}; }

}  // namespace

namespace tstwo {

// Checks and launches one sum (fold: the fused round); `out` = 8 device-visible words.
// The fold's challenge is r (host words) or, when r_dev is given, 4 words of device memory written earlier on the stream; lambda
// likewise: host words, or (lambda null) the 4 device words at lambda_dev.
int gkr_sum(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const onum[4],
            u32 *const oden[4], u32 n_vars, const u32 r[4], const u32 *r_dev, const u32 lambda[4], const u32 *lambda_dev, u32 *out,
            bool fold) {
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
    if (lambda) a.lambda = to_q(lambda);
    else a.lambda_dev = lambda_dev;
    if (kind == TSTWO_GKR_LOGUP_GENERIC) { TSTWO_REQUIRE_TABLE(num, 4); a.num = csoa(num); }
    if (kind == TSTWO_GKR_LOGUP_MULTIPLICITIES) { TSTWO_REQUIRE_TABLE(num, 1); a.num = csoa1(num[0]); }
    if (fold) {
        if (!r && !r_dev) return set_error(TSTWO_ERR_BAD_ARG, "null challenge");
        if (!aligned16(r_dev)) return set_error(TSTWO_ERR_BAD_ARG, "device challenge is not 16-byte aligned");
        if (r) a.r = to_q(r);
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
        case TSTWO_GKR_GRAND_PRODUCT: return launch_sum_kind<TSTWO_GKR_GRAND_PRODUCT>(a, fold, grid);
        case TSTWO_GKR_LOGUP_GENERIC: return launch_sum_kind<TSTWO_GKR_LOGUP_GENERIC>(a, fold, grid);
        case TSTWO_GKR_LOGUP_MULTIPLICITIES: return launch_sum_kind<TSTWO_GKR_LOGUP_MULTIPLICITIES>(a, fold, grid);
        default: return launch_sum_kind<TSTWO_GKR_LOGUP_SINGLES>(a, fold, grid);
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
    const qm31 rv = r ? to_q(r) : qm31{0u, 0u, 0u, 0u};
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

// Checks and launches one eq table: scratch, the two half tables, their expansion.  Host words travel in the kernel's arguments.
int eq_evals(const u32 *y, u32 n_y, const u32 *v, bool dev, u32 *const out[4]) {
    if (n_y > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "eq table too large");
    if (dev) {
        if (!dev_scalar_ok(v) || (n_y && !dev_scalar_ok(y))) return set_error(TSTWO_ERR_BAD_ARG, "eq table: null or misaligned device scalar");
    } else if (!v || (n_y && !y)) {
        return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    }
    TSTWO_REQUIRE_TABLE(out, 4);
    EqY ys{};
    qm31 vq{};
    if (!dev) {
        for (u32 k = 0; k < n_y; k++) ys.y[k] = to_q(y + 4 * k);
        vq = to_q(v);
    }
    const u32 lo = n_y / 2, hi = n_y - lo, nt = (1u << hi) + (1u << lo);
    if (int rc = ensure_scratch(kTabOff + (size_t)nt * sizeof(qm31))) return rc;
    qm31 *tab = (qm31 *)((uint8_t *)ctx().scratch + kTabOff);
    hipLaunchKernelGGL(k_eq_tables, dim3(ceil_div(nt, kThreads)), dim3(kThreads), 0, ctx().stream, ys, vq, dev ? y : nullptr, dev ? v : nullptr,
                       hi, lo, tab);
    TSTWO_LAUNCH_CHECK();
    const Soa4 o = soa(out);
    const u32 n = 1u << n_y;
    if (lo >= 2 && all_aligned16(o)) hipLaunchKernelGGL(k_eq_expand<4>, dim3(grid_for(n / 4, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    else hipLaunchKernelGGL(k_eq_expand<1>, dim3(grid_for(n, 32)), dim3(kThreads), 0, ctx().stream, tab, hi, lo, o);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

int launch_next_layer(u32 kind, const u32 *const num[4], const u32 *const den[4], u32 log_n, u32 *const onum[4], u32 *const oden[4]) {
    const u32 n_out = 1u << (log_n - 1);
    const dim3 g(grid_for(n_out, 32)), b(kThreads);
    const CSoa4 d = csoa(den);
    const Soa4 od = soa(oden);
    hipStream_t st = ctx().stream;
    switch (kind) {
        case TSTWO_GKR_GRAND_PRODUCT: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_GRAND_PRODUCT>, g, b, 0, st, CSoa4{}, d, Soa4{}, od, n_out); break;
        case TSTWO_GKR_LOGUP_GENERIC: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_GENERIC>, g, b, 0, st, csoa(num), d, soa(onum), od, n_out); break;
        case TSTWO_GKR_LOGUP_MULTIPLICITIES:
            hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_MULTIPLICITIES>, g, b, 0, st, csoa1(num[0]), d, soa(onum), od, n_out);
            break;
        default: hipLaunchKernelGGL(k_next_layer<TSTWO_GKR_LOGUP_SINGLES>, g, b, 0, st, CSoa4{}, d, soa(onum), od, n_out); break;
    }
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // namespace tstwo

extern "C" {

int tstwo_gkr_gen_eq_evals(const u32 *y, u32 n_y, const u32 v[4], u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    return eq_evals(y, n_y, v, false, out);
}

int tstwo_gkr_next_layer_grand_product(const u32 *const in[4], u32 log_n, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    if (log_n == 0) return set_error(TSTWO_ERR_BAD_ARG, "next_layer of an output layer");
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "GKR layer too large");
    TSTWO_REQUIRE_TABLE(in, 4); TSTWO_REQUIRE_TABLE(out, 4);
    return launch_next_layer(TSTWO_GKR_GRAND_PRODUCT, nullptr, in, log_n, nullptr, out);
}

int tstwo_gkr_next_layer_logup(u32 kind, const u32 *const num[4], const u32 *const den[4], u32 log_n, u32 *const out_num[4],
                               u32 *const out_den[4]) {
    TSTWO_REQUIRE_READY();
    if (kind < TSTWO_GKR_LOGUP_GENERIC || kind > TSTWO_GKR_LOGUP_SINGLES) return set_error(TSTWO_ERR_BAD_ARG, "unknown LogUp numerator kind");
    if (log_n == 0) return set_error(TSTWO_ERR_BAD_ARG, "next_layer of an output layer");
    if (log_n > kMaxLog) return set_error(TSTWO_ERR_BAD_ARG, "GKR layer too large");
    TSTWO_REQUIRE_TABLE(den, 4); TSTWO_REQUIRE_TABLE(out_num, 4); TSTWO_REQUIRE_TABLE(out_den, 4);
    if (kind == TSTWO_GKR_LOGUP_GENERIC) TSTWO_REQUIRE_TABLE(num, 4);
    if (kind == TSTWO_GKR_LOGUP_MULTIPLICITIES) TSTWO_REQUIRE_TABLE(num, 1);
    return launch_next_layer(kind, num, den, log_n, out_num, out_den);
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
    if (int rc = gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, lambda, nullptr, dst, false)) return rc;
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
    return gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, lambda, nullptr, out_dev, false);
}

int tstwo_gkr_round(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const out_num[4],
                    u32 *const out_den[4], u32 n_vars, const u32 r[4], const u32 lambda[4], u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev);
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, r, nullptr, lambda, nullptr, out_dev, true);
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
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, nullptr, r_dev, lambda, nullptr, out_dev, true);
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
    return eq_evals(y_dev, n_y, v_dev, true, out);
}

int tstwo_gkr_sum_poly_async_ldev(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 n_vars,
                                  const u32 *lambda_dev, u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev, lambda_dev);
    return gkr_sum(kind, eq, num, den, nullptr, nullptr, n_vars, nullptr, nullptr, nullptr, lambda_dev, out_dev, false);
}

int tstwo_gkr_round_dev_ldev(u32 kind, const u32 *const eq[4], const u32 *const num[4], const u32 *const den[4], u32 *const out_num[4],
                             u32 *const out_den[4], u32 n_vars, const u32 *r_dev, const u32 *lambda_dev, u32 *out_dev) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_PTRS(out_dev, r_dev, lambda_dev);
    return gkr_sum(kind, eq, num, den, out_num, out_den, n_vars, nullptr, r_dev, nullptr, lambda_dev, out_dev, true);
}

}  // extern "C"

// gkr_transcript.hip — the O(instances) parts of a GKR proof, each by ONE wave, so that prove_batch is enqueued without a read-back:
//   round finish    k_gkr_round_finish: the end of a sum-check round — round polynomials, combination, Blake2s channel mix + draw,
//                   new claims.  y_k, inv_eq0 and alpha come by value or from device words (tstwo_gkr_round_finish_dev).
//   layer begin/end k_gkr_layer_begin, k_gkr_layer_end: what the host does around a layer's sum-check (claims, lambda, masks).
// The streaming ops are in gkr_ops.hip, the one-call proof that chains all of them in gkr_prove.hip.
#include "gkr_internal.h"
#include "blake2s.cuh"

using namespace tstwo;

namespace {

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
    const u32 *y_dev, *a_dev, *alpha_dev;    // non-null = that scalar is read from these 4 device words instead (scalar_q)
    u32 *poly_out, *ch_out;
    u32 *status;                             // non-null = a degenerate y sets kStatusDegenerate here (the host checked it otherwise)
};
__device__ __forceinline__ bool q_eq_m31(qm31 v, u32 a) { return v.a == a && (v.b | v.c | v.d) == 0u; }
// y = 1/2: b is undefined; y = 1, 0, 1/3: b = 0, 1, 2 collides with an interpolation point
__device__ __forceinline__ bool degenerate_y(qm31 y) { return q_eq_m31(y, 0u) || q_eq_m31(y, 1u) || q_eq_m31(y, 1u << 30) || q_eq_m31(y, 0x55555555u); }
__device__ __forceinline__ uint4 u4_of(qm31 v) { return make_uint4(v.a, v.b, v.c, v.d); }

__global__ void __launch_bounds__(64) k_gkr_round_finish(FinishArgs f) {
    using namespace b2s;
    const u32 lane = threadIdx.x;
    const bool in = lane < f.n, act = in && ((f.mask >> lane) & 1u);
    const qm31 zero = {0u, 0u, 0u, 0u}, one = {1u, 0u, 0u, 0u};
    constexpr u32 kHalf = 1u << 30;                                   // 1/2 in M31
    const qm31 y = scalar_q(f.y, f.y_dev), a = scalar_q(f.a, f.a_dev), alpha = scalar_q(f.alpha, f.alpha_dev);
    // the round still finishes (every loop below is bounded and the inversion is a fixed power chain); its outputs mean nothing
    if (f.status && lane == 0 && degenerate_y(y)) __hip_atomic_fetch_or(f.status, kStatusDegenerate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // requested first: the channel words are needed last
    u32 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = gload1(f.chan, k);
    u32 n_chal = gload1(f.chan, 8), n_sent = gload1(f.chan, 9);
    qm31 claim = zero, corr = zero, f0 = zero, f2 = zero;
    if (in) { claim = q_of(gload4(f.state, 8 * lane)); corr = q_of(gload4(f.state, 8 * lane + 4)); }
    if (act) { f0 = q_of(gload4(f.sums, 8 * lane)); f2 = q_of(gload4(f.sums, 8 * lane + 4)); }

    // wave-uniform: D = 1 - 2y, 1/y and 1/D from one inversion, b, A = a D
    const qm31 one_y = qm31_sub(one, y), D = qm31_sub(one_y, y);
    const qm31 inv_yd = qm31_inv(qm31_mul(y, D));
    const qm31 inv_y = qm31_mul(inv_yd, D), inv_d = qm31_mul(inv_yd, y);
    const qm31 b = qm31_mul(one_y, inv_d), A = qm31_mul(a, D);

    // lane i: the coefficients of p_i
    qm31 c0, c1 = zero, c2 = zero, c3 = zero;
    if (act) {
        const qm31 ca = qm31_mul(corr, A);
        const qm31 g0 = qm31_mul(f0, ca), g2 = qm31_mul(f2, ca);
        const qm31 w0 = qm31_neg(qm31_mul_m31(g0, kHalf)), w2 = qm31_neg(qm31_mul_m31(g2, kHalf));
        const qm31 w1 = qm31_mul(qm31_sub(qm31_mul(claim, D), qm31_mul(g0, one_y)), inv_y);
        const qm31 q2 = qm31_add(qm31_add(w0, w1), w2);
        const qm31 w01 = qm31_add(w0, w1);                            // q1 = -(3 w0 + 2 w1 + w2) = -(w0 + (w0 + w1) + q2)
        const qm31 q1 = qm31_neg(qm31_add(qm31_add(w0, w01), q2));
        c0 = qm31_mul(b, g0);                                         // -b q0, q0 = 2 w0 = -g0
        c1 = qm31_sub(qm31_neg(g0), qm31_mul(b, q1));
        c2 = qm31_sub(q1, qm31_mul(b, q2));
        c3 = q2;
    } else {
        c0 = qm31_mul_m31(claim, kHalf);                              // the constant claim / 2 (zero beyond the instances)
    }

    // rp = sum_i alpha^i p_i (sumcheck.ts combine): alpha^lane by square and multiply, then a sum over the wave
    qm31 pw = one, sq = alpha;
#pragma unroll 1
    for (u32 k = 0; ((f.n - 1) >> k) != 0; k++) {
        if ((lane >> k) & 1u) pw = qm31_mul(pw, sq);
        sq = qm31_mul(sq, sq);
    }
    u32 rp[16];
    {
        const qm31 t0 = qm31_mul(c0, pw);
        qm31 t1 = zero, t2 = zero, t3 = zero;
        if (act) { t1 = qm31_mul(c1, pw); t2 = qm31_mul(c2, pw); t3 = qm31_mul(c3, pw); }
        rp[0] = t0.a; rp[1] = t0.b; rp[2] = t0.c; rp[3] = t0.d; rp[4] = t1.a; rp[5] = t1.b; rp[6] = t1.c; rp[7] = t1.d;
        rp[8] = t2.a; rp[9] = t2.b; rp[10] = t2.c; rp[11] = t2.d; rp[12] = t3.a; rp[13] = t3.b; rp[14] = t3.c; rp[15] = t3.d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 16; k++) rp[k] = m31_add(rp[k], (u32)__shfl_xor((int)rp[k], off, 64));
#pragma unroll
    for (int k = 0; k < 16; k++) rp[k] = (u32)__builtin_amdgcn_readfirstlane((int)rp[k]);
    u32 n_coeffs = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (rp[4 * j] | rp[4 * j + 1] | rp[4 * j + 2] | rp[4 * j + 3]) n_coeffs = j + 1;

    // mix_felts(rp.coeffs[:n_coeffs]): the words of the trimmed coefficients are zero
    chan_mix_felts(d, n_chal, n_sent, rp, n_coeffs);
    u32 felt[4] = {0u, 0u, 0u, 0u};
    chan_mix_draw(d, n_chal, n_sent, nullptr, false, true, felt);
    const qm31 ch = {felt[0], felt[1], felt[2], felt[3]};

    // claim_i <- p_i(ch); corr_i <- corr_i eq(ch, y) for the active instances
    if (in) {
        qm31 v = c0;
        if (act) {
            v = qm31_add(qm31_mul(qm31_add(qm31_mul(qm31_add(qm31_mul(c3, ch), c2), ch), c1), ch), c0);
            const qm31 e = qm31_add(qm31_mul(ch, y), qm31_mul(qm31_sub(one, ch), one_y));
            gstore4(f.state, 8 * lane + 4, u4_of(qm31_mul(corr, e)));
        }
        gstore4(f.state, 8 * lane, u4_of(v));
    }
    if (lane == 0) {
        gstore4(f.poly_out, 0, make_uint4(n_coeffs, 0u, 0u, 0u));
#pragma unroll
        for (int j = 0; j < 4; j++) gstore4(f.poly_out, 4 + 4 * j, make_uint4(rp[4 * j], rp[4 * j + 1], rp[4 * j + 2], rp[4 * j + 3]));
        gstore4(f.ch_out, 0, u4_of(ch));
#pragma unroll
        for (int k = 0; k < 8; k++) gstore1(f.chan, k, d[k]);
        gstore1(f.chan, 8, n_chal);
        gstore1(f.chan, 9, n_sent);
    }
}

// ---------------------------------------------------------------- the top and the bottom of a layer (gkr_prover.ts:452-500, 540-575)
// What prove_batch's host loop does around a layer's sum-check, by ONE wave each: lane j owns the j-th active instance (a
// tstwo_gkr_lane in device memory); the channel is wave-uniform.  The mixes of a layer are a serial hash chain by the definition
// of the transcript: lane j's felts are broadcast and every lane runs the same compression, as k_gkr_round_finish does.
typedef const TSTWO_GLOBAL tstwo_gkr_lane *lane_ptr;
__device__ __forceinline__ qm31 bcast_q(qm31 v, u32 j) {
    return {(u32)__shfl((int)v.a, (int)j, 64), (u32)__shfl((int)v.b, (int)j, 64), (u32)__shfl((int)v.c, (int)j, 64), (u32)__shfl((int)v.d, (int)j, 64)};
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
        const qm31 f0 = bcast_q(c0, j), f1 = bcast_q(c1, j);
        const u32 w[8] = {f0.a, f0.b, f0.c, f0.d, f1.a, f1.b, f1.c, f1.d};
        const u32 nf = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)n_felts, (int)j, 64));
        chan_mix_felts(d, n_chal, n_sent, w, nf);
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
        const qm31 f0 = bcast_q(a0, j), f1 = bcast_q(b0, j), f2 = bcast_q(a1, j), f3 = bcast_q(b1, j);
        const u32 w[16] = {f0.a, f0.b, f0.c, f0.d, f1.a, f1.b, f1.c, f1.d, f2.a, f2.b, f2.c, f2.d, f3.a, f3.b, f3.c, f3.d};
        const u32 nf = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)n_felts, (int)j, 64));
        chan_mix_felts(d, n_chal, n_sent, w, nf);
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

}  // namespace

namespace tstwo {

int round_finish(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 *y, const u32 *a, const u32 *alpha,
                 bool dev, u32 *round_poly_out, u32 *challenge_out, u32 *status) {
    TSTWO_REQUIRE_PTRS(chan, sums, state, round_poly_out, challenge_out);
    if (dev) TSTWO_REQUIRE_PTRS(status);
    else if (!y || !a || !alpha) return set_error(TSTWO_ERR_BAD_ARG, "null host argument");
    if (n_instances == 0 || n_instances > 64) return set_error(TSTWO_ERR_BAD_ARG, "sum-check: 1 to 64 instances per round");
    if (((uintptr_t)chan & 3) || ((uintptr_t)status & 3) || !aligned16(sums) || !aligned16(state) || !aligned16(round_poly_out) ||
        !aligned16(challenge_out))
        return set_error(TSTWO_ERR_BAD_ARG, "sum-check: misaligned device pointer");
    FinishArgs f{};
    if (dev) {
        if (!dev_scalar_ok(y) || !dev_scalar_ok(a) || !dev_scalar_ok(alpha))
            return set_error(TSTWO_ERR_BAD_ARG, "sum-check: null or misaligned device scalar");
        f.y_dev = y; f.a_dev = a; f.alpha_dev = alpha;
    } else {
        // y_k = 1/2: b is undefined; y_k = 1, 0, 1/3: b = 0, 1, 2 collides with an interpolation point
        if (q_is(y, 0u) || q_is(y, 1u) || q_is(y, 1u << 30) || q_is(y, 0x55555555u))
            return set_error(TSTWO_ERR_BAD_ARG, "sum-check: degenerate eq point");
        f.y = to_q(y); f.a = to_q(a); f.alpha = to_q(alpha);
    }
    f.chan = chan; f.sums = sums; f.state = state; f.n = n_instances;
    f.mask = n_instances == 64 ? active_mask : active_mask & ((1ull << n_instances) - 1);
    f.poly_out = round_poly_out; f.ch_out = challenge_out; f.status = status;
    hipLaunchKernelGGL(k_gkr_round_finish, dim3(1), dim3(64), 0, ctx().stream, f);
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

}  // namespace tstwo

extern "C" {

int tstwo_gkr_round_finish(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 y_k[4],
                           const u32 inv_eq0[4], const u32 alpha[4], u32 *round_poly_out, u32 *challenge_out) {
    TSTWO_REQUIRE_READY();
    return round_finish(chan, sums, state, n_instances, active_mask, y_k, inv_eq0, alpha, false, round_poly_out, challenge_out, nullptr);
}

int tstwo_gkr_round_finish_dev(u32 *chan, const u32 *sums, u32 *state, u32 n_instances, uint64_t active_mask, const u32 *y_k_dev,
                               const u32 *inv_eq0_dev, const u32 *alpha_dev, u32 *round_poly_out, u32 *challenge_out, u32 *status) {
    TSTWO_REQUIRE_READY();
    return round_finish(chan, sums, state, n_instances, active_mask, y_k_dev, inv_eq0_dev, alpha_dev, true, round_poly_out, challenge_out, status);
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

}  // extern "C"

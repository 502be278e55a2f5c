// fri.hip — FriOps: the fold kernels (fold_line, fold_circle_into_line), k_line_interpolate, decompose, the fold entries and
// FriProver.commit's layer loop (tstwo_fri_commit_layers; its schedule is fri_plan.h).  PolyOps.eval_at_point is poly_eval.hip.
//
// A FRI fold is one inverse-CFFT layer followed by f0 + alpha*f1: the per-output
// twiddle domain.at(bitrev(2i)).x^-1 (resp. .y^-1) that the reference recomputes per element with a
// scalar multiplication and a Fermat inverse (fri.ts:138-141,180-183) is a slice of the inverse
// twiddle tree.  One lane per output row on SoA QM31 (4 coalesced 8-byte loads, 4 coalesced stores).
// Algorithmic bytes per output row: fold_line 48 (32 in + 16 out), fold_circle_into_line 64
// (32 src + 16 dst in + 16 dst out).
#include <string.h>
#include <vector>

#include "common.h"
#include "fri_plan.h"

using namespace tstwo;

namespace {

__device__ __forceinline__ qm31 load_pair_fold(const CSoa4 &in, size_t i, u32 t, qm31 *f0_out) {
    // (f0, f1) = ibutterfly(in[2i], in[2i+1], t) per coordinate (fft.ts:25-30)
    uint2 a = gload2(in.p[0] + 2 * i);
    uint2 b = gload2(in.p[1] + 2 * i);
    uint2 c = gload2(in.p[2] + 2 * i);
    uint2 d = gload2(in.p[3] + 2 * i);
    *f0_out = {m31_add(a.x, a.y), m31_add(b.x, b.y), m31_add(c.x, c.y), m31_add(d.x, d.y)};
    qm31 diff = {m31_sub(a.x, a.y), m31_sub(b.x, b.y), m31_sub(c.x, c.y), m31_sub(d.x, d.y)};
    return qm31_mul_m31(diff, t);
}

// fri.ts:120-152.  inv_x[i] = domain.at(bitrev(2i)).x^-1.
__global__ void __launch_bounds__(256) k_fold_line(CSoa4 in, Soa4 out, size_t n_out, const u32 *__restrict__ inv_x, qm31 alpha,
                                                  const qm31 *__restrict__ alpha_dev) {
    if (alpha_dev) alpha = *alpha_dev;          // alpha drawn by the device channel (uniform load)
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
        qm31 f0;
        qm31 f1 = load_pair_fold(in, i, inv_x[i], &f0);
        qm31 r = qm31_add(f0, qm31_mul(alpha, f1));
        out.p[0][i] = r.a; out.p[1][i] = r.b; out.p[2][i] = r.c; out.p[3][i] = r.d;
    }
}

// fri.ts:162-192.  Twiddle = circle-layer inverse twiddle: either explicit inv_y[i], or derived from the
// layer-1 slice of the inverse tree: +-seg1[(i>>1)^1], negative iff (i ^ (i>>1)) & 1.
// ACCUM = false: dst is written, not updated (dst = alpha f1 + f0) — the first fold of a FRI commit, whose line evaluation starts
// at zero (fri.ts:687-693): no zero fill of dst, no read of it.
template <bool FROM_TREE, bool ACCUM = true>
__global__ void __launch_bounds__(256) k_fold_circle(Soa4 dst, CSoa4 src, size_t n_out, const u32 *__restrict__ twp,
                                                    qm31 alpha, qm31 alpha_sq, const qm31 *__restrict__ alpha_dev) {
    if (alpha_dev) { alpha = *alpha_dev; if (ACCUM) alpha_sq = qm31_mul(alpha, alpha); }
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
        u32 t;
        if (FROM_TREE) {
            t = twp[(i >> 1) ^ 1];
            if ((i ^ (i >> 1)) & 1) t = m31_neg(t);
        } else {
            t = twp[i];
        }
        qm31 f0;
        qm31 f1 = load_pair_fold(src, i, t, &f0);
        qm31 fp = qm31_add(qm31_mul(alpha, f1), f0);
        qm31 r = fp;
        if (ACCUM) {
            qm31 cur = {dst.p[0][i], dst.p[1][i], dst.p[2][i], dst.p[3][i]};
            r = qm31_add(qm31_mul(cur, alpha_sq), fp);
        }
        dst.p[0][i] = r.a; dst.p[1][i] = r.b; dst.p[2][i] = r.c; dst.p[3][i] = r.d;
    }
}

// Two consecutive output rows per lane: 16-byte loads of the source, 8-byte accesses of dst (log 24: 94.2 against 96.7 us for the
// one-row form; needs 16-byte aligned source columns and 8-byte aligned dst columns, tree twiddles).
template <bool ACCUM>
__global__ void __launch_bounds__(256) k_fold_circle2(Soa4 dst, CSoa4 src, size_t n_out, const u32 *__restrict__ twp,
                                                     qm31 alpha, qm31 alpha_sq, const qm31 *__restrict__ alpha_dev) {
    if (alpha_dev) { alpha = *alpha_dev; if (ACCUM) alpha_sq = qm31_mul(alpha, alpha); }
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_out / 2; j += stride) {
        // rows i = 2j, 2j + 1 share the twiddle twp[j ^ 1] up to sign: negative iff (i ^ (i >> 1)) & 1
        const u32 tw = twp[j ^ 1];
        const u32 t0 = (j & 1) ? m31_neg(tw) : tw, t1 = (j & 1) ? tw : m31_neg(tw);
        const uint4 a = gload4(src.p[0] + 4 * j), b = gload4(src.p[1] + 4 * j), c = gload4(src.p[2] + 4 * j), d = gload4(src.p[3] + 4 * j);
        uint2 cur[4];
        if (ACCUM) {
#pragma unroll
            for (int k = 0; k < 4; k++) cur[k] = gload2(dst.p[k] + 2 * j);
        }
        qm31 r[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u32 ax = h ? a.z : a.x, ay = h ? a.w : a.y, bx = h ? b.z : b.x, by = h ? b.w : b.y;
            const u32 cx = h ? c.z : c.x, cy = h ? c.w : c.y, dx = h ? d.z : d.x, dy = h ? d.w : d.y;
            const qm31 f0 = {m31_add(ax, ay), m31_add(bx, by), m31_add(cx, cy), m31_add(dx, dy)};
            const qm31 f1 = qm31_mul_m31({m31_sub(ax, ay), m31_sub(bx, by), m31_sub(cx, cy), m31_sub(dx, dy)}, h ? t1 : t0);
            r[h] = qm31_add(qm31_mul(alpha, f1), f0);
            if (ACCUM) {
                const qm31 cu = {h ? cur[0].y : cur[0].x, h ? cur[1].y : cur[1].x, h ? cur[2].y : cur[2].x, h ? cur[3].y : cur[3].x};
                r[h] = qm31_add(qm31_mul(cu, alpha_sq), r[h]);
            }
        }
        *(TSTWO_GLOBAL u32x2_t *)(dst.p[0] + 2 * j) = u32x2_t{r[0].a, r[1].a};
        *(TSTWO_GLOBAL u32x2_t *)(dst.p[1] + 2 * j) = u32x2_t{r[0].b, r[1].b};
        *(TSTWO_GLOBAL u32x2_t *)(dst.p[2] + 2 * j) = u32x2_t{r[0].c, r[1].c};
        *(TSTWO_GLOBAL u32x2_t *)(dst.p[3] + 2 * j) = u32x2_t{r[0].d, r[1].d};
    }
}

// (A form with a lane owning 4 consecutive output rows — every access 16 bytes per lane instead of 8 / 4 — was built and
// measured in round 3: fold_circle_into_line log 24 103.9 against 106.7 us, fold_line log 23 37.9 against 35.3 us: the
// folds already move 5.0 - 5.9 TB/s and the 120 VGPRs of the 4-row form cost as much occupancy as the wider accesses
// gain.  Removed; gpurun_out/r03b/f1.log.)
// LineEvaluation.interpolate (poly/line.ts:312-329) with lineIfft (line.ts:354-390) for a layer that fits one workgroup's LDS — the
// last FRI layer (2^7 rows by default): bit reversal on the way in, log_n levels of ibutterflies with x^-1 =
// domain.at(i)^-1 taken from the inverse twiddle tree (level of coset size 2^k: itw_end - 2^k + bitrev(i, k - 1)), the 1/n
// scaling, coefficients out in the reference's bit-reversed order.  One workgroup, coordinate c of a value handled like a
// column (every twiddle is in the base field).
__global__ void __launch_bounds__(256) k_line_interpolate(CSoa4 in, Soa4 out, u32 log_n, const u32 *__restrict__ itw_end, u32 n_inv) {
    extern __shared__ u32 lsh[];                 // [4][n]
    const u32 n = 1u << log_n, t = threadIdx.x;
    for (u32 i = t; i < 4 * n; i += 256) {
        const u32 c = i >> log_n, j = i & (n - 1);
        const u32 nat = log_n ? __brev(j) >> (32 - log_n) : 0u;
        lsh[(c << log_n) + nat] = gload1(in.p[c] + j);
    }
    __syncthreads();
    for (u32 k = log_n; k >= 1; k--) {                              // chunks of 2^k values
        const u32 half = 1u << (k - 1);
        for (u32 w = t; w < 2 * n; w += 256) {                      // 4 coordinates x n/2 butterflies
            const u32 c = w >> (log_n - 1), b = w & ((n >> 1) - 1);
            const u32 i = b & (half - 1), chunk = b >> (k - 1);
            const u32 l = (c << log_n) + (chunk << k) + i, r = l + half;
            const u32 br = k > 1 ? __brev(i) >> (32 - (k - 1)) : 0u;
            const u32 x_inv = itw_end[(int)br - (int)(1u << k)];
            const u32 a = lsh[l], bb = lsh[r];
            lsh[l] = m31_add(a, bb);                                  // ibutterfly (fft.ts:25-30)
            lsh[r] = m31_mul(m31_sub(a, bb), x_inv);
        }
        __syncthreads();
    }
    for (u32 i = t; i < 4 * n; i += 256) gstore1(out.p[i >> log_n] + (i & (n - 1)), m31_mul(lsh[i], n_inv));
}

// backend/cpu/fri.ts:97-123: sums of the two halves of each coordinate column (exact in u64).
// VEC: 16-byte loads (columns 16-byte aligned, halves a multiple of 4 words).
template <bool VEC>
__global__ void __launch_bounds__(256) k_half_sums(CSoa4 in, size_t n, unsigned long long *sums /* [4][2] */) {
    __shared__ unsigned long long sh[256 / 64];
    const u32 coord = blockIdx.y, halfsel = blockIdx.z;
    const size_t half = n / 2;
    const u32 *p = in.p[coord] + (halfsel ? half : 0);
    const size_t cnt = halfsel ? n - half : half;
    unsigned long long acc = 0;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    if (VEC) {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt / 4; i += stride) {
            const uint4 v = gload4(p + 4 * i);
            acc += (unsigned long long)v.x + v.y + ((unsigned long long)v.z + v.w);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += stride) acc += p[i];
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = sh[0] + sh[1] + sh[2] + sh[3];
        atomicAdd(&sums[coord * 2 + halfsel], tot);
    }
}
// backend/cpu/fri.ts:133-164: g = f - lambda on the first half, f + lambda on the second (n == 1: f - lambda)
template <bool VEC>
__global__ void __launch_bounds__(256) k_decompose_apply(CSoa4 in, Soa4 out, size_t n, qm31 lambda) {
    const u32 coord = blockIdx.y;
    const u32 lam = coord == 0 ? lambda.a : coord == 1 ? lambda.b : coord == 2 ? lambda.c : lambda.d;
    const size_t half = n / 2;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    if (VEC) {              // n >= 8: the 4 words of a vector lie in one half
        const u32 nlam = m31_neg(lam);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            const uint4 v = gload4(in.p[coord] + 4 * i);
            const u32 add = 4 * i < half ? nlam : lam;          // f - lambda = f + (-lambda)
            gstore4(out.p[coord] + 4 * i, make_uint4(m31_add(v.x, add), m31_add(v.y, add), m31_add(v.z, add), m31_add(v.w, add)));
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            u32 v = in.p[coord][i];
            out.p[coord][i] = (i < half || n == 1) ? m31_sub(v, lam) : m31_add(v, lam);
        }
    }
}

unsigned capped_blocks(size_t work_items, unsigned threads) {
    unsigned blocks = ceil_div(work_items, threads);
    const unsigned mult = (unsigned)knobs().fold_cap;     // workgroups per CU before lanes grid-stride (8: fold_circle log 24 102 us, fold_line log 23 33.5 us; 32-1024: 97 / 32.5 us)
    unsigned cap = (unsigned)ctx().n_cus * mult;
    if (blocks > cap) blocks = cap;
    return blocks ? blocks : 1;
}

static void launch_fold_line(const CSoa4 &i4, const Soa4 &o4, size_t n_out, const u32 *inv_x, qm31 alpha, const qm31 *alpha_dev) {
    // (a two-rows-per-lane form with 16-byte loads, as in k_fold_circle2, measured the same 6.2-6.4 TB/s: not kept)
    hipLaunchKernelGGL(k_fold_line, dim3(capped_blocks(n_out, 256)), dim3(256), 0, ctx().stream, i4, o4, n_out, inv_x, alpha, alpha_dev);
}
// accum = false (dst written, not updated: the first fold of tstwo_fri_commit_layers) exists with tree twiddles only
static void launch_fold_circle(bool from_tree, bool accum, const Soa4 &d4, const CSoa4 &s4, size_t n_out, const u32 *twp, qm31 a, qm31 a2,
                               const qm31 *alpha_dev) {
    bool two = from_tree && n_out >= 4;
    for (int k = 0; k < 4; k++) two = two && (((uintptr_t)s4.p[k]) & 15) == 0 && (((uintptr_t)d4.p[k]) & 7) == 0;
    const dim3 g2(capped_blocks(n_out / 2, 256)), g1(capped_blocks(n_out, 256));
    hipStream_t st = ctx().stream;
    if (two && accum) hipLaunchKernelGGL(k_fold_circle2<true>, g2, dim3(256), 0, st, d4, s4, n_out, twp, a, a2, alpha_dev);
    else if (from_tree && accum) hipLaunchKernelGGL(k_fold_circle<true>, g1, dim3(256), 0, st, d4, s4, n_out, twp, a, a2, alpha_dev);
    else if (!from_tree) hipLaunchKernelGGL(k_fold_circle<false>, g1, dim3(256), 0, st, d4, s4, n_out, twp, a, a2, alpha_dev);
    else if (two) hipLaunchKernelGGL(k_fold_circle2<false>, g2, dim3(256), 0, st, d4, s4, n_out, twp, a, a2, alpha_dev);
    else hipLaunchKernelGGL((k_fold_circle<true, false>), g1, dim3(256), 0, st, d4, s4, n_out, twp, a, a2, alpha_dev);
}

// ---- one checked path per fold.  An input with several defects reports the first of: library not ready, null pointers, size,
// twiddles, shard, alpha alignment.
struct FoldRows { size_t offset, n; };                 // row shard (contiguous row sharding of FRI layers, no exchange): the
                                                       // pointers address this shard's rows only, log_n is the WHOLE layer's size, the
                                                       // shard produces output rows [offset, offset + n)
struct FoldTwiddles { const u32 *p; bool tree; u32 tw_log; };       // the slice the kernel reads, or (tree) the inverse twiddle tree
struct FoldAlpha { const u32 *p; bool dev; };          // 4 host words, or 16-byte aligned device words (written by the device channel on
                                                       // the same stream: a commit needs no host round trip between a tree and the next fold)

int check_shard(const char *fn, u32 log_n, const FoldRows &r) {
    size_t n_out = (size_t)1 << (log_n - 1);
    if (r.n == 0 || r.offset + r.n > n_out || (r.offset & 3) || ((r.n & 3) && r.n != n_out)) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: shard rows [%zu, +%zu) must be 4-aligned and lie inside the %zu output rows", fn, r.offset, r.n, n_out);
        return set_error(TSTWO_ERR_BAD_ARG, buf);
    }
    return TSTWO_OK;
}

int fold_line(const u32 *const in[4], u32 log_n, const FoldRows *rows, FoldTwiddles tw, FoldAlpha alpha, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_TABLE(in, 4); TSTWO_REQUIRE_TABLE(out, 4); TSTWO_REQUIRE_PTRS(tw.p, alpha.p);
    if (log_n == 0) return set_error(TSTWO_ERR_TOO_SMALL, "fold_line: Evaluation too small, must have at least 2 elements.");
    // the upper bound of the size stands behind the twiddle check: a layer of log_n > 31 lies beyond every tree, and the tree entries
    // have always answered that with the twiddle error; only an explicit slice gets as far as the range error
    if (tw.tree && (tw.tw_log > 31 || log_n > tw.tw_log)) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");
    if (log_n > 31) return set_error(TSTWO_ERR_BAD_ARG, "fold_line: log size out of range");
    if (rows)
        if (int rc = check_shard("fold_line_rows", log_n, *rows)) return rc;
    if (alpha.dev && !aligned16(alpha.p)) return set_error(TSTWO_ERR_BAD_ARG, "fold: alpha must be 16-byte aligned");
    // level of the tree whose coset has log size log_n: 2^(log_n-1) entries starting 2^log_n before the end
    const u32 *inv_x = (tw.tree ? tw.p + ((size_t)1 << tw.tw_log) - ((size_t)1 << log_n) : tw.p) + (rows ? rows->offset : 0);
    CSoa4 i4 = {{in[0], in[1], in[2], in[3]}};
    Soa4 o4 = {{out[0], out[1], out[2], out[3]}};
    launch_fold_line(i4, o4, rows ? rows->n : (size_t)1 << (log_n - 1), inv_x, alpha.dev ? qm31{0, 0, 0, 0} : to_q(alpha.p),
                     alpha.dev ? (const qm31 *)alpha.p : nullptr);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// dst_len: the rows of dst as the caller states them (whole layers only; a shard states its rows in `rows`)
int fold_circle(u32 *const dst[4], size_t dst_len, const u32 *const src[4], u32 log_n, const FoldRows *rows, FoldTwiddles tw, FoldAlpha alpha,
                bool accum = true) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_TABLE(dst, 4); TSTWO_REQUIRE_TABLE(src, 4); TSTWO_REQUIRE_PTRS(tw.p, alpha.p);
    if (rows) {
        if (log_n < 3 || log_n > 31) return set_error(TSTWO_ERR_BAD_ARG, "fold_circle_into_line_rows: log_n must be in [3, 31]");
    } else {
        if (log_n == 0 || log_n > 31 || (((size_t)1 << log_n) >> 1) != dst_len)
            return set_error(TSTWO_ERR_LEN_MISMATCH, "fold_circle_into_line: Length mismatch between src and dst after considering fold step.");
        if (tw.tree && log_n < 3)
            return set_error(TSTWO_ERR_BAD_ARG, "fold_circle_into_line: log_n < 3 needs explicit twiddles (tstwo_fri_fold_circle_into_line_tw)");
    }
    if (tw.tree && (tw.tw_log > 31 || log_n - 1 > tw.tw_log)) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");
    if (rows)
        if (int rc = check_shard("fold_circle_into_line_rows", log_n, *rows)) return rc;
    if (alpha.dev && !aligned16(alpha.p)) return set_error(TSTWO_ERR_BAD_ARG, "fold: alpha must be 16-byte aligned");
    // the layer-1 slice of the tree, 2^(log_n-2) entries: the kernel reads seg1[(i>>1)^1] with sign (i ^ (i>>1)) & 1, both invariant
    // under a 4-aligned shift of i
    const u32 *twp = tw.tree ? tw.p + ((size_t)1 << tw.tw_log) - ((size_t)1 << (log_n - 1)) + (rows ? rows->offset >> 1 : 0) : tw.p;
    host::Q a = {{0, 0, 0, 0}}, a2 = a;
    if (!alpha.dev) { a = to_hq(alpha.p); a2 = host::qmul(a, a); }
    Soa4 d4 = {{dst[0], dst[1], dst[2], dst[3]}};
    CSoa4 s4 = {{src[0], src[1], src[2], src[3]}};
    launch_fold_circle(tw.tree, accum, d4, s4, rows ? rows->n : dst_len, twp, to_q(a), to_q(a2), alpha.dev ? (const qm31 *)alpha.p : nullptr);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

}  // namespace

// fold_circle with the alpha in device memory, written (accum = false) or accumulated: what a commit loop in another file needs
// (poseidon_coop.hip) and the C ABI does not say — tstwo_fri_fold_circle_into_line_dev always accumulates
int tstwo::fri_fold_circle_dev(u32 *const dst[4], size_t dst_len, const u32 *const src[4], u32 log_n, const u32 *itw, u32 tw_log,
                               const u32 *alpha_dev, bool accum) {
    return fold_circle(dst, dst_len, src, log_n, nullptr, {itw, true, tw_log}, {alpha_dev, true}, accum);
}

extern "C" {

int tstwo_fri_fold_line_tw(const u32 *const in[4], u32 log_n, const u32 *inv_x, const u32 alpha[4], u32 *const out[4]) {
    return fold_line(in, log_n, nullptr, {inv_x, false, 0}, {alpha, false}, out);
}
int tstwo_fri_fold_line(const u32 *const in[4], u32 log_n, const u32 *itw, u32 tw_log, const u32 alpha[4], u32 *const out[4]) {
    return fold_line(in, log_n, nullptr, {itw, true, tw_log}, {alpha, false}, out);
}
int tstwo_fri_fold_line_dev(const u32 *const in[4], u32 log_n, const u32 *itw, u32 tw_log, const u32 *alpha_dev, u32 *const out[4]) {
    return fold_line(in, log_n, nullptr, {itw, true, tw_log}, {alpha_dev, true}, out);
}
int tstwo_fri_fold_line_rows(const u32 *const in[4], u32 log_n, size_t row_offset, size_t n_rows, const u32 *itw, u32 tw_log,
                             const u32 alpha[4], u32 *const out[4]) {
    const FoldRows rows = {row_offset, n_rows};
    return fold_line(in, log_n, &rows, {itw, true, tw_log}, {alpha, false}, out);
}

int tstwo_fri_fold_circle_into_line_tw(u32 *const dst[4], size_t dst_len, const u32 *const src[4], u32 log_n,
                                       const u32 *inv_y, const u32 alpha[4]) {
    return fold_circle(dst, dst_len, src, log_n, nullptr, {inv_y, false, 0}, {alpha, false});
}
int tstwo_fri_fold_circle_into_line(u32 *const dst[4], size_t dst_len, const u32 *const src[4], u32 log_n,
                                    const u32 *itw, u32 tw_log, const u32 alpha[4]) {
    return fold_circle(dst, dst_len, src, log_n, nullptr, {itw, true, tw_log}, {alpha, false});
}
int tstwo_fri_fold_circle_into_line_dev(u32 *const dst[4], size_t dst_len, const u32 *const src[4], u32 log_n, const u32 *itw, u32 tw_log,
                                        const u32 *alpha_dev) {
    return fold_circle(dst, dst_len, src, log_n, nullptr, {itw, true, tw_log}, {alpha_dev, true});
}
int tstwo_fri_fold_circle_into_line_rows(u32 *const dst[4], const u32 *const src[4], u32 log_n, size_t row_offset, size_t n_rows,
                                         const u32 *itw, u32 tw_log, const u32 alpha[4]) {
    const FoldRows rows = {row_offset, n_rows};
    return fold_circle(dst, 0, src, log_n, &rows, {itw, true, tw_log}, {alpha, false});
}

int tstwo_line_interpolate(const u32 *const in[4], u32 log_n, const u32 *itw, u32 tw_log, u32 *const out[4]) {
    TSTWO_REQUIRE_READY();
    TSTWO_REQUIRE_TABLE(in, 4); TSTWO_REQUIRE_TABLE(out, 4);
    if (!itw) return set_error(TSTWO_ERR_BAD_ARG, "null device pointer");
    if (log_n > 12) return set_error(TSTWO_ERR_BAD_ARG, "line_interpolate: at most 2^12 values (one workgroup); larger layers are interpolated by the caller");
    if (tw_log > 31 || log_n > tw_log) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");
    CSoa4 i4 = {{in[0], in[1], in[2], in[3]}};
    Soa4 o4 = {{out[0], out[1], out[2], out[3]}};
    const u32 n_inv = host::inv((u32)1 << log_n);
    hipLaunchKernelGGL(k_line_interpolate, dim3(1), dim3(256), (size_t)16 << log_n, ctx().stream, i4, o4, log_n, itw + ((size_t)1 << tw_log), n_inv);
    TSTWO_LAUNCH_CHECK();
    return TSTWO_OK;
}

// ---- FriProver.commit's layer loop in ONE call (commitInnerLayers, fri.ts:676-716, with the Merkle / channel wiring of the Rust
// text): first-layer tree over every circle column's coordinate columns, then per layer: mix the root and draw alpha on the
// device channel, fold, commit the folded evaluation.  The host-side loop did the same through ~10 C-ABI calls and a dozen
// host objects per layer (40-50 us of host time each, more than the kernels of a layer below 2^16 rows take); here a layer
// costs its launches only.  Everything is enqueued on the library's stream; nothing is read back.
// Which launches an input takes is fri_plan() (fri_plan.h); every argument is checked before the first allocation, so a failed
// check leaves the channel and the alphas as they were.
int tstwo_fri_commit_layers(const u32 *const *circle_cols, const u32 *col_logs, size_t n_columns, const u32 *itw, u32 tw_log,
                            u32 log_last_layer_size, u32 *chan, u32 *alphas, size_t alphas_cap, uint8_t **first_tree,
                            tstwo_fri_layer_out *out, size_t out_cap, size_t *n_out) {
    TSTWO_REQUIRE_READY();
    if (!circle_cols || !col_logs || !first_tree || !out || !n_out) return set_error(TSTWO_ERR_BAD_ARG, "fri commit: null argument");
    *n_out = 0;
    *first_tree = nullptr;
    TSTWO_REQUIRE_TABLE(circle_cols, 4 * n_columns);
    TSTWO_REQUIRE_PTRS(itw, chan, alphas);
    if (!aligned16(alphas)) return set_error(TSTWO_ERR_BAD_ARG, "fold: alpha must be 16-byte aligned");
    std::vector<FriStep> plan;
    if (const char *why = fri_plan(col_logs, n_columns, log_last_layer_size, plan)) return set_error(TSTWO_ERR_BAD_ARG, why);
    const u32 first_log = col_logs[0] - 1;
    const size_t n_inner = first_log - log_last_layer_size;
    if (out_cap < n_inner + 1 || alphas_cap < n_inner + 1) return set_error(TSTWO_ERR_BAD_ARG, "fri commit: output / alpha capacity too small");
    if (tw_log > 31 || first_log > tw_log) return set_error(TSTWO_ERR_TWIDDLES, "Not enough twiddles!");      // bounds every fold's need
    std::vector<void *> owned;                       // everything allocated here, released again if a step fails
    auto fail = [&](int rc) { for (void *p : owned) (void)tstwo_free(p); *first_tree = nullptr; return rc; };
    auto alloc = [&](void **p, size_t bytes) { int rc = tstwo_malloc(p, bytes); if (!rc) owned.push_back(*p); return rc; };
    auto alloc_tree = [&](uint8_t **t, u32 lg) { return alloc((void **)t, tstwo_merkle_layers_bytes(lg)); };
    auto alloc_eval = [&](u32 *cols[4], u32 lg) {
        for (int k = 0; k < 4; k++) { int rc = alloc((void **)&cols[k], sizeof(u32) << lg); if (rc) return rc; }
        return (int)TSTWO_OK;
    };
    u32 *ev[32][4] = {};                             // line layer i: its evaluation and its tree (the last layer has none: it is
    uint8_t *tree[32] = {};                          // interpolated, not committed, fri.ts:718-754)
    const FoldTwiddles tw = {itw, true, tw_log};
    for (const FriStep &s : plan) {
        u32 *const a_in = alphas + 4 * (size_t)s.alpha_in, *const a_out = alphas + 4 * (size_t)s.alpha_out;
        const u32 lg4[4] = {s.log, s.log, s.log, s.log};
        int rc = TSTWO_OK;
        switch (s.kind) {
        case FriStep::FIRST_TREE: {                  // Rust FriFirstLayerProver::new, root -> channel -> alpha_0
            std::vector<u32> logs(4 * n_columns);
            for (size_t i = 0; i < n_columns; i++) for (int k = 0; k < 4; k++) logs[4 * i + k] = col_logs[i];
            if ((rc = alloc_tree(first_tree, s.log))) break;
            rc = merkle_commit_then_channel(circle_cols, logs.data(), 4 * n_columns, *first_tree, chan, a_out, nullptr, nullptr, nullptr);
            break;
        }
        case FriStep::CIRCLE_WRITE:                  // the line evaluation starts at zero (fri.ts:687-693): written, not accumulated — bit-
            // identical to zero-filling it and folding into it (0 * alpha^2 + x = x), without the fill and the read of the zeros
            if ((rc = alloc_eval(ev[s.layer], s.log))) break;
            [[fallthrough]];
        case FriStep::CIRCLE_ACCUM:
            rc = fold_circle(ev[s.layer], (size_t)1 << s.log, circle_cols + 4 * s.column, col_logs[s.column], nullptr, tw, {a_in, true},
                             s.kind == FriStep::CIRCLE_ACCUM);
            break;
        case FriStep::COMMIT:                        // FriInnerLayerProver::new + mix / draw
            if ((rc = alloc_tree(&tree[s.layer], s.log))) break;
            rc = merkle_commit_then_channel(ev[s.layer], lg4, 4, tree[s.layer], chan, a_out, nullptr, nullptr, nullptr);
            break;
        case FriStep::FOLD_COMMIT:                   // the folded row is the leaf message of its tree (merkle_commit_then_channel's fold)
            if ((rc = alloc_eval(ev[s.layer], s.log)) || (rc = alloc_tree(&tree[s.layer], s.log))) break;
            rc = merkle_commit_then_channel(ev[s.layer], lg4, 4, tree[s.layer], chan, a_out, ev[s.layer - 1],
                                            itw + ((size_t)1 << tw_log) - ((size_t)2 << s.log), a_in);
            break;
        case FriStep::FOLD_LINE:
            if ((rc = alloc_eval(ev[s.layer], s.log))) break;
            rc = fold_line(ev[s.layer - 1], s.log + 1, nullptr, tw, {a_in, true}, ev[s.layer]);
            break;
        case FriStep::TAIL:                          // k_fri_tail: tree / mix / draw / fold for every remaining layer
            if (s.pre && (rc = alloc_eval(ev[s.layer], s.log))) break;
            for (u32 i = 0; i < s.n_layers && !rc; i++)
                if (!(rc = alloc_tree(&tree[s.layer + i], s.log - i))) rc = alloc_eval(ev[s.layer + i + 1], s.log - i - 1);
            if (rc) break;
            rc = launch_fri_tail(ev + s.layer, tree + s.layer, s.n_layers, s.log, itw, tw_log, chan, a_out, s.pre ? ev[s.layer - 1] : nullptr,
                                 s.pre ? a_in : nullptr);
            break;
        }
        if (rc) return fail(rc);
    }
    for (size_t i = 0; i <= n_inner; i++) {
        out[i].log_size = first_log - (u32)i;
        for (int k = 0; k < 4; k++) out[i].cols[k] = ev[i][k];
        out[i].layers = tree[i];
    }
    *n_out = n_inner + 1;
    return TSTWO_OK;
}

int tstwo_fri_decompose(const u32 *const in[4], size_t n, u32 *const out[4], u32 lambda[4]) {
    TSTWO_REQUIRE_READY();
    if (n == 0) return set_error(TSTWO_ERR_BAD_ARG, "decompose: empty evaluation");
    TSTWO_REQUIRE_TABLE(in, 4); TSTWO_REQUIRE_TABLE(out, 4); TSTWO_REQUIRE_PTRS(lambda);
    Context &c = ctx();
    int rc = ensure_scratch(64);
    if (rc) return rc;
    unsigned long long *sums = (unsigned long long *)c.scratch;
    TSTWO_HIP(hipMemsetAsync(sums, 0, 8 * sizeof(unsigned long long), c.stream));
    CSoa4 i4 = {{in[0], in[1], in[2], in[3]}};
    Soa4 o4 = {{out[0], out[1], out[2], out[3]}};
    bool vec = n >= 8 && n % 8 == 0;              // both halves whole 16-byte vectors
    for (int k = 0; k < 4; k++) vec = vec && ((((uintptr_t)in[k]) | ((uintptr_t)out[k])) & 15) == 0;
    unsigned blocks = ceil_div(n, 256 * 16);
    if (blocks > 256) blocks = 256;           // (x 4 coordinates x 2 halves; every workgroup ends in one 64-bit atomic on one of 8 words: 4096 of them per word cost 0.25 ms)
    if (blocks == 0) blocks = 1;
    if (vec) hipLaunchKernelGGL(k_half_sums<true>, dim3(blocks, 4, 2), dim3(256), 0, c.stream, i4, n, sums);
    else hipLaunchKernelGGL(k_half_sums<false>, dim3(blocks, 4, 2), dim3(256), 0, c.stream, i4, n, sums);
    TSTWO_LAUNCH_CHECK();
    unsigned long long h[8];
    { int rc2 = small_d2h(h, sums, sizeof(h)); if (rc2) return rc2; }
    // lambda = (a_sum - b_sum) / n  (n == 1: first half empty -> lambda = -f[0])
    u32 n_inv = host::inv((u32)(n % host::P));
    qm31 lam;
    u32 l[4];
    for (int k = 0; k < 4; k++) {
        u32 a = (u32)(h[2 * k] % host::P), b = (u32)(h[2 * k + 1] % host::P);
        l[k] = host::mul(host::sub(a, b), n_inv);
    }
    lam = {l[0], l[1], l[2], l[3]};
    if (vec) hipLaunchKernelGGL(k_decompose_apply<true>, dim3(capped_blocks(n / 4, 256), 4), dim3(256), 0, c.stream, i4, o4, n, lam);
    else hipLaunchKernelGGL(k_decompose_apply<false>, dim3(capped_blocks(n, 256), 4), dim3(256), 0, c.stream, i4, o4, n, lam);
    TSTWO_LAUNCH_CHECK();
    for (int k = 0; k < 4; k++) lambda[k] = l[k];
    return TSTWO_OK;
}

}  // extern "C"

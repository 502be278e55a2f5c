/*
 * draw_edge_search.c -- finds Blake2sChannel states whose next draw_felt lands on an edge of the rejection rule
 * (csrc/blake2s.cuh chan_mix_draw, tstwo_amd/channel.py _draw_base_felts): a word of the draw's first hash equal to 2P, 2^32 - 1,
 * 2P - 1 or P.  Such a hash has probability 2^-28 .. 2^-30, so no seeded test ever meets one; the digests found here are committed
 * in tests/golden/blake2s_draw_edges.json and replayed by tests/test_cpu_draw_edges.py and tests/test_gpu_draw_edges.py.
 * NOT run by the suite except for a short, sanitizer-built self check.  TEST INFRASTRUCTURE ONLY.
 *
 * Build:  cc -O3 -pthread -Ioracle -o draw_edge_search tools/draw_edge_search.c oracle/tstwo_oracle.c
 *
 * A trial g = 0, 1, ... < --bound starts a channel at digest = {TAG, lane, counter lo, counter hi, salt, 0, 0, 0} with
 * lane = g mod lanes and counter = --start + g / lanes, n_sent = --n-sent, and replays a transcript up to the targeted draw:
 *   generic   every --mix HEX payload in order (digest <- H(digest || payload), n_sent <- 0), then --pre-draws true draws
 *   --fri     the commit loop of FriProver.commit over the circle columns of --cols (the oracle's trees and folds) up to alpha
 *             number --draw
 *   --gkr-gp  prove_batch of one grand-product instance over the four input felts HEX, up to the draw of its sum-check round
 * and tests the FIRST hash of that draw against --cond.  The report is the smallest g that meets it, whatever the thread timing,
 * so the same arguments give the same report.  --lane L walks lane L alone (one thread): with --start C --bound 1 it re-examines
 * one recorded trial.
 *
 * Conditions (k = index of the first matching word):
 *   rej_lo_2P  rej_lo_max  rej_lo    a word k < 4 is 0xFFFFFFFE / 0xFFFFFFFF / either; the redraw is accepted
 *   rej_hi_2P  rej_hi_max  rej_hi    a word k >= 4 is ...; words 0..3 are all < 2P; the redraw is accepted
 *   acc_lo_top acc_hi_top            a word k < 4 / k >= 4 is 2P - 1 = 0xFFFFFFFD, no word is >= 2P
 *   acc_P                            a word k < 4 is P = 0x7FFFFFFF, no word is >= 2P
 *   rej                              any word is >= 2P; the redraw is accepted
 */
#include <inttypes.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "tstwo_oracle.h"

typedef uint32_t u32;
typedef uint64_t u64;

#define TAG 0xD4A3ED6Eu
#define TWO_P 0xFFFFFFFEu
#define MAX_MIX 8
#define MAX_COLS 4
#define MAX_LOG 6

static const u32 IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};

typedef struct { u32 d[8]; u32 n_sent; } chan_t;

/* The channel's own compressions, unrolled (RFC 7693; the trees of --fri go through the oracle's).  main() checks it against
 * orc_blake2s_compress before any search. */
#define ROTR(x, r) (((x) >> (r)) | ((x) << (32 - (r))))
#define G(a, b, c, d, x, y)                        \
    do {                                           \
        a = a + b + (x); d = ROTR(d ^ a, 16);      \
        c = c + d;       b = ROTR(b ^ c, 12);      \
        a = a + b + (y); d = ROTR(d ^ a, 8);       \
        c = c + d;       b = ROTR(b ^ c, 7);       \
    } while (0)
#define ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                                      \
    G(v0, v4, v8, v12, m[s0], m[s1]); G(v1, v5, v9, v13, m[s2], m[s3]); G(v2, v6, v10, v14, m[s4], m[s5]);               \
    G(v3, v7, v11, v15, m[s6], m[s7]); G(v0, v5, v10, v15, m[s8], m[s9]); G(v1, v6, v11, v12, m[s10], m[s11]);           \
    G(v2, v7, v8, v13, m[s12], m[s13]); G(v3, v4, v9, v14, m[s14], m[s15]);
static inline void compress(u32 h[8], const u32 m[16], u32 count, int last) {
    u32 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    u32 v8 = IV[0], v9 = IV[1], v10 = IV[2], v11 = IV[3], v12 = IV[4] ^ count, v13 = IV[5], v14 = last ? ~IV[6] : IV[6], v15 = IV[7];
    ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
    ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
    ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
    ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
    ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
    ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
    ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
    ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
    h[0] ^= v0 ^ v8; h[1] ^= v1 ^ v9; h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

/* digest <- Blake2s(digest || payload), payload of n_words words; n_sent <- 0 */
static void chan_mix(chan_t *c, const u32 *payload, size_t n_words) {
    u32 h[8], m[16];
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01010020u;
    size_t total = 8 + n_words, done = 0;               /* words of the whole message */
    do {
        size_t take = total - done < 16 ? total - done : 16;
        for (size_t i = 0; i < 16; i++) {
            size_t w = done + i;
            m[i] = i >= take ? 0 : (w < 8 ? c->d[w] : payload[w - 8]);
        }
        done += take;
        compress(h, m, (u32)(4 * done), done == total);
    } while (done < total);
    memcpy(c->d, h, sizeof h);
    c->n_sent = 0;
}

/* one hash of a draw: H(digest || LE32(n_sent) || 0^28); n_sent += 1 */
static void chan_draw_hash(chan_t *c, u32 w[8]) {
    u32 m[16] = {0};
    for (int i = 0; i < 8; i++) { w[i] = IV[i]; m[i] = c->d[i]; }
    w[0] ^= 0x01010020u;
    m[8] = c->n_sent;
    c->n_sent += 1;
    compress(w, m, 64, 1);
}

/* the unrolled compression against the oracle's, on a two-block message */
static int self_check(void) {
    u32 m[16], a[8], b[8], o[8];
    for (int i = 0; i < 16; i++) m[i] = 0x9E3779B9u * (u32)(i + 1);
    for (int i = 0; i < 8; i++) a[i] = b[i] = IV[i] ^ (i ? 0 : 0x01010020u);
    for (int blk = 0; blk < 2; blk++) {
        compress(a, m, 64u * (u32)(blk + 1), blk);
        orc_blake2s_compress(b, m, 64u * (u32)(blk + 1), 0, blk ? 0xFFFFFFFFu : 0, 0, o);
        memcpy(b, o, sizeof b);
        m[blk] ^= a[7];
    }
    return !memcmp(a, b, sizeof a);
}

static int accepted(const u32 w[8]) {
    for (int k = 0; k < 8; k++) if (w[k] >= TWO_P) return 0;
    return 1;
}

/* draw_felt: hashes until all 8 words are < 2P; the first four, reduced */
static orc_qm31 chan_draw_felt(chan_t *c) {
    u32 w[8];
    do chan_draw_hash(c, w); while (!accepted(w));
    u32 f[4];
    for (int k = 0; k < 4; k++) f[k] = w[k] >= ORC_P ? w[k] - ORC_P : w[k];
    return (orc_qm31){f[0], f[1], f[2], f[3]};
}

/* ---- conditions */
typedef struct { const char *name; int lo, hi; u32 v0, v1; int rejected; } cond_t;
static const cond_t CONDS[] = {
    {"rej_lo_2P", 0, 4, 0xFFFFFFFEu, 0xFFFFFFFEu, 1}, {"rej_lo_max", 0, 4, 0xFFFFFFFFu, 0xFFFFFFFFu, 1},
    {"rej_lo", 0, 4, 0xFFFFFFFEu, 0xFFFFFFFFu, 1},    {"rej_hi_2P", 4, 8, 0xFFFFFFFEu, 0xFFFFFFFEu, 1},
    {"rej_hi_max", 4, 8, 0xFFFFFFFFu, 0xFFFFFFFFu, 1}, {"rej_hi", 4, 8, 0xFFFFFFFEu, 0xFFFFFFFFu, 1},
    {"acc_lo_top", 0, 4, 0xFFFFFFFDu, 0xFFFFFFFDu, 0}, {"acc_hi_top", 4, 8, 0xFFFFFFFDu, 0xFFFFFFFDu, 0},
    {"acc_P", 0, 4, 0x7FFFFFFFu, 0x7FFFFFFFu, 0},     {"rej", 0, 8, 0xFFFFFFFEu, 0xFFFFFFFFu, 1},
};

/* the index of the first word of w that meets the condition, or -1; c = the channel after the hash (for the redraw) */
static int cond_meets(const cond_t *cd, const u32 w[8], const chan_t *c) {
    int k = -1;
    for (int i = cd->lo; i < cd->hi && k < 0; i++) if (w[i] == cd->v0 || w[i] == cd->v1) k = i;
    if (k < 0) return -1;
    if (!cd->rejected) return accepted(w) ? k : -1;
    if (cd->lo == 4) for (int i = 0; i < 4; i++) if (w[i] >= TWO_P) return -1;
    chan_t r = *c;
    u32 w2[8];
    chan_draw_hash(&r, w2);
    return accepted(w2) ? k : -1;
}

/* ---- the job */
typedef struct {
    const cond_t *cond;
    u32 salt, n_sent;
    size_t n_mix;
    u32 *mix[MAX_MIX];
    size_t mix_words[MAX_MIX];
    u32 pre_draws;
    /* fri */
    size_t n_cols;
    u32 col_logs[MAX_COLS];
    u32 *cols[MAX_COLS][4];
    u32 target_draw;
    uint8_t first_root[32];
    /* gkr */
    int gkr;
    orc_qm31 gkr_d[4];
    /* walk */
    u32 lanes;
    int only_lane;
    u64 start, bound;
    _Atomic u64 best;
} job_t;

static void digest_of(const job_t *J, u32 lane, u64 counter, u32 d[8]) {
    d[0] = TAG; d[1] = lane; d[2] = (u32)counter; d[3] = (u32)(counter >> 32); d[4] = J->salt; d[5] = d[6] = d[7] = 0;
}

static void root_words(const uint8_t r[32], u32 w[8]) {
    for (int i = 0; i < 8; i++) w[i] = (u32)r[4 * i] | (u32)r[4 * i + 1] << 8 | (u32)r[4 * i + 2] << 16 | (u32)r[4 * i + 3] << 24;
}

/* the commit loop up to the first hash of alpha number target_draw; returns 0 on an oracle error */
static int fri_to_draw(const job_t *J, chan_t *c, u32 w[8]) {
    u32 buf[2][4][1 << MAX_LOG];
    uint8_t layers[32 * (2 << MAX_LOG)], root[32];
    u32 rw[8];
    const u32 log = J->col_logs[0], tw_log = log + 1;
    const u32 ho = orc_half_odds_initial(tw_log);
    root_words(J->first_root, rw);
    chan_mix(c, rw, 8);
    if (J->target_draw == 0) { chan_draw_hash(c, w); return 1; }
    orc_qm31 alpha = chan_draw_felt(c);
    int cur = 0;
    u32 *dst[4] = {buf[0][0], buf[0][1], buf[0][2], buf[0][3]};
    for (int k = 0; k < 4; k++) memset(dst[k], 0, sizeof(u32) << (log - 1));
    const u32 *src[4] = {J->cols[0][0], J->cols[0][1], J->cols[0][2], J->cols[0][3]};
    if (orc_fold_circle_into_line(dst, (size_t)1 << (log - 1), src, log, (ho << (tw_log - log + 1)) & 0x7FFFFFFFu, alpha)) return 0;
    u32 draw = 1;
    for (u32 lg = log - 1;; lg--) {
        const u32 *in[4] = {buf[cur][0], buf[cur][1], buf[cur][2], buf[cur][3]};
        const u32 logs[4] = {lg, lg, lg, lg};
        if (orc_merkle_commit(in, logs, 4, layers, root)) return 0;
        root_words(root, rw);
        chan_mix(c, rw, 8);
        if (draw == J->target_draw) { chan_draw_hash(c, w); return 1; }
        alpha = chan_draw_felt(c);
        draw++;
        if (lg == 0) return 0;
        u32 *out[4] = {buf[cur ^ 1][0], buf[cur ^ 1][1], buf[cur ^ 1][2], buf[cur ^ 1][3]};
        if (orc_fold_line(in, lg, (ho << (tw_log - lg)) & 0x7FFFFFFFu, alpha, out)) return 0;
        cur ^= 1;
        for (size_t j = 1; j < J->n_cols; j++) {
            if (J->col_logs[j] != lg) continue;           /* a circle column of log lg joins the line layer of log lg - 1 */
            const u32 *s[4] = {J->cols[j][0], J->cols[j][1], J->cols[j][2], J->cols[j][3]};
            if (orc_fold_circle_into_line(out, (size_t)1 << (lg - 1), s, lg, (ho << (tw_log - lg + 1)) & 0x7FFFFFFFu, alpha)) return 0;
        }
    }
}

/* ---- --gkr-gp: prove_batch (gkr_prover.ts:440-580) of ONE grand-product instance of 2^2 inputs d[0..3], up to the first hash of
 * the draw behind its only sum-check round: layer 0 (mix the output, draw alpha and lambda, mix the mask, draw r), the top of
 * layer 1 (mix the claim, draw alpha and lambda), the round polynomial (tests/gkr_round_model.py corrected_poly), its mix. */
typedef orc_qm31 q31;
static void mix_q(chan_t *c, const q31 *f, size_t n) {
    u32 w[16];
    for (size_t i = 0; i < n; i++) { w[4 * i] = f[i].a; w[4 * i + 1] = f[i].b; w[4 * i + 2] = f[i].c; w[4 * i + 3] = f[i].d; }
    chan_mix(c, w, 4 * n);
}
static int q_is_zero(q31 x) { return !(x.a | x.b | x.c | x.d); }
static int gkr_gp_to_draw(const q31 d[4], chan_t *c, u32 w[8]) {
    const q31 zero = {0, 0, 0, 0}, one = {1, 0, 0, 0}, two = {2, 0, 0, 0};
    q31 p[2] = {orc_qm31_mul(d[0], d[1]), orc_qm31_mul(d[2], d[3])};
    q31 out = orc_qm31_mul(p[0], p[1]);
    mix_q(c, &out, 1);
    chan_draw_felt(c);
    chan_draw_felt(c);
    mix_q(c, p, 2);
    q31 r = chan_draw_felt(c);
    q31 claim = orc_qm31_add(orc_qm31_mul(r, orc_qm31_sub(p[1], p[0])), p[0]);
    mix_q(c, &claim, 1);
    chan_draw_felt(c);
    chan_draw_felt(c);
    /* the eq table of the point (r) is the one value 1 - r; f(0), f(2) of the oracle's one variable */
    q31 e = orc_qm31_sub(one, r), a, t;
    q31 f0 = orc_qm31_mul(orc_qm31_mul(d[0], d[1]), e);
    q31 f2 = orc_qm31_mul(orc_qm31_mul(orc_qm31_sub(orc_qm31_add(d[2], d[2]), d[0]), orc_qm31_sub(orc_qm31_add(d[3], d[3]), d[1])), e);
    if (orc_qm31_inverse(e, &a) || orc_qm31_inverse(orc_qm31_sub(one, orc_qm31_add(r, r)), &t)) return 0;
    q31 xs[4] = {zero, one, two, orc_qm31_mul(e, t)}, ys[4], co[4] = {zero, zero, zero, zero};
    ys[0] = orc_qm31_mul(orc_qm31_mul(f0, e), a);
    ys[1] = orc_qm31_sub(claim, ys[0]);
    ys[2] = orc_qm31_mul(orc_qm31_mul(f2, orc_qm31_sub(orc_qm31_mul_m31(r, 3), one)), a);
    ys[3] = zero;
    for (int i = 0; i < 4; i++) {                                   /* interpolate_lagrange */
        q31 term[4] = {ys[i], zero, zero, zero};
        int len = 1;
        for (int j = 0; j < 4; j++) {
            if (j == i) continue;
            if (orc_qm31_inverse(orc_qm31_sub(xs[i], xs[j]), &t)) return 0;
            term[0] = orc_qm31_mul(term[0], t);
        }
        for (int j = 0; j < 4; j++) {                               /* term *= (x - xs[j]) */
            if (j == i) continue;
            for (int k = len; k >= 0; k--)
                term[k] = orc_qm31_sub(k > 0 ? term[k - 1] : zero, k < len ? orc_qm31_mul(term[k], xs[j]) : zero);
            len++;
        }
        for (int k = 0; k < 4; k++) co[k] = orc_qm31_add(co[k], term[k]);
    }
    size_t n = 4;
    while (n && q_is_zero(co[n - 1])) n--;
    mix_q(c, co, n);
    chan_draw_hash(c, w);
    return 1;
}

typedef struct { job_t *J; u32 lane, stride; u64 checksum; int hit_word; u32 hit_value; } worker_t;

static void *worker(void *arg) {
    worker_t *W = (worker_t *)arg;
    job_t *J = W->J;
    u64 g = J->only_lane >= 0 ? 0 : W->lane;
    for (u64 counter = J->start; g < J->bound; counter++, g += W->stride) {
        if (g > atomic_load_explicit(&J->best, memory_order_relaxed)) break;
        chan_t c;
        u32 w[8];
        digest_of(J, W->lane, counter, c.d);
        c.n_sent = J->n_sent;
        if (J->n_cols) {
            if (!fri_to_draw(J, &c, w)) { fprintf(stderr, "oracle error in the commit loop\n"); exit(2); }
        } else if (J->gkr) {
            if (!gkr_gp_to_draw(J->gkr_d, &c, w)) continue;            /* a division by zero on the way: no proof from this state */
        } else {
            for (size_t i = 0; i < J->n_mix; i++) chan_mix(&c, J->mix[i], J->mix_words[i]);
            for (u32 i = 0; i < J->pre_draws; i++) chan_draw_felt(&c);
            chan_draw_hash(&c, w);
        }
        W->checksum += w[0];
        int k = cond_meets(J->cond, w, &c);
        if (k >= 0) {
            u64 old = atomic_load(&J->best);
            while (g < old && !atomic_compare_exchange_weak(&J->best, &old, g)) {}
            W->hit_word = k;
            W->hit_value = w[k];
            break;
        }
    }
    return NULL;
}

static int parse_hex(const char *s, u32 **out, size_t *n_words) {
    size_t n = strlen(s);
    if (n % 8) return 0;
    *n_words = n / 8;
    *out = (u32 *)calloc(*n_words ? *n_words : 1, sizeof(u32));
    for (size_t i = 0; i < n / 2; i++) {
        unsigned b;
        if (sscanf(s + 2 * i, "%2x", &b) != 1) { free(*out); *out = NULL; return 0; }
        (*out)[i / 4] |= (u32)b << (8 * (i % 4));
    }
    return 1;
}

static int usage(void) {
    fprintf(stderr, "usage: draw_edge_search --cond NAME [--salt N] [--n-sent S] [--mix HEX]... [--pre-draws K]\n"
                    "         [--fri LOG[,LOG..] --cols FILE --draw I] [--gkr-gp HEX] [--lanes T] [--lane L] [--start C] --bound B\n");
    return 64;
}

int main(int argc, char **argv) {
    static job_t J;
    J.lanes = 8; J.only_lane = -1; J.bound = 0;
    const char *cols_path = NULL;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i], *v = i + 1 < argc ? argv[i + 1] : NULL;
        if (!v) return usage();
        i++;
        if (!strcmp(a, "--cond")) {
            for (size_t k = 0; k < sizeof CONDS / sizeof *CONDS; k++) if (!strcmp(CONDS[k].name, v)) J.cond = &CONDS[k];
            if (!J.cond) return usage();
        } else if (!strcmp(a, "--salt")) J.salt = (u32)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--n-sent")) J.n_sent = (u32)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--pre-draws")) J.pre_draws = (u32)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--draw")) J.target_draw = (u32)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--lanes")) J.lanes = (u32)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--lane")) J.only_lane = (int)strtoul(v, NULL, 0);
        else if (!strcmp(a, "--start")) J.start = strtoull(v, NULL, 0);
        else if (!strcmp(a, "--bound")) J.bound = strtoull(v, NULL, 0);
        else if (!strcmp(a, "--cols")) cols_path = v;
        else if (!strcmp(a, "--mix")) {
            if (J.n_mix == MAX_MIX || !parse_hex(v, &J.mix[J.n_mix], &J.mix_words[J.n_mix])) return usage();
            J.n_mix++;
        } else if (!strcmp(a, "--gkr-gp")) {
            u32 *d = NULL;
            size_t n;
            if (!parse_hex(v, &d, &n) || n != 16) { free(d); return usage(); }
            for (int k = 0; k < 4; k++) J.gkr_d[k] = (orc_qm31){d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]};
            free(d);
            J.gkr = 1;
        } else if (!strcmp(a, "--fri")) {
            for (const char *p = v; *p && J.n_cols < MAX_COLS;) {
                char *end;
                J.col_logs[J.n_cols++] = (u32)strtoul(p, &end, 10);
                p = *end == ',' ? end + 1 : end;
            }
        } else return usage();
    }
    if (!J.cond || !J.bound || J.lanes < 1 || J.lanes > 64) return usage();
    if (!self_check()) { fprintf(stderr, "the unrolled compression disagrees with the oracle's\n"); return 2; }
    if (J.n_cols) {                                        /* --cols: per column its four coordinate columns, little-endian words */
        FILE *f = cols_path ? fopen(cols_path, "rb") : NULL;
        if (!f) return usage();
        const u32 *flat[4 * MAX_COLS];
        u32 logs[4 * MAX_COLS];
        for (size_t j = 0; j < J.n_cols; j++) {
            u32 lg = J.col_logs[j];
            if (lg < 3 || lg > MAX_LOG || (j && lg >= J.col_logs[j - 1])) { fclose(f); return usage(); }
            for (int k = 0; k < 4; k++) {
                J.cols[j][k] = (u32 *)malloc(sizeof(u32) << lg);
                if (fread(J.cols[j][k], sizeof(u32), (size_t)1 << lg, f) != (size_t)1 << lg) { fclose(f); return usage(); }
                flat[4 * j + k] = J.cols[j][k];
                logs[4 * j + k] = lg;
            }
        }
        fclose(f);
        uint8_t *layers = (uint8_t *)malloc(32 * ((size_t)2 << J.col_logs[0]));
        int rc = orc_merkle_commit(flat, logs, 4 * J.n_cols, layers, J.first_root);
        free(layers);
        if (rc) return 2;
    }
    atomic_store(&J.best, UINT64_MAX);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    u32 n_threads = J.only_lane >= 0 ? 1 : J.lanes;
    pthread_t th[64];
    worker_t W[64];
    for (u32 t = 0; t < n_threads; t++) {
        W[t] = (worker_t){&J, J.only_lane >= 0 ? (u32)J.only_lane : t, n_threads, 0, -1, 0};
        if (pthread_create(&th[t], NULL, worker, &W[t])) return 2;
    }
    for (u32 t = 0; t < n_threads; t++) pthread_join(th[t], NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    u64 best = atomic_load(&J.best), checksum = 0;
    for (u32 t = 0; t < n_threads; t++) checksum += W[t].checksum;
    if (best == UINT64_MAX) {
        printf("{\"found\": false, \"cond\": \"%s\", \"trials\": %" PRIu64 ", \"checksum\": %" PRIu64 "}\n", J.cond->name, J.bound, checksum);
    } else {
        u32 t = (u32)(best % n_threads), d[8];
        u64 counter = J.start + best / n_threads;
        digest_of(&J, W[t].lane, counter, d);
        printf("{\"found\": true, \"cond\": \"%s\", \"digest\": [", J.cond->name);
        for (int k = 0; k < 8; k++) printf("%s%" PRIu32, k ? ", " : "", d[k]);
        printf("], \"lane\": %" PRIu32 ", \"counter\": %" PRIu64 ", \"trials\": %" PRIu64 ", \"word\": %d, \"value\": \"0x%08" PRIX32 "\"}\n",
               W[t].lane, counter, best + 1, W[t].hit_word, W[t].hit_value);
    }
    fprintf(stderr, "seconds %.2f\n", (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec));
    for (size_t i = 0; i < J.n_mix; i++) free(J.mix[i]);
    for (size_t j = 0; j < J.n_cols; j++) for (int k = 0; k < 4; k++) free(J.cols[j][k]);
    return 0;
}

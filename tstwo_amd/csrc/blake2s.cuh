// blake2s.cuh — BLAKE2s-256 on the device (RFC 7693, unkeyed, 32-byte digest — what @noble/hashes blake2s computes for the
// reference, vcs/blake2_hash.ts:53) for the Merkle kernels, the FRI commit tail and the grind (merkle.hip): the compression by
// one lane (b2s_compress), by a quad of lanes with the message in registers or in LDS (b2s_quad_block64[_lds]), and the
// Blake2sChannel steps built on the quad form (chan_mix_draw).  Device-only; nothing here touches memory except through the
// pointers it is handed.
#pragma once
#include "m31.cuh"

namespace tstwo {
namespace b2s {

constexpr u32 IV0 = 0x6A09E667u, IV1 = 0xBB67AE85u, IV2 = 0x3C6EF372u, IV3 = 0xA54FF53Au, IV4 = 0x510E527Fu,
              IV5 = 0x9B05688Cu, IV6 = 0x1F83D9ABu, IV7 = 0x5BE0CD19u;

// The message schedule SIGMA (vcs/blake2s_ref.ts:9-20), one row per round: R(round, s0 .. s15).  Expanded by the three forms of
// the compression below so that every message index is a literal.
#define B2S_SIGMA(R)                                               \
    R(0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)     \
    R(1, 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)     \
    R(2, 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)     \
    R(3, 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)     \
    R(4, 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)     \
    R(5, 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)     \
    R(6, 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)     \
    R(7, 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)     \
    R(8, 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)     \
    R(9, 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)

__device__ __forceinline__ u32 rotr32(u32 x, int r) { return __builtin_amdgcn_alignbit(x, x, r); }

#define B2S_G(a, b, c, d, x, y)                     \
    do {                                            \
        a = a + b + (x); d = rotr32(d ^ a, 16);     \
        c = c + d;       b = rotr32(b ^ c, 12);     \
        a = a + b + (y); d = rotr32(d ^ a, 8);      \
        c = c + d;       b = rotr32(b ^ c, 7);      \
    } while (0)

// Four independent G functions (a column step or a diagonal step of a round) issued opcode by opcode in priority phases
// (phase.cuh: heavy = v_add3 / v_alignbit on port 0 at high priority, light = v_xor / v_add on either port): per step
// 24 heavy + 24 light instructions.  Entered and left at kPrioHeavy.
#define B2S_STEP4(a0, b0, c0, d0, a1, b1, c1, d1, a2, b2, c2, d2, a3, b3, c3, d3, x0, y0, x1, y1, x2, y2, x3, y3) \
    do {                                                                                                          \
        a0 = a0 + b0 + (x0); a1 = a1 + b1 + (x1); a2 = a2 + b2 + (x2); a3 = a3 + b3 + (x3);                       \
        phase<kPrioLight>(a0, a1, a2, a3);                                                                        \
        d0 ^= a0; d1 ^= a1; d2 ^= a2; d3 ^= a3;                                                                   \
        phase<kPrioHeavy>(d0, d1, d2, d3);                                                                        \
        d0 = rotr32(d0, 16); d1 = rotr32(d1, 16); d2 = rotr32(d2, 16); d3 = rotr32(d3, 16);                       \
        phase<kPrioLight>(d0, d1, d2, d3);                                                                        \
        c0 += d0; c1 += d1; c2 += d2; c3 += d3;                                                                   \
        b0 ^= c0; b1 ^= c1; b2 ^= c2; b3 ^= c3;                                                                   \
        phase<kPrioHeavy>(b0, b1, b2, b3);                                                                        \
        b0 = rotr32(b0, 12); b1 = rotr32(b1, 12); b2 = rotr32(b2, 12); b3 = rotr32(b3, 12);                       \
        a0 = a0 + b0 + (y0); a1 = a1 + b1 + (y1); a2 = a2 + b2 + (y2); a3 = a3 + b3 + (y3);                       \
        phase<kPrioLight>(a0, a1, a2, a3);                                                                        \
        d0 ^= a0; d1 ^= a1; d2 ^= a2; d3 ^= a3;                                                                   \
        phase<kPrioHeavy>(d0, d1, d2, d3);                                                                        \
        d0 = rotr32(d0, 8); d1 = rotr32(d1, 8); d2 = rotr32(d2, 8); d3 = rotr32(d3, 8);                           \
        phase<kPrioLight>(d0, d1, d2, d3);                                                                        \
        c0 += d0; c1 += d1; c2 += d2; c3 += d3;                                                                   \
        b0 ^= c0; b1 ^= c1; b2 ^= c2; b3 ^= c3;                                                                   \
        phase<kPrioHeavy>(b0, b1, b2, b3);                                                                        \
        b0 = rotr32(b0, 7); b1 = rotr32(b1, 7); b2 = rotr32(b2, 7); b3 = rotr32(b3, 7);                           \
    } while (0)

// One compression (vcs/blake2s_ref.ts:176-230): h <- F(h, m, t, last)
__device__ __forceinline__ void b2s_compress(u32 h[8], const u32 m[16], u32 t_lo, bool last) {
    u32 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    u32 v8 = IV0, v9 = IV1, v10 = IV2, v11 = IV3, v12 = IV4 ^ t_lo, v13 = IV5, v14 = last ? ~IV6 : IV6, v15 = IV7;
    phase<kPrioHeavy>(v0, v1, v2, v3);
#define B2S_ROUND(r, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                                 \
    B2S_STEP4(v0, v4, v8, v12, v1, v5, v9, v13, v2, v6, v10, v14, v3, v7, v11, v15,                                         \
              m[s0], m[s1], m[s2], m[s3], m[s4], m[s5], m[s6], m[s7]);                                                      \
    B2S_STEP4(v0, v5, v10, v15, v1, v6, v11, v12, v2, v7, v8, v13, v3, v4, v9, v14,                                         \
              m[s8], m[s9], m[s10], m[s11], m[s12], m[s13], m[s14], m[s15]);
    B2S_SIGMA(B2S_ROUND)
#undef B2S_ROUND
    phase<kPrioLight>(v4, v5, v6, v7);
    h[0] ^= v0 ^ v8;  h[1] ^= v1 ^ v9;  h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

// A digest in registers; a node without columns = Blake2s(left || right), one 64-byte final block.
struct Digest { u32 w[8]; };
__device__ __forceinline__ Digest hash_pair(const Digest &l, const Digest &r) {
    Digest d = {{IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7}};
    const u32 m[16] = {l.w[0], l.w[1], l.w[2], l.w[3], l.w[4], l.w[5], l.w[6], l.w[7], r.w[0], r.w[1], r.w[2], r.w[3], r.w[4], r.w[5], r.w[6], r.w[7]};
    b2s_compress(d.w, m, 64u, true);
    return d;
}

// ---- Upper tree, latency path: one compression spread over a QUAD of lanes (lane j of the quad owns column j of the
// 4x4 Blake2s state).  The column step is lane-local; the diagonal step rotates rows b, c, d by 1, 2, 3 lanes with DPP
// quad_perm moves and rotates them back.  A lane needs message words m[SIGMA[r][2j..]], i.e. a lane-dependent choice
// among registers that are literal per round: three v_cndmask on the constant lane masks j==1, j==2, j==3.
// ~1/2.4 of the dependent-instruction chain of the one-lane compression, which is what bounds the top of a tree.
__device__ __forceinline__ u32 quad_rot(u32 x, int by) {   // value held by lane (j + by) & 3 of this lane's quad
    return by == 1 ? (u32)__builtin_amdgcn_mov_dpp((int)x, 0x39, 0xF, 0xF, false)
         : by == 2 ? (u32)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, false)
                   : (u32)__builtin_amdgcn_mov_dpp((int)x, 0x93, 0xF, 0xF, false);
}
__device__ __forceinline__ u32 sel4(u32 x0, u32 x1, u32 x2, u32 x3, u32 j) {
    u32 r = x0;
    r = j == 1 ? x1 : r;
    r = j == 2 ? x2 : r;
    r = j == 3 ? x3 : r;
    return r;
}
// Single 64-byte final block from the initial state (a node of children only: hashNode, vcs/blake2_merkle.ts:9-24).
// Returns the digest words j (o_lo) and 4+j (o_hi) in lane j of the quad.
__device__ __forceinline__ void b2s_quad_block64(const u32 (&m)[16], u32 j, u32 &o_lo, u32 &o_hi) {
    const u32 ivlo = sel4(IV0, IV1, IV2, IV3, j), ivhi = sel4(IV4, IV5, IV6, IV7, j);
    const u32 h_lo = ivlo ^ (j == 0 ? 0x01010020u : 0u), h_hi = ivhi;
    u32 a = h_lo, b = h_hi, c = ivlo, d = ivhi ^ sel4(64u, 0u, 0xFFFFFFFFu, 0u, j);
#define B2SQ_ROUND(r, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)       \
    {                                                                                            \
        u32 x = sel4(m[s0], m[s2], m[s4], m[s6], j), y = sel4(m[s1], m[s3], m[s5], m[s7], j);     \
        B2S_G(a, b, c, d, x, y);                                                                  \
        b = quad_rot(b, 1); c = quad_rot(c, 2); d = quad_rot(d, 3);                               \
        x = sel4(m[s8], m[s10], m[s12], m[s14], j); y = sel4(m[s9], m[s11], m[s13], m[s15], j);   \
        B2S_G(a, b, c, d, x, y);                                                                  \
        b = quad_rot(b, 3); c = quad_rot(c, 2); d = quad_rot(d, 1);                               \
    }
    B2S_SIGMA(B2SQ_ROUND)
#undef B2SQ_ROUND
    o_lo = h_lo ^ a ^ c;
    o_hi = h_hi ^ b ^ d;
}

// The same with the message in LDS instead of registers: lane j of the quad reads its words of round r — m[SIGMA[r][2j]],
// m[SIGMA[r][2j+1]] for the column step, m[SIGMA[r][8+2j]], m[SIGMA[r][8+2j+1]] for the diagonal step — from 40 LDS byte addresses
// it computed ONCE (quad_msg_addrs: the quad's message slot does not move between tree levels).  40 ds_read_b32 per compression
// instead of 120 v_cndmask (the three selects per word above): a third fewer issue slots on a path where one wave issues alone.
typedef __attribute__((address_space(3))) const u32 lds_cu32;
struct QuadMsgAddrs { u32 a[40]; };
__device__ __forceinline__ void quad_msg_addrs(QuadMsgAddrs &qa, u32 msg_byte_base, u32 j) {
#define B2SQ_ADDR(r, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                   \
    qa.a[4 * r + 0] = msg_byte_base + sel4(4u * s0, 4u * s2, 4u * s4, 4u * s6, j);                             \
    qa.a[4 * r + 1] = msg_byte_base + sel4(4u * s1, 4u * s3, 4u * s5, 4u * s7, j);                             \
    qa.a[4 * r + 2] = msg_byte_base + sel4(4u * s8, 4u * s10, 4u * s12, 4u * s14, j);                          \
    qa.a[4 * r + 3] = msg_byte_base + sel4(4u * s9, 4u * s11, 4u * s13, 4u * s15, j);
    B2S_SIGMA(B2SQ_ADDR)
#undef B2SQ_ADDR
}
__device__ __forceinline__ u32 lds_word(u32 byte_addr) { return *(lds_cu32 *)(uintptr_t)byte_addr; }
__device__ __forceinline__ void b2s_quad_block64_lds(const QuadMsgAddrs &qa, u32 j, u32 &o_lo, u32 &o_hi) {
    const u32 ivlo = sel4(IV0, IV1, IV2, IV3, j), ivhi = sel4(IV4, IV5, IV6, IV7, j);
    const u32 h_lo = ivlo ^ (j == 0 ? 0x01010020u : 0u), h_hi = ivhi;
    u32 a = h_lo, b = h_hi, c = ivlo, d = ivhi ^ sel4(64u, 0u, 0xFFFFFFFFu, 0u, j);
    u32 w[40];
#pragma unroll
    for (int k = 0; k < 40; k++) w[k] = lds_word(qa.a[k]);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        B2S_G(a, b, c, d, w[4 * r], w[4 * r + 1]);
        b = quad_rot(b, 1); c = quad_rot(c, 2); d = quad_rot(d, 3);
        B2S_G(a, b, c, d, w[4 * r + 2], w[4 * r + 3]);
        b = quad_rot(b, 3); c = quad_rot(c, 2); d = quad_rot(d, 1);
    }
    o_lo = h_lo ^ a ^ c;
    o_hi = h_hi ^ b ^ d;
}

// ---- Blake2sChannel on the device (channel/blake2.ts:25-224, Rust semantics).  State = 10 words: digest[8], n_challenges,
// n_sent.  One quad of lanes runs the (latency-bound) compressions; used by the FRI commit loop so that a layer's root
// never has to travel to the host before the next fold can be launched.
__device__ __forceinline__ void chan_hash64(const u32 (&m)[16], u32 j, u32 (&digest)[8]) {
    u32 lo, hi;
    b2s_quad_block64(m, j, lo, hi);
    // every lane of the quad needs the whole digest: word k lives in lane k & 3 (lo for k < 4, hi for k >= 4)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        digest[k] = (u32)__builtin_amdgcn_readlane((int)lo, k);
        digest[4 + k] = (u32)__builtin_amdgcn_readlane((int)hi, k);
    }
}
// mix_root (vcs/blake2_merkle.ts:28-31): digest <- H(digest || root), n_challenges += 1, n_sent <- 0; then (optionally)
// draw_felt (blake2.ts:158-184): H(digest || LE32(n_sent) || 0^28) until all 8 words < 2P; felt = first 4 words reduced.
// state in registers of every lane of a wave (d, n_chal, n_sent); root: 8 words (global or LDS); felt: the drawn QM31 (valid in
// every lane).  Executed by one whole wave (chan_hash64 broadcasts through readlane of lanes 0..3).
__device__ __forceinline__ void chan_mix_draw(u32 (&d)[8], u32 &n_chal, u32 &n_sent, const u32 *root, bool do_mix, bool do_draw, u32 (&felt)[4]) {
    const u32 j = threadIdx.x & 3;
    if (do_mix) {
        u32 m[16];
#pragma unroll
        for (int k = 0; k < 8; k++) { m[k] = d[k]; m[8 + k] = root[k]; }
        chan_hash64(m, j, d);
        n_chal += 1;
        n_sent = 0;
    }
    if (do_draw) {
        u32 w[8];
        bool ok = false;
        // retry probability per round ~ 2^-28; the loop is bounded so that the kernel always terminates (64 rejections in a
        // row have probability 2^-1792)
        for (int tries = 0; tries < 64 && !ok; tries++) {
            u32 m[16];
#pragma unroll
            for (int k = 0; k < 8; k++) { m[k] = d[k]; m[8 + k] = 0; }
            m[8] = n_sent;
            n_sent += 1;
            chan_hash64(m, j, w);
            ok = true;
#pragma unroll
            for (int k = 0; k < 8; k++) ok = ok && (w[k] < 2u * M31_P);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) felt[k] = w[k] >= M31_P ? w[k] - M31_P : w[k];       // M31.reduce of a value < 2P
    }
}
// mix_felts (channel/blake2.ts:113-118) of the first n_felts QM31s of w (N = 8: at most 2 felts, 16: at most 4): Blake2s over
// digest || 16 n_felts bytes, by every lane on its own (one or two compressions).  The words of w beyond the felts are zero, which
// is the padding of the last block.
template <int N>
__device__ __forceinline__ void chan_mix_felts(u32 (&d)[8], u32 &n_chal, u32 &n_sent, const u32 (&w)[N], u32 n_felts) {
    static_assert(N == 8 || N == 16, "2 or 4 felts");
    u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
    u32 m[16];
#pragma unroll
    for (int k = 0; k < 8; k++) { m[k] = d[k]; m[8 + k] = w[k]; }
    const u32 len = 32u + 16u * n_felts;
    if (N == 8 || n_felts <= 2) {
        b2s_compress(h, m, len, true);
    } else {
        b2s_compress(h, m, 64u, false);
#pragma unroll
        for (int k = 0; k < 8; k++) { m[k] = w[N - 8 + k]; m[8 + k] = 0u; }
        b2s_compress(h, m, len, true);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = h[k];
    n_chal += 1;
    n_sent = 0;
}

}  // namespace b2s
}  // namespace tstwo

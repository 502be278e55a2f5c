// The body of k_gkr_round_finish and k_gkr_round_finish_dev (gkr.hip), over `FinishArgs f`: pasted into both kernels, so that
// the first keeps, instruction for instruction, the code it had before the second existed.
    using namespace b2s;
    const u32 lane = threadIdx.x;
    const bool in = lane < f.n, act = in && ((f.mask >> lane) & 1u);
    const qm31 zero = {0u, 0u, 0u, 0u}, one = {1u, 0u, 0u, 0u};
    constexpr u32 kHalf = 1u << 30;                                   // 1/2 in M31
    // requested first: the channel words are needed last
    u32 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = gload1(f.chan, k);
    u32 n_chal = gload1(f.chan, 8), n_sent = gload1(f.chan, 9);
    qm31 claim = zero, corr = zero, f0 = zero, f2 = zero;
    if (in) { claim = q_of(gload4(f.state, 8 * lane)); corr = q_of(gload4(f.state, 8 * lane + 4)); }
    if (act) { f0 = q_of(gload4(f.sums, 8 * lane)); f2 = q_of(gload4(f.sums, 8 * lane + 4)); }

    // wave-uniform: D = 1 - 2y, 1/y and 1/D from one inversion, b, A = a D
    const qm31 y = f.y, one_y = qm31_sub(one, y), D = qm31_sub(one_y, y);
    const qm31 inv_yd = qm31_inv(qm31_mul(y, D));
    const qm31 inv_y = qm31_mul(inv_yd, D), inv_d = qm31_mul(inv_yd, y);
    const qm31 b = qm31_mul(one_y, inv_d), A = qm31_mul(f.a, D);

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
    qm31 pw = one, sq = f.alpha;
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

    // mix_felts(rp.coeffs[:n_coeffs]) (channel/blake2.ts:113-118): Blake2s over digest || 16 n_coeffs bytes.  The words of the
    // trimmed coefficients are zero, which is the padding of the last block.
    {
        u32 h[8] = {IV0 ^ 0x01010020u, IV1, IV2, IV3, IV4, IV5, IV6, IV7};
        u32 m[16];
#pragma unroll
        for (int k = 0; k < 8; k++) { m[k] = d[k]; m[8 + k] = rp[k]; }
        const u32 len = 32u + 16u * n_coeffs;
        if (n_coeffs <= 2) {
            b2s_compress(h, m, len, true);
        } else {
            b2s_compress(h, m, 64u, false);
#pragma unroll
            for (int k = 0; k < 8; k++) { m[k] = rp[8 + k]; m[8 + k] = 0u; }
            b2s_compress(h, m, len, true);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = h[k];
        n_chal += 1;
        n_sent = 0;
    }
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

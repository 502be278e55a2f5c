// The body of k_sum<KIND, FOLD> and k_sum_ldev<KIND, FOLD> (gkr.hip), over `SumArgs a`: pasted into both kernels, so that the
// first keeps, instruction for instruction, the code it had before the second existed.
    __shared__ u32 lds[8 * (kThreads / 64) + 1];       // wave partials; [last] = "this block is the last arriver"
    u32 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const u32 nt = a.n_terms, stride = gridDim.x * kThreads;
    if (FOLD && a.r_dev) a.r = ld_uniform_q(a.r_dev);
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

// grind_plan.h — which nonces each launch of a proof-of-work search tests (host only: no HIP, no context).
// tests/grind_plan.py restates this in Python; tests/test_cpu_grind.py compiles this header and compares.
#pragma once
#include <cstdint>

namespace tstwo {

enum GrindKind { GRIND_BLAKE2S = 0, GRIND_P252 = 1 };

// Nonce 2^64 - 1 is the "none found" value of the kernels' atomicMin cell: it is never tested and never returned.
constexpr uint64_t kGrindNone = ~(uint64_t)0;
// Lanes per workgroup of k_grind and k_p252_grind: a launch has ceil(batch / kGrindLanes) workgroups, and the lanes of the last
// one at or past `batch` return without a hash.
constexpr uint32_t kGrindLanes = 256;

// Blake2s (63 G hashes/s): batches grow with the expected work so easy targets return after one small launch.
constexpr uint64_t kGrindBlake2sSmall = (uint64_t)1 << 20;       // while fewer than kGrindBlake2sSmallSpan nonces are done
constexpr uint64_t kGrindBlake2sSmallSpan = (uint64_t)1 << 22;
constexpr uint64_t kGrindBlake2sLarge = (uint64_t)1 << 26;
// Poseidon252: a nonce costs ~2 permutations (~1.5e5 lane instructions): batches start small, so that easy targets return after one
// short launch, and grow 4x up to 2^22 nonces (~10 ms).
constexpr uint64_t kGrindP252First = (uint64_t)1 << 16;
constexpr uint32_t kGrindP252GrowLog = 2;
constexpr uint64_t kGrindP252Max = (uint64_t)1 << 22;

// The size of the next batch of a search.  done: nonces tested since start_nonce (the next batch starts at start_nonce + done);
// prev: the size of the batch before it, 0 for the first; left: kGrindNone minus the next batch's first nonce.  0: the nonce space is
// exhausted.  A batch never holds kGrindNone: it ends at 2^64 - 2 at the latest, so it is a multiple of kGrindLanes everywhere but
// there.
inline uint64_t grind_batch(GrindKind kind, uint64_t done, uint64_t prev, uint64_t left) {
    uint64_t batch;
    if (kind == GRIND_BLAKE2S)
        batch = done >= kGrindBlake2sSmallSpan ? kGrindBlake2sLarge : kGrindBlake2sSmall;
    else
        batch = prev == 0 ? kGrindP252First : prev < kGrindP252Max ? prev << kGrindP252GrowLog : prev;
    return left < batch ? left : batch;
}

// A search from `start`: grind_next moves to the next batch, nonces [base, base + batch), behind the one before it, and says whether
// there is one.  The entries launch one kernel per batch and stop at the first batch with a hit.
struct GrindSearch {
    GrindKind kind;
    uint64_t start, base, batch;
};
inline GrindSearch grind_begin(GrindKind kind, uint64_t start) { return {kind, start, start, 0}; }
inline bool grind_next(GrindSearch &s) {
    s.base += s.batch;
    s.batch = grind_batch(s.kind, s.base - s.start, s.batch, kGrindNone - s.base);
    return s.batch != 0;
}

}  // namespace tstwo

// cfft_plan.h — which launches a Circle FFT entry takes for an input (host only: no HIP, no context).
// tests/cfft_plan.py restates this in Python; tests/test_cpu_cfft_plan.py compiles this header and compares.
//
// The n layers of a transform are cut into passes over HBM.  A pass owns the layers [lo, lo + k) and a workgroup owns a tile of
// 2^logt words: the bottom pass (lo = 0, k = logt) a contiguous one, a strided pass 2^k rows of 2^(logt - k) words.  cfft.hip
// launches what cfft_plan() returns and decides nothing itself but the grid (plan_grid asks the runtime for occupancy).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tstwo {

enum CfftEntry : uint8_t { CFFT_EVALUATE, CFFT_INTERPOLATE, CFFT_INTERPOLATE_TO, CFFT_EVALUATE_EXTENDED };
enum CfftRoute : uint8_t {
    CFFT_SMALL,         // n <= 2: k_cfft_small, one lane per column
    CFFT_GENERIC,       // 3 <= n <= 12: k_cfft_pass, the whole column in one tile
    CFFT_TILED,         // n >= 13: the kernels of cfft_fast.cuh
    CFFT_FALLBACK       // interpolate_to / evaluate_extended only: copy / extend into the output, then transform it in place (planned again, as that entry)
};
enum CfftKind : uint8_t {
    CFFT_WHOLE,             // the one launch of the small and generic routes
    CFFT_BOTTOM,            // k_cfft_b<INV, LOGT>
    CFFT_BOTTOM_STREAM,     // k_cfft_b_stream<LOGT>: forward, tile accesses with the non-temporal policy
    CFFT_BOTTOM_OOP,        // k_cfft_b<true, LOGT, true>: reads a second table (the first pass of interpolate_to)
    CFFT_STRIDED,           // k_cfft_a<INV, K, 0, LOGT>
    CFFT_STRIDED_STREAM,    // k_cfft_a_stream<K> (LOGT = 15)
    CFFT_STRIDED_EXT        // k_cfft_a<false, K, EXT, LOGT>: reads the smaller polynomial (the first pass of evaluate_extended)
};

// Every (kind, K, LOGT) that has a kernel: the planner refuses a plan that names another one, cfft.hip instantiates and dispatches
// exactly these.  knob_only: no input reaches it but through TSTWO_CFFT_KB / KA / LOGTA of the experiments build.
struct CfftShape { CfftKind kind; uint8_t logt, k_lo, k_hi; bool knob_only; };
constexpr CfftShape kCfftShapes[] = {
    {CFFT_BOTTOM, 11, 11, 11, true},        {CFFT_BOTTOM, 12, 12, 12, false},       {CFFT_BOTTOM, 13, 13, 13, false},
    {CFFT_BOTTOM, 14, 14, 14, false},       {CFFT_BOTTOM_STREAM, 13, 13, 13, false}, {CFFT_BOTTOM_STREAM, 14, 14, 14, false},
    {CFFT_BOTTOM_OOP, 13, 13, 13, false},   {CFFT_BOTTOM_OOP, 14, 14, 14, false},
    {CFFT_STRIDED, 12, 2, 8, false},        // small strided tiles (few columns): 256 lanes, rows of 2^(12-K) >= 16 words
    {CFFT_STRIDED, 13, 9, 9, false},
    {CFFT_STRIDED, 14, 1, 1, true},         {CFFT_STRIDED, 14, 2, 9, false},        {CFFT_STRIDED, 14, 10, 10, true},
    {CFFT_STRIDED, 15, 8, 10, false},       // the 128 KiB tile (two virtual lanes per lane): 10 layers on 128-byte rows, 9 on 256-byte rows
    {CFFT_STRIDED_STREAM, 15, 8, 10, false},
    {CFFT_STRIDED_EXT, 14, 2, 9, false},    {CFFT_STRIDED_EXT, 15, 8, 10, false},
};
constexpr size_t kCfftShapeRows = sizeof(kCfftShapes) / sizeof(kCfftShapes[0]);
constexpr bool cfft_shape_supported(CfftKind kind, uint32_t k, uint32_t logt) {
    for (size_t r = 0; r < kCfftShapeRows; r++)
        if (kCfftShapes[r].kind == kind && kCfftShapes[r].logt == logt && kCfftShapes[r].k_lo <= k && k <= kCfftShapes[r].k_hi) return true;
    return false;
}

constexpr uint32_t kCfftMaxLog = 30;         // MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4): a 4 GiB column; word offsets stay below 2^30
constexpr uint32_t kCfftMaxPasses = 8;
constexpr uint32_t kCfftTiledLog = 13;       // the tiled route from here on; also the default bottom tile: 2^13 words = 32 KiB + pad, 512 lanes
constexpr uint32_t kCfftGenericThreads = 256, kCfftSmallThreads = 64;

struct CfftKnobs { uint32_t kb, ka_max, logta; };       // experiments build: bottom tile, strided-pass layer limit, strided tile (0 = none)
struct CfftPass {
    CfftKind kind;
    bool scale;                 // the last inverse pass multiplies by 2^-n
    uint32_t lo, k, logt;       // layers [lo, lo + k) on tiles of 2^logt words
    uint32_t threads, lds_bytes, tiles;
};
struct CfftPlan {
    CfftRoute route;
    uint32_t n_passes;          // 0 for CFFT_FALLBACK
    uint32_t cols_per_wg;       // CFFT_GENERIC
    uint32_t blocks;            // CFFT_SMALL, CFFT_GENERIC: the grid (a tiled pass gets its grid from plan_grid)
    CfftPass pass[kCfftMaxPasses];      // in execution order: high -> low layers forward, low -> high inverse
};

// Whether the tile accesses of a forward pass carry the non-temporal policy (cfft_fast.cuh: k_cfft_b_stream / k_cfft_a_stream): a
// column set of 1 GiB and more — several times the 256 MiB cache, where the in-place read-modify-write gains with it
// (tools/microbench7.hip) and 256 x 2^22 is 2 % faster; 32 x 2^22 (512 MiB) measures the same either way, 128 MiB and less lose.
constexpr bool cfft_streams_past_cache(uint64_t n_cols, uint32_t n) { return (n_cols << n) >= ((uint64_t)1 << 28); }

// The default cut of a many-column transform (every entry starts from it):
//   n <= 13, n = 14      ONE pass on the contiguous tile (2^14 words at n = 14: 256 columns 16.4 against 21.2 us for 13 + 1);
//   15 <= n <= 20        13 bottom layers + one strided pass on 2^14-word tiles (n = 19, 20 on the 2^15 tile measured equal or 1 % slower);
//   n = 21               13 + 8 on the 2^15-word tile (512-byte rows) from two workgroups per CU on: 512 x 2^21 3.60 against 3.64 ms,
//                        interpolate 3.78 against 3.85 (128 columns: 0.930 / 0.976 against 0.938 / 0.989);
//   n = 22, 23           13 + 9 / 13 + 10 with the strided pass on the 2^15-word tile (two virtual lanes per lane, 256- / 128-byte
//                        rows) when the launch still has two workgroups per CU — round 4, same box, 256 x 2^22: 3.775 against
//                        3.805 ms forward, 3.985 against 4.027 inverse; 128 x 2^23: 3.815 against 3.895 (14 + 9 on 2^14-word tiles,
//                        round 3's two-pass plan, which stays for few columns) and 4.02 against 4.08;
//   n = 24               14 + 10, the strided pass on the 2^15-word tile: TWO passes instead of 13 + 6 + 5 (round 4: 32 x 2^24
//                        2.09 against 2.66 ms, 64 columns 4.08 against 5.29);
//   n >= 25              13 bottom layers + two strided passes (a 2^14-word bottom tile changes nothing there).
// 12 + 10 at n = 22 (a layer moved from the issue-bound bottom pass to the HBM-bound strided one) measured 3.86 against 3.78.
inline CfftKnobs cfft_default_shape(uint32_t n, uint64_t n_cols, uint32_t n_cus) {
    const bool wide = n >= 15 && (((uint64_t)1 << (n - 15)) * n_cols) >= (uint64_t)2 * n_cus;      // the 2^15 tile halves the workgroup count
    if (n == 24) return {14, 10, 15};
    if (n == 23) return wide ? CfftKnobs{13, 10, 15} : CfftKnobs{14, 9, 14};
    if ((n == 22 || n == 21) && wide) return {13, 9, 15};
    if (n == 14) return {14, 9, 14};
    return {kCfftTiledLog, 9, 14};      // at most 9 layers per strided pass on the 2^14 tile: rows of >= 32 words = 128 B
}

// Fills `plan` for `entry` on n_cols columns of 2^n words (ext: log_size - log_poly of evaluate_extended) on a device of n_cus
// compute units, or returns why there is none (a TSTWO_ERR_BAD_ARG).  Nothing is launched before the whole plan stands.
inline const char *cfft_plan(CfftEntry entry, uint32_t ext, uint32_t n, uint64_t n_cols, uint32_t n_cus, const CfftKnobs &kn, CfftPlan &plan) {
    plan = CfftPlan{};
    if (n == 0 || n > 31) return "cfft: log_size out of range";
    if (n > kCfftMaxLog) return "cfft: log_size > 30 exceeds MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4)";
    const bool inverse = entry == CFFT_INTERPOLATE || entry == CFFT_INTERPOLATE_TO;
    const bool in_place = entry == CFFT_EVALUATE || entry == CFFT_INTERPOLATE;
    plan.route = CFFT_FALLBACK;
    if (!in_place && (n < kCfftTiledLog || kn.kb || kn.ka_max)) return nullptr;      // only the tiled kernels read a second table

    if (n < kCfftTiledLog) {        // one launch
        CfftPass &ps = plan.pass[0];
        ps = {CFFT_WHOLE, inverse, 0, n, n, kCfftSmallThreads, 0, 1};
        uint64_t blocks = (n_cols + kCfftSmallThreads - 1) / kCfftSmallThreads;
        plan.route = CFFT_SMALL;
        if (n > 2) {
            // columns per workgroup: amortise the twiddle staging, but keep >= ~6 workgroups per CU in the grid
            uint64_t cpw = 4;
            while (cpw > 1 && (n_cols + cpw - 1) / cpw < (uint64_t)n_cus * 6) cpw >>= 1;
            if (cpw > n_cols && n_cols) cpw = n_cols;
            const uint32_t tile = 1u << n, heap = 1u << (n - 1);      // the padded tile, the twiddle heap behind it (the circle layer has no entries)
            ps.threads = kCfftGenericThreads;
            ps.lds_bytes = (((tile + (tile >> 5) + 3u) & ~3u) + heap + 4u) * 4u;
            blocks = (n_cols + cpw - 1) / cpw;
            plan.route = CFFT_GENERIC;
            plan.cols_per_wg = (uint32_t)cpw;
        }
        if (n_cols > 0xffffffffu) return "cfft: too many (tile, column) work items";      // (the kernels count columns in 32 bits)
        plan.blocks = (uint32_t)blocks;
        plan.n_passes = 1;
        return nullptr;
    }

    // ---- bottom tile, strided-pass layer limit, strided tile
    CfftKnobs sh = cfft_default_shape(n, n_cols, n_cus);
    if (in_place) {
        if (kn.kb) sh.kb = kn.kb;
        if (kn.ka_max) sh.ka_max = kn.ka_max;
        if (n > sh.kb && n >= 14 && !kn.kb && !kn.ka_max) {       // n = 13 (and 14) is one bottom pass whatever the column count
            // Few columns: the default tiles (2^13 contiguous, 2^14 strided) give 2^(n-13) x cols and 2^(n-14) x cols workgroups;
            // below ~2 per CU pick the split with the most workgroups in its emptier pass (ties: the larger tiles).
            // n = 20, one column: 12 + 8 layers on 2^12-word tiles = 256 + 256 workgroups instead of 128 + 64.
            const uint64_t want = (uint64_t)2 * n_cus;
            if ((((uint64_t)1 << (n - 14)) * n_cols) < want && n - 13 <= sh.ka_max) {
                uint64_t best = 0;
                for (uint32_t tb = 13; tb >= 11; tb--) {
                    const uint32_t k = n - tb;
                    if (k < 1 || k > sh.ka_max) continue;         // one strided pass
                    const uint32_t ta = k <= 8 ? 12u : (k == 9 ? 13u : 14u);
                    if (ta > n) continue;
                    const uint64_t wa = ((uint64_t)1 << (n - ta)) * n_cols, wb = ((uint64_t)1 << (n - tb)) * n_cols;
                    uint64_t score = wa < wb ? wa : wb;
                    if (score > want) score = want;
                    if (score > best) { best = score; sh.kb = tb; sh.logta = ta; }
                }
            }
        }
        if (kn.logta) sh.logta = kn.logta;
    }

    // ---- the cut, low -> high: sh.kb bottom layers, the rest in equal strided passes of at most sh.ka_max layers
    struct { uint32_t lo, k, logt; } cut[kCfftMaxPasses];
    uint32_t np = 1;
    cut[0] = {0, n < sh.kb ? n : sh.kb, n < sh.kb ? n : sh.kb};
    if (n > sh.kb) {
        const uint32_t rem = n - sh.kb, ns = (rem + sh.ka_max - 1) / sh.ka_max;
        if (1 + ns > kCfftMaxPasses) return "cfft: more passes than a plan holds";
        uint32_t lo = sh.kb;
        for (uint32_t s = 0; s < ns; s++) {
            const uint32_t k = rem / ns + (s < rem % ns ? 1 : 0);
            uint32_t c = sh.logta - k;                // log2(words per row)
            if (c > lo) c = lo;
            cut[np++] = {lo, k, c + k};
            lo += k;
        }
    }
    // the fused extension: the top pass reads the polynomial and skips the layers that only replicate, which takes two register layers
    if (entry == CFFT_EVALUATE_EXTENDED && !(np >= 2 && (ext == 1 || ext == 2) && cut[np - 1].k >= 2)) return nullptr;

    // ---- kernels, in execution order
    plan.route = CFFT_TILED;
    plan.n_passes = np;
    const bool stream = !inverse && cfft_streams_past_cache(n_cols, n);
    for (uint32_t i = 0; i < np; i++) {
        const auto &cu = cut[inverse ? i : np - 1 - i];
        CfftPass &ps = plan.pass[i];
        ps.lo = cu.lo, ps.k = cu.k, ps.logt = cu.logt;
        ps.scale = inverse && i == np - 1;
        ps.tiles = 1u << (n - cu.logt);
        if (cu.lo == 0) {
            ps.kind = i == 0 && entry == CFFT_INTERPOLATE_TO ? CFFT_BOTTOM_OOP : stream && (cu.k == 13 || cu.k == 14) ? CFFT_BOTTOM_STREAM : CFFT_BOTTOM;
            ps.threads = 1u << (cu.k - 4);
            ps.lds_bytes = ((1u << cu.k) + (1u << (cu.k - 5)) + (1u << (cu.k - 4))) * 4u;     // padded tile + twiddle heap
            if (!cfft_shape_supported(ps.kind, ps.k, ps.logt)) return "cfft: unsupported bottom pass";
        } else {
            ps.kind = i == 0 && entry == CFFT_EVALUATE_EXTENDED ? CFFT_STRIDED_EXT : stream && cu.logt == 15 ? CFFT_STRIDED_STREAM : CFFT_STRIDED;
            ps.threads = (1u << (cu.logt - 4)) / (cu.logt == 15 ? 2 : 1);                     // 2^15: two virtual lanes per lane
            ps.lds_bytes = ((1u << cu.logt) + (1u << (cu.logt - 5)) + (1u << cu.k)) * 4u;
            if (!cfft_shape_supported(ps.kind, ps.k, ps.logt)) return "cfft: unsupported pass shape";
        }
        if ((uint64_t)ps.tiles * n_cols > 0xffffffffu) return "cfft: too many (tile, column) work items";
    }
    return nullptr;
}

}  // namespace tstwo

/*
 * tstwo_hip.h — C ABI of libtstwo_hip.so, the MI355X (gfx950) backend for tstwo's data-parallel
 * hot path.  This is the drop-in boundary: exactly the entry points a `HipBackend` for
 * teddyjfpender/tstwo binds with bun:ffi (INTEGRATION.md shows the TypeScript stub).  The reference
 * has no FFI today; each entry point below cites the TypeScript interface/function it replaces
 * (paths relative to packages/core/src of the reference).
 *
 * Conventions
 *  - Every function returns 0 on success, nonzero on failure; tstwo_last_error() then holds the
 *    reference's own error text where the reference throws (e.g. "0 has no inverse",
 *    "length is not power of two", "Not enough twiddles!") so the wrapper can `throw new Error(msg)`.
 *  - Columns are plain little-endian uint32 device buffers holding canonical M31 values in [0, P),
 *    P = 2^31-1 (M31.intoSlice layout, fields/m31.ts:272-284).  QM31 / SecureColumnByCoords data
 *    is struct-of-arrays: 4 coordinate columns (fields/secure_columns.ts:124).  Hashes are 32-byte
 *    Blake2s digests, layers are arrays of digests (vcs/blake2_hash.ts:5-49).
 *  - "dev" pointers are device addresses (from tstwo_malloc, or any HIP allocation of the same
 *    process, e.g. a torch tensor's data_ptr()).  `const uint32_t *const *cols` style arguments are
 *    HOST arrays of device pointers, borrowed for the duration of the call.
 *  - Work is enqueued on one HIP stream per process (tstwo_set_stream to borrow the caller's).
 *    Calls that hand results to host memory synchronise; the others are asynchronous and ordered
 *    on that stream; tstwo_sync() drains it.
 *  - Threading: the library is thread-compatible — one thread at a time inside it, the caller
 *    serialises calls — with one exception: tstwo_malloc / tstwo_free / tstwo_trim lock the
 *    allocator, so a block may be released from any thread (a finaliser / GC thread under ctypes or
 *    bun:ffi, which drop the interpreter lock during a call) while another thread is in a call.
 *  - No CPU fallback exists: every entry point fails with an error if no GPU is present.
 */
#ifndef TSTWO_HIP_H
#define TSTWO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSTWO_OK 0
#define TSTWO_ERR_HIP 1            /* HIP runtime failure (text has the hipError string) */
#define TSTWO_ERR_ZERO_INVERSE 2   /* "0 has no inverse"                      fields/m31.ts:139 */
#define TSTWO_ERR_NOT_POW2 3       /* "length is not power of two"            backend/cpu/index.ts:65 */
#define TSTWO_ERR_TWIDDLES 4       /* "Not enough twiddles!"                  poly/utils.ts:86 */
#define TSTWO_ERR_TOO_SMALL 5      /* "fold_line: Evaluation too small, ..."  fri.ts:127 */
#define TSTWO_ERR_LEN_MISMATCH 6   /* "fold_circle_into_line: Length mismatch ..." fri.ts:168 */
#define TSTWO_ERR_BAD_ARG 7
#define TSTWO_ERR_LOG_SIZE 8       /* "log size too small"                    backend/cpu/circle.ts:72 */
#define TSTWO_ERR_COMM 9           /* RCCL missing or failing (text has the ncclResult string) */
#define TSTWO_ERR_ZERO_VARIABLES 10 /* "Number of variables must not be zero" backend/cpu/lookups/gkr.ts:155 */

/* ---------------------------------------------------------------- lifecycle / plumbing */
int tstwo_init(int device);                 /* select GPU `device`, create the stream; idempotent */
int tstwo_shutdown(void);
const char *tstwo_last_error(void);
const char *tstwo_version(void);
int tstwo_device_count(int *out);
int tstwo_device_name(char *buf, size_t buflen);
int tstwo_set_stream(void *hip_stream);     /* borrow a caller stream (NULL = back to the library's) */
int tstwo_sync(void);
int tstwo_malloc(void **dev, size_t bytes);
int tstwo_free(void *dev);                   /* returns the block to the library's caching allocator (no sync) */
int tstwo_trim(void);                        /* synchronises and gives every cached block back to HIP */
/* Where tstwo_malloc gets its blocks.  POOL (default): size-class free lists over hipMalloc, reuse ordered on the
 * library's stream.  DIRECT: hipMalloc / hipFree per call (free synchronises).  ASYNC: HIP's stream-ordered pool
 * (hipMallocAsync / hipFreeAsync on the library's stream) — UNSAFE: on ROCm 7.2 / gfx950 that pool silently returns wrong
 * data from the second or third allocate / compute / free cycle on (reproduced without any code of this library,
 * tools/repro_hipmallocasync.hip), so tstwo_set_alloc_mode(ASYNC) and TSTWO_ALLOC=async FAIL with TSTWO_ERR_BAD_ARG unless
 * the environment holds TSTWO_ALLOW_UNSAFE_ASYNC_ALLOC=1 (for re-checking a newer runtime).  OR in POISON to have every
 * block handed out filled with 0xA5 bytes first (debugging aid: reads of memory the library never wrote stop looking right
 * by accident).  Environment, read at the first tstwo_malloc: TSTWO_ALLOC=pool|direct|async, TSTWO_POISON=1. */
#define TSTWO_ALLOC_POOL 0
#define TSTWO_ALLOC_DIRECT 1
#define TSTWO_ALLOC_ASYNC 2
#define TSTWO_ALLOC_POISON 0x10
int tstwo_set_alloc_mode(int mode);
/* The host buffer may be reused as soon as tstwo_upload returns; the copy itself is ordered on the stream (small
 * uploads travel through a page-locked ring without a host synchronisation, large ones synchronise). */
int tstwo_upload(void *dev_dst, const void *host_src, size_t bytes);
/* Host hand-over beside the kernels — the boundary createBaseFieldColumn(data) crosses (backend/index.ts:20-31,
 * backend/cpu/index.ts:85-90).  tstwo_upload is synchronous and, from pageable memory, staged by the runtime (35-39 GB/s on the
 * MI355X box).  Page-locked memory makes a copy ONE DMA at link rate, and tstwo_upload_async issues it on the library's copy
 * stream, beside the kernels of the main stream (upload of column group k+1 under the transform of group k):
 *   tstwo_host_register / _unregister   page-lock (and unlock) a range of the CALLER's memory (a Uint32Array's backing store);
 *   tstwo_host_alloc / _free            page-locked memory from the library (bun:ffi toArrayBuffer wraps it);
 *   tstwo_upload_async(dst, src, n)     enqueue the copy and return.  It starts after everything enqueued on the main stream
 *                                       BEFORE this call (a block tstwo_malloc has just recycled is no longer in use by then);
 *                                       src must stay valid and unchanged until tstwo_upload_wait / tstwo_sync returns, dst must
 *                                       not be freed before.  Pageable src works, at tstwo_upload's rate.  Refused during
 *                                       graph capture;
 *   tstwo_upload_fence()                everything enqueued on the main stream AFTER this call waits (on the device) for the
 *                                       copies issued so far; the host does not block;
 *   tstwo_upload_wait()                 the host blocks until the copies issued so far have landed. */
int tstwo_host_register(void *host, size_t bytes);
int tstwo_host_unregister(void *host);
int tstwo_host_alloc(void **host, size_t bytes);
int tstwo_host_free(void *host);
int tstwo_upload_async(void *dev_dst, const void *host_src, size_t bytes);
int tstwo_upload_fence(void);
int tstwo_upload_wait(void);
int tstwo_download(void *host_dst, const void *dev_src, size_t bytes);   /* synchronous */
/* n_pieces small device buffers in one round trip: piece i = n_bytes[i] bytes (whole 4-byte aligned words) at srcs[i]; the pieces
 * land back to back in host_out.  Up to 256 KiB in all they are packed on the device into page-locked host memory and cost one
 * stream synchronisation (the read-backs that end a FRI commit — channel state, the last layer's four coordinate columns
 * `LineEvaluation.interpolate` wants on the host, poly/line.ts:312-329 — took six); larger requests are fetched piece by piece.
 * srcs / n_bytes are host arrays.  Synchronous. */
int tstwo_download_many(const void *const *srcs, const size_t *n_bytes, size_t n_pieces, void *host_out);
int tstwo_copy(void *dev_dst, const void *dev_src, size_t bytes);        /* async d2d */
int tstwo_zero(void *dev, size_t bytes);                                  /* async; Column.zeros, backend/index.ts:56 */
/* hipGraph capture of a launch sequence (launch-bound loops: e.g. the 20+ small kernels of a FRI commit with the device
 * channel).  Between begin and end every asynchronous entry point is RECORDED on the library's stream instead of executed;
 * tstwo_graph_launch replays the recorded sequence with one call.  Rules while capturing: no entry point that returns data
 * to the host (they synchronise) and none that uploads a host array (column tables beyond 64 pointers, gather requests,
 * quotient constants: the staging slot they travel through is only valid at capture time — such a call fails with
 * TSTWO_ERR_BAD_ARG "host-array upload during graph capture" and records nothing); allocations must hit the
 * library's caching allocator (run the sequence once eagerly first); all buffers the sequence uses must outlive the
 * graph, which addresses them by value.  The library's own scratch block (the ticket, partial sums and eq tables of
 * tstwo_gkr_sum_poly_async, tstwo_gkr_round[_dev] and tstwo_gkr_gen_eq_evals live in it) is recorded by value too: a block that a
 * later call outgrows is retired, not freed, and stays mapped until tstwo_shutdown, so a graph may be replayed after any
 * eager call, however much scratch that call needed.  A captured call that would itself have to grow the block fails with
 * TSTWO_ERR_BAD_ARG "scratch growth during graph capture" and records nothing; the eager run of the sequence sizes it. */
int tstwo_graph_begin_capture(void);
int tstwo_graph_end_capture(void **graph_exec);
int tstwo_graph_launch(void *graph_exec);
int tstwo_graph_destroy(void *graph_exec);
/* HIP events on the library's stream (bench.py times kernels with these) */
int tstwo_event_create(void **ev);
int tstwo_event_record(void *ev);
int tstwo_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);    /* synchronises on ev_stop */
int tstwo_event_destroy(void *ev);

/* ---------------------------------------------------------------- field column ops
 * M31.add/sub/mul/neg applied per element (fields/m31.ts:147-173); bench/m31.bench.ts workload. */
int tstwo_m31_add(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
int tstwo_m31_sub(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
int tstwo_m31_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
int tstwo_m31_neg(const uint32_t *a, uint32_t *out, size_t n);
/* batchInverse (fields/fields.ts:66-207).  Result = elementwise inverse; any zero input fails with
 * TSTWO_ERR_ZERO_INVERSE like the reference's single final inverse().  Synchronises (error flag). */
int tstwo_m31_batch_inverse(const uint32_t *in, uint32_t *out, size_t n);
int tstwo_cm31_batch_inverse(const uint32_t *const in[2], uint32_t *const out[2], size_t n);
int tstwo_qm31_batch_inverse(const uint32_t *const in[4], uint32_t *const out[4], size_t n);
/* Deferred error reporting for a phase of many small calls: the *_async variants only enqueue the kernel; a zero input
 * sets a sticky flag in device memory instead of failing the call (the affected outputs are unspecified).
 * tstwo_check_zero_flag() synchronises ONCE, clears the flag and fails with TSTWO_ERR_ZERO_INVERSE ("0 has no
 * inverse", fields/m31.ts:139) if any call since the last check met a zero.  The synchronous calls above are
 * unchanged (= async + check). */
int tstwo_m31_batch_inverse_async(const uint32_t *in, uint32_t *out, size_t n);
int tstwo_cm31_batch_inverse_async(const uint32_t *const in[2], uint32_t *const out[2], size_t n);
int tstwo_qm31_batch_inverse_async(const uint32_t *const in[4], uint32_t *const out[4], size_t n);
int tstwo_check_zero_flag(void);
/* QM31.mul / QM31.add per element on SoA columns (fields/qm31.ts:168-233) */
int tstwo_qm31_mul(const uint32_t *const a[4], const uint32_t *const b[4], uint32_t *const out[4], size_t n);
/* AccumulationOps.accumulate: col[i] += other[i] (backend/cpu/accumulation.ts:38-49) */
int tstwo_secure_accumulate(uint32_t *const col[4], const uint32_t *const other[4], size_t n);

/* ---------------------------------------------------------------- ColumnOps.bitReverseColumn
 * In-place bit-reversal permutation of each column (backend/index.ts:20, backend/cpu/index.ts:62-79).
 * n == 0 or not a power of two -> TSTWO_ERR_NOT_POW2. */
int tstwo_bit_reverse(uint32_t *const *cols, size_t n_cols, size_t n);

/* ---------------------------------------------------------------- PolyOps.precomputeTwiddles
 * Twiddle tree of the coset (initial index `coset_initial`, log size `log_size`): 2^log_size words
 * (backend/cpu/circle.ts:210-239, poly/twiddles.ts:10-29).  itw = elementwise inverse (may be NULL).
 * Generated on the device. */
int tstwo_twiddles_build(uint32_t coset_initial, uint32_t log_size, uint32_t *tw, uint32_t *itw);

/* ---------------------------------------------------------------- PolyOps.evaluate / interpolate
 * Circle FFT over n_cols independent columns of 2^log_size words, in place, bit-reversed evaluation
 * order (backend/cpu/circle.ts:84-134 / :136-207).  The domain is CircleDomain(half coset =
 * (half_initial, log_size-1)); tw / itw is the (inverse) twiddle tree of a root coset of log
 * tw_log of which that half coset is a doubling (the wrapper checks is_doubling_of and throws
 * "twiddle tree mismatch").  evaluate expects coefficients already extended to 2^log_size
 * (tstwo_poly_extend).  The true transform (Rust-exact) is computed; the reference's log_size==3
 * output swap (circle.ts:123-131) is offered by the wrapper as a compat option, not here.
 * 1 <= log_size <= 30 = MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4; a 4 GiB column); larger sizes return
 * TSTWO_ERR_BAD_ARG. */
int tstwo_cfft_evaluate(uint32_t *const *cols, size_t n_cols, uint32_t log_size, uint32_t half_initial,
                        const uint32_t *tw, uint32_t tw_log);
int tstwo_cfft_interpolate(uint32_t *const *cols, size_t n_cols, uint32_t log_size, uint32_t half_initial,
                           const uint32_t *itw, uint32_t tw_log);
/* Out-of-place interpolate: src[i] (evaluations, read only) -> dst[i] (coefficients).  The reference's interpolate has
 * value semantics (the evaluation survives, backend/cpu/circle.ts:136-207 works on a copy); here the copy is folded into
 * the first pass.  Bit-identical to copying and calling tstwo_cfft_interpolate. */
int tstwo_cfft_interpolate_to(const uint32_t *const *src, uint32_t *const *dst, size_t n_cols, uint32_t log_size,
                              uint32_t half_initial, const uint32_t *itw, uint32_t tw_log);
/* CirclePoly.extend + evaluate (backend/cpu/circle.ts:71-134; pcs/prover.ts Rust text "Extension": evaluate_polynomials
 * on the blown-up domain) without materialising the zero padding: polys[i] = 2^log_poly coefficients (read only),
 * out[i] = 2^log_size evaluations.  Bit-identical to tstwo_poly_extend followed by tstwo_cfft_evaluate.
 * log_size < log_poly -> TSTWO_ERR_LOG_SIZE ("log size too small"). */
int tstwo_cfft_evaluate_extended(const uint32_t *const *polys, uint32_t log_poly, uint32_t *const *out, size_t n_cols,
                                 uint32_t log_size, uint32_t half_initial, const uint32_t *tw, uint32_t tw_log);
/* How many passes over HBM (= kernel launches, each reading and writing every column once) tstwo_cfft_evaluate /
 * tstwo_cfft_interpolate take for n_cols columns of 2^log_size words — the planner's own answer, for callers that price a
 * transform against the memory roofline (bench.py: roofline.launches_per_step).  Host-side only, touches no device state. */
int tstwo_cfft_plan_passes(uint32_t log_size, size_t n_cols, uint32_t *n_passes);
/* PolyOps.extend (circle.ts:71-82): dst[0..2^log_dst) = src[0..2^log_src) zero-padded.
 * log_dst < log_src -> TSTWO_ERR_LOG_SIZE ("log size too small"). */
int tstwo_poly_extend(const uint32_t *src, uint32_t log_src, uint32_t *dst, uint32_t log_dst);
/* PolyOps.eval_at_point (circle.ts:52-69): point and result are QM31 as 4 host words. */
int tstwo_eval_at_point(const uint32_t *coeffs, uint32_t log_size, const uint32_t point_x[4],
                        const uint32_t point_y[4], uint32_t out[4]);
/* The same for n_cols polynomials of one size at one point (prove_values samples every column of a tree at the same
 * out-of-domain point): one launch sequence and one read-back.  coeffs: host array of device pointers; out: 4 words per
 * column (host). */
int tstwo_eval_at_point_batch(const uint32_t *const *coeffs, size_t n_cols, uint32_t log_size, const uint32_t px[4],
                              const uint32_t py[4], uint32_t *out);
/* PolyOps.eval_at_point (backend/cpu/circle.ts:52-69) for every (column, point) pair of an opening: the reference's caller loops
 * per column over that column's points (packages/core/src/pcs/prover.ts:94-106).  Columns sampled at the same points form a
 * group; one call takes any number of groups of mixed sizes, loads every coefficient once per sweep of up to 4 points and ends
 * with one read-back.  Synchronous.
 *   coeffs        host array of device pointers: the columns of group 0, then group 1, ...  Any 4-byte alignment (one column off a
 *                 16-byte boundary puts its group on the word loads); a column may appear more than once.
 *   group_cols    columns of group g (>= 1), each of 2^group_logs[g] coefficients (log <= 31)
 *   group_points  points of group g: 1..TSTWO_EVAL_MAX_POINTS; a point may repeat
 *   points        host, 8 words per point (x[4], y[4]), the groups' points one after the other
 *   out           host, 4 words per (group, column, point), in that nesting order
 * n_groups == 0 is a no-op.  Refused with TSTWO_ERR_BAD_ARG before anything is enqueued, `out` untouched ("eval_at_points: ..."):
 * "null argument", "a group without columns", "1 to 16 points per group", "log size out of range", "point word out of range"
 * (a word >= 2^31 - 1), and a call while the stream is capturing ("host read-back during graph capture ..."). */
#define TSTWO_EVAL_MAX_POINTS 16
int tstwo_eval_at_points(const uint32_t *const *coeffs, const uint32_t *group_cols, const uint32_t *group_logs,
                         const uint32_t *group_points, size_t n_groups, const uint32_t *points, uint32_t *out);

/* ---------------------------------------------------------------- FriOps (fri.ts:93-110)
 * Twiddles come from the inverse twiddle tree `itw` (root coset log tw_log) — a FRI fold is one
 * inverse-CFFT layer followed by f0 + alpha*f1.
 * fold_line (fri.ts:120-152): in = 2^log_n rows on LineDomain(coset of log log_n, a doubling of the
 * tree's root), out = 2^(log_n-1) rows.  log_n == 0 -> TSTWO_ERR_TOO_SMALL. */
int tstwo_fri_fold_line(const uint32_t *const in[4], uint32_t log_n, const uint32_t *itw, uint32_t tw_log,
                        const uint32_t alpha[4], uint32_t *const out[4]);
/* LineEvaluation.interpolate (poly/line.ts:312-329: bit reversal, lineIfft :354-390, scaling by 1/n) of an evaluation of
 * 2^log_n <= 2^12 rows on LineDomain(coset of log log_n, a doubling of the tree's root): in = the evaluation's four coordinate
 * columns as LineEvaluation stores them (bit-reversed order), out = the LinePoly coefficients in the reference's bit-reversed
 * order, per coordinate.  The last FRI layer (fri.ts:718-754) is the caller.  Asynchronous. */
int tstwo_line_interpolate(const uint32_t *const in[4], uint32_t log_n, const uint32_t *itw, uint32_t tw_log,
                           uint32_t *const out[4]);
/* fold_circle_into_line (fri.ts:162-192): src = 2^log_n rows on a CircleDomain whose half coset is a
 * doubling of the tree's root; dst (dst_len rows) is updated in place: dst*alpha^2 + (alpha*f1 + f0).
 * dst_len != 2^(log_n-1) -> TSTWO_ERR_LEN_MISMATCH. */
int tstwo_fri_fold_circle_into_line(uint32_t *const dst[4], size_t dst_len, const uint32_t *const src[4],
                                    uint32_t log_n, const uint32_t *itw, uint32_t tw_log, const uint32_t alpha[4]);
/* Variants for a commit loop that never leaves the device: alpha_dev points to 4 words (16-byte aligned) in device memory,
 * written earlier on the stream by tstwo_channel_mix_root_draw_felt.  Same results as the by-value calls. */
int tstwo_fri_fold_line_dev(const uint32_t *const in[4], uint32_t log_n, const uint32_t *itw, uint32_t tw_log,
                            const uint32_t *alpha_dev, uint32_t *const out[4]);
int tstwo_fri_fold_circle_into_line_dev(uint32_t *const dst[4], size_t dst_len, const uint32_t *const src[4],
                                        uint32_t log_n, const uint32_t *itw, uint32_t tw_log, const uint32_t *alpha_dev);
/* FriProver.commit's whole layer loop (commitInnerLayers, fri.ts:676-716, with the Merkle / channel wiring of the Rust text) in
 * ONE call, enqueued on the library's stream with nothing read back: a tree over the coordinate columns of every circle
 * evaluation (first layer), then per line layer: mix its root and draw alpha on the device channel
 * (tstwo_channel_mix_root_draw_felt), fold (tstwo_fri_fold_*_dev), commit the folded evaluation — until the evaluation has
 * 2^log_last_layer_size rows.
 * circle_cols: host array of 4 * n_columns device pointers (coordinate columns of the circle evaluations, canonic domains whose
 * half cosets are doublings of the tree's root — the wrapper checks, as for tstwo_fri_fold_circle_into_line); col_logs: their
 * log sizes, strictly decreasing ("column sizes not decreasing" otherwise), each >= 3.  chan: the device channel state
 * (10 words); alphas: device, 4 words per drawn alpha (16-byte aligned, alphas_cap entries >= number of trees).
 * Outputs: *first_tree = the first layer's tree; out[0 .. *n_out - 2] = the inner layers (evaluation + tree, largest first);
 * out[*n_out - 1] = the last layer's evaluation (layers = NULL), which the caller interpolates (fri.ts:718-754).  Every
 * buffer returned is a tstwo_malloc block the CALLER owns (tstwo_free); on failure nothing is returned and nothing leaks. */
typedef struct {
    uint32_t log_size;                     /* the line evaluation has 2^log_size rows */
    uint32_t *cols[4];                     /* device: its coordinate columns */
    uint8_t *layers;                       /* device: the tree committed over them (tstwo_merkle_commit layout), or NULL */
} tstwo_fri_layer_out;
int tstwo_fri_commit_layers(const uint32_t *const *circle_cols, const uint32_t *col_logs, size_t n_columns, const uint32_t *itw,
                            uint32_t tw_log, uint32_t log_last_layer_size, uint32_t *chan, uint32_t *alphas, size_t alphas_cap,
                            uint8_t **first_tree, tstwo_fri_layer_out *out, size_t out_cap, size_t *n_out);
/* Blake2sChannel on the device (channel/blake2.ts:25-224; Rust draw semantics).  chan = 10 words of device memory:
 * digest[8], n_challenges, n_sent (upload the host channel's state, download it back when done).
 * root != NULL: mix_root (vcs/blake2_merkle.ts:28-31) of the 32 bytes at `root` (device memory, e.g. byte 0 of a
 * tstwo_merkle_commit layers buffer).  felt != NULL: draw_felt into the 4 words at `felt` (device memory).
 * Asynchronous: later calls on the stream see the results; nothing reaches the host. */
int tstwo_channel_mix_root_draw_felt(uint32_t *chan, const uint8_t *root, uint32_t *felt);
/* Row shards of a FRI layer for multi-GPU provers (SURVEY.md 8e "contiguous row sharding"; output i of fri.ts:120-192
 * depends on inputs 2i, 2i+1 only).  `in`/`src` hold input rows [2*row_offset, 2*(row_offset+n_rows)) and `out`/`dst`
 * output rows [row_offset, row_offset+n_rows) of a layer of 2^log_n input rows.  row_offset and n_rows are multiples
 * of 4 (TSTWO_ERR_BAD_ARG otherwise).  The concatenation over shards equals tstwo_fri_fold_line /
 * tstwo_fri_fold_circle_into_line on the whole layer. */
int tstwo_fri_fold_line_rows(const uint32_t *const in[4], uint32_t log_n, size_t row_offset, size_t n_rows,
                             const uint32_t *itw, uint32_t tw_log, const uint32_t alpha[4], uint32_t *const out[4]);
int tstwo_fri_fold_circle_into_line_rows(uint32_t *const dst[4], const uint32_t *const src[4], uint32_t log_n,
                                         size_t row_offset, size_t n_rows, const uint32_t *itw, uint32_t tw_log,
                                         const uint32_t alpha[4]);
/* Variants taking the n/2 per-output inverse twiddles explicitly (domains that are not a doubling
 * of a precomputed tree, and log_n < 3 for the circle fold). */
int tstwo_fri_fold_line_tw(const uint32_t *const in[4], uint32_t log_n, const uint32_t *inv_x,
                           const uint32_t alpha[4], uint32_t *const out[4]);
int tstwo_fri_fold_circle_into_line_tw(uint32_t *const dst[4], size_t dst_len, const uint32_t *const src[4],
                                       uint32_t log_n, const uint32_t *inv_y, const uint32_t alpha[4]);
/* decompose (backend/cpu/fri.ts:97-164): lambda (host, 4 words) and g = f -/+ lambda per half. */
int tstwo_fri_decompose(const uint32_t *const in[4], size_t n, uint32_t *const out[4], uint32_t lambda[4]);

/* ---------------------------------------------------------------- MerkleOps (vcs/ops.ts:16-26)
 * commitOnLayer: node i = Blake2s( [prev[2i] || prev[2i+1]]  ||  LE32(cols[0][i]) || ... ), i < 2^log_size
 * (vcs/blake2_merkle.ts:9-24).  prev = NULL for the bottom layer.  out: 2^log_size * 32 bytes (device). */
int tstwo_merkle_commit_layer(uint32_t log_size, const uint8_t *prev, const uint32_t *const *cols,
                              size_t n_cols, uint8_t *out);
/* MerkleProver.commit (vcs/prover.ts:13-30): columns of mixed log sizes join at their layer (input
 * order kept within a size class).  layers (device) receives every layer, root first: layer k (2^k
 * digests) starts at byte offset 32*(2^k - 1); total 32*(2^(max_log+1) - 1) bytes.  root (host, 32 B)
 * may be NULL (then nothing is synchronised).  n_cols == 0 -> one hash of the empty message. */
int tstwo_merkle_commit(const uint32_t *const *cols, const uint32_t *log_sizes, size_t n_cols,
                        uint8_t *layers, uint8_t root[32]);
/* Several trees in one launch sequence (a TreeVec committed together, pcs/prover.ts:62-64: the 8 trees of 32 columns that
 * BASELINE config 5's trace makes on one GPU).  Request r = the arguments of tstwo_merkle_commit for tree r; every tree's layers
 * buffer receives exactly what tstwo_merkle_commit writes.  When the trees share one shape the static leaf kernel serves (16,
 * 32, 48 or 64 columns of one log size >= 17; at most 8 trees, 256 columns in all) each launch covers all of them, so that
 * the latency-bound top of the trees (layers below 2^19 nodes) runs side by side instead of 8 times in a row; any other input
 * is committed tree by tree.  roots (host, n_trees * 32 bytes) may be NULL (then nothing is synchronised). */
typedef struct {
    const uint32_t *const *cols;           /* host array of n_cols device column pointers */
    const uint32_t *log_sizes;
    size_t n_cols;
    uint8_t *layers;                       /* device: tstwo_merkle_layers_bytes(max log) bytes */
} tstwo_commit_request;
int tstwo_merkle_commit_many(const tstwo_commit_request *reqs, size_t n_trees, uint8_t *roots);
size_t tstwo_merkle_layers_bytes(uint32_t max_log);
/* MerkleProver.decommit (vcs/prover.ts:32-109) on a tree built by tstwo_merkle_commit: `layers` is that call's buffer,
 * `cols` / `col_log_sizes` the same columns in the same order.  Query set k = n_queries[k] ascending positions
 * queries[k][] (host) into the layer of log size query_logs[k].  Outputs (host): the queried column values (layer by
 * layer from the largest, node by node, column by column — the order MerkleVerifier.verify consumes), the hash
 * witness (32 bytes each) and the column witness.  The three size_t are in/out: capacity in elements on entry, count on
 * return; if a buffer is too small the counts are returned with TSTWO_ERR_BAD_ARG and nothing is written. */
int tstwo_merkle_decommit(const uint8_t *layers, uint32_t max_log, const uint32_t *const *cols,
                          const uint32_t *col_log_sizes, size_t n_cols, const uint32_t *query_logs,
                          const uint64_t *const *queries, const size_t *n_queries, size_t n_query_sets,
                          uint32_t *queried_values, size_t *n_queried, uint8_t *hash_witness, size_t *n_hashes,
                          uint32_t *column_witness, size_t *n_column_witness);
/* The same for several trees in ONE round trip (all layers of a FRI proof; all trees of a commitment scheme).  Outputs are the
 * per-request outputs concatenated in request order; counts[3r..3r+2] = (queried values, hashes, column-witness words) of
 * request r; totals[3] is in/out (capacities in elements / required sizes), like the single-tree call. */
typedef struct {
    const uint8_t *layers;                 /* device: the tree's tstwo_merkle_commit buffer */
    uint32_t max_log;
    const uint32_t *const *cols;           /* host array of device column pointers */
    const uint32_t *col_log_sizes;
    size_t n_cols;
    const uint32_t *query_logs;            /* query set k: n_queries[k] ascending positions queries[k][] of layer query_logs[k] */
    const uint64_t *const *queries;
    const size_t *n_queries;
    size_t n_query_sets;
} tstwo_decommit_request;
int tstwo_merkle_decommit_many(const tstwo_decommit_request *reqs, size_t n_reqs, uint32_t *queried_values,
                               uint8_t *hash_witness, uint32_t *column_witness, size_t *counts, size_t totals[3]);
/* FriProver.decommit_on_queries (fri.ts:768-785) for a whole FRI proof in ONE round trip: per layer the position logic of
 * computeDecommitmentPositionsAndWitnessEvals (fri.ts:346-384), the witness evaluations, and the Merkle decommitment of the
 * layer's tree at those positions (the queried values are not part of a FriLayerProof, fri.ts:262-269).
 * layers[0] = the first layer: n_evals circle evaluations (possibly of several sizes) under one tree, each queried at the
 * positions folded to its own size (fri.ts:470-480) with fold step `first_fold_step` (CIRCLE_TO_LINE_FOLD_STEP = 1);
 * layers[1..] = the inner layers: one line evaluation each, queried at the positions folded so far, with `fold_step`
 * (FOLD_STEP = 1).  cols: host array of 4 * n_evals device pointers — the coordinate columns of each evaluation in the order
 * the tree was committed with (tstwo_merkle_commit).  queries: ascending distinct positions in [0, 2^log_domain_size).
 * Outputs (host), concatenated layer by layer: witness_evals (4 words per evaluation, in the order fri.ts:346-384 pushes
 * them; first layer: evaluation by evaluation), hash_witness (32 bytes each), column_witness; counts[3r..3r+2] = (witness
 * evaluations, hashes, column-witness words) of layer r; totals[3] is in/out (capacities / required sizes) like
 * tstwo_merkle_decommit_many.  commitments (host, n_layers * 32 bytes, may be NULL): every tree's root
 * (FriLayerProof.commitment) in the same round trip. */
typedef struct {
    const uint8_t *layers;                 /* device: the layer's tstwo_merkle_commit buffer */
    uint32_t max_log;                      /* log size of the tree */
    const uint32_t *const *cols;           /* host array of 4 * n_evals device column pointers */
    const uint32_t *eval_logs;             /* log size of each evaluation */
    size_t n_evals;
} tstwo_fri_layer;
int tstwo_fri_decommit(const tstwo_fri_layer *layers, size_t n_layers, const uint64_t *queries, size_t n_queries,
                       uint32_t log_domain_size, uint32_t first_fold_step, uint32_t fold_step, uint32_t *witness_evals,
                       uint8_t *hash_witness, uint32_t *column_witness, uint8_t *commitments, size_t *counts, size_t totals[3]);
/* Gather for MerkleProver.decommit (vcs/prover.ts:32-109): item i = `words` consecutive uint32 words starting at
 * word index idx[i]*words of the device buffer srcs[i] (a column: words = 1; a layer of digests: words = 8).
 * Results land contiguously in host_out (n_items * words words).  srcs / idx are host arrays.  Synchronises. */
int tstwo_gather_words(const void *const *srcs, const uint64_t *idx, uint32_t words, size_t n_items, uint32_t *host_out);

/* ---------------------------------------------------------------- GrindOps (backend/cpu/grind.ts:31-42, proof_of_work.ts)
 * Smallest nonce >= start_nonce such that Blake2sChannel.mix_u64(nonce) applied to a channel with digest `digest`
 * yields a digest with at least pow_bits trailing zero bits (channel/blake2.ts:96-111: the first 16 digest bytes read
 * as a little-endian u128).  The reference's sequential loop returns the same (first) nonce.  Synchronises.
 * Nonce 2^64 - 1 is never tested and never returned (it is the search's "none found" value): the search covers
 * [start_nonce, 2^64 - 2], in batches whose sizes csrc/grind_plan.h sets, and one that reaches 2^64 - 1 without a hit — at once for
 * start_nonce = 2^64 - 1 — fails with TSTWO_ERR_BAD_ARG "grind: nonce space exhausted", *nonce_out untouched.  Refused likewise:
 * pow_bits > 128, a null digest or nonce_out.  The same holds for tstwo_grind_poseidon252 below. */
int tstwo_grind_blake2s(const uint8_t digest[32], uint32_t pow_bits, uint64_t start_nonce, uint64_t *nonce_out);

/* ---------------------------------------------------------------- Poseidon252 Merkle channel
 * The second MerkleChannel of the reference (vcs/poseidon252_merkle.ts, channel/poseidon.ts, backend/cpu/poseidon252.ts):
 * Starknet's Poseidon over F_p, p = 2^251 + 17*2^192 + 1 (Hades permutation, width 3, 8 full + 83 partial rounds).
 * An element (FieldElement252) in device memory and across this ABI is 8 little-endian uint32 limbs, least significant first,
 * canonical (< p): 32 bytes, the size of a Blake2s digest.  A Poseidon tree therefore has exactly the tstwo_merkle_commit layout
 * (layer k at byte 32*(2^k - 1), root first), and tstwo_merkle_decommit[_many], tstwo_gather_words and tstwo_fri_decommit work
 * on its buffer unchanged: they only gather (the hash witness comes back as 32-byte limb records).
 * hash_many(v) = poseidonHashMany (@scure/starknet, used by poseidon252_merkle.ts:52 and poseidon.ts:246,283): append 1, then
 * 0 if the length is odd; from s = (0,0,0), per pair (x, y): s0 += x, s1 += y, permute; result s0.
 * hashNode (vcs/poseidon252_merkle.ts:22-58): hash_many([left, right (if children)] + blocks), one block per 8 columns
 * (zero-padded): sum of v_k * 2^(31*(7-k)), the first column most significant.
 * tstwo_poseidon252_hash_many: message i = in[i*felts_per_msg .. (i+1)*felts_per_msg) (elements of 8 words, device, each
 * canonical — not checked), out[i] = hash_many(message i) (device, 8 words each).  Asynchronous. */
int tstwo_poseidon252_hash_many(const uint32_t *in, size_t n_msgs, uint32_t felts_per_msg, uint32_t *out);
/* CpuPoseidon252MerkleOps.commitOnLayer (backend/cpu/poseidon252.ts:44-78): node i = hashNode((prev[2i], prev[2i+1]) or none,
 * cols[..][i]), i < 2^log_size.  prev = NULL for the bottom layer.  out: 2^log_size * 32 bytes (device).  Asynchronous. */
int tstwo_poseidon252_merkle_commit_layer(uint32_t log_size, const uint8_t *prev, const uint32_t *const *cols,
                                          size_t n_cols, uint8_t *out);
/* MerkleProver.commit (vcs/prover.ts:13-30) over Poseidon252: the contract of tstwo_merkle_commit (mixed sizes join at their
 * layer, input order kept within a size class, layers buffer of tstwo_merkle_layers_bytes(max log) bytes, root (host, 32 bytes:
 * the 8 limbs) may be NULL); n_cols == 0 gives hashNode(None, []) = hash_many([]). */
int tstwo_poseidon252_merkle_commit(const uint32_t *const *cols, const uint32_t *log_sizes, size_t n_cols,
                                    uint8_t *layers, uint8_t root[32]);
/* GrindOps over Poseidon252Channel (backend/cpu/grind.ts:31-42): smallest nonce >= start_nonce such that mix_u64(nonce)
 * (= mix_u32s([0,0,0,0,0,hi,lo]), channel/poseidon.ts:294-307: hash_many([digest, nonce])) gives a digest with at least
 * pow_bits trailing zeros as channel/poseidon.ts:209-229 counts them: the first 16 bytes of the big-endian encoding read as a
 * little-endian u128, so counting starts at bit 248 of the element.  digest: host, 8 limbs, canonical.  Synchronises. */
int tstwo_grind_poseidon252(const uint32_t digest[8], uint32_t pow_bits, uint64_t start_nonce, uint64_t *nonce_out);
/* The same hashes with 8 lanes per hash instead of one (csrc/felt252_coop.cuh): a lone permutation, or a layer too small to fill
 * the device, waits for one lane's instruction stream in the entries above and for a fraction of it here.
 * tstwo_poseidon252_hash_many_coop: poseidonHashMany (@scure/starknet) with exactly the contract of tstwo_poseidon252_hash_many. */
int tstwo_poseidon252_hash_many_coop(const uint32_t *in, size_t n_msgs, uint32_t felts_per_msg, uint32_t *out);
/* CpuPoseidon252MerkleOps.commitOnLayer (backend/cpu/poseidon252.ts:44-78) with exactly the contract of
 * tstwo_poseidon252_merkle_commit_layer: any n_cols, prev may be NULL, one block per 8 columns. */
int tstwo_poseidon252_merkle_commit_layer_coop(uint32_t log_size, const uint8_t *prev, const uint32_t *const *cols,
                                               size_t n_cols, uint8_t *out);
/* Poseidon252Channel on the device (channel/poseidon.ts:122-360; mix_root: vcs/poseidon252_merkle.ts:146-178).  chan = 10 words
 * of device memory: the digest's 8 limbs (canonical), n_challenges, n_sent — the shape of the Blake2s device channel.
 * root != NULL: digest = hash_many([digest, root]) of the element at `root` (device memory, e.g. byte 0 of a Poseidon tree's
 * layers buffer), n_challenges += 1, n_sent = 0.  felt != NULL: draw_felt into the 4 words at `felt` (device memory): the first
 * four of the eight 31-bit slices of poseidonHash(digest, n_sent), least significant first, each reduced as M31.reduce does;
 * n_sent += 1.  One wave.  Asynchronous: later calls on the stream see the results; nothing reaches the host. */
int tstwo_poseidon252_channel_mix_root_draw_felt(uint32_t *chan, const uint8_t *root, uint32_t *felt);
/* FriProver.commit's whole layer loop (commitInnerLayers, fri.ts:676-716) over Poseidon252 trees and the Poseidon252 device
 * channel: the arguments, outputs, ownership, error texts and failure behaviour of tstwo_fri_commit_layers (every check before
 * the first allocation; on failure nothing is returned, nothing leaks, the channel and the alphas are as they were).  chan: the
 * 10 words of tstwo_poseidon252_channel_mix_root_draw_felt.  Trees have the tstwo_merkle_commit layout. */
int tstwo_fri_commit_layers_poseidon252(const uint32_t *const *circle_cols, const uint32_t *col_logs, size_t n_columns,
                                        const uint32_t *itw, uint32_t tw_log, uint32_t log_last_layer_size, uint32_t *chan,
                                        uint32_t *alphas, size_t alphas_cap, uint8_t **first_tree, tstwo_fri_layer_out *out,
                                        size_t out_cap, size_t *n_out);

/* ---------------------------------------------------------------- QuotientOps
 * accumulateQuotients row loop (backend/cpu/quotients.ts:52-116,160-178) with the per-batch constants
 * computed by the wrapper (quotientConstants, quotients.ts:124-191; constraints.ts:117-128):
 *   batch b covers entries [batch_off[b], batch_off[b+1]) of col_idx / abc;
 *   abc[3*j..3*j+2] = (alpha^j a, alpha^j b, alpha^j c) as QM31 (4 words each);
 *   den_b(row) = (prx[b] - p.x) * piy[b] - (pry[b] - p.y) * pix[b]  in CM31 (2 words each);
 *   acc = acc * batch_coeff[b] + num_b * den_b^-1.
 * Domain = CircleDomain(half coset (half_initial, log_size-1)), rows in bit-reversed order.
 * All constant arrays are host memory.  A vanishing denominator fails with TSTWO_ERR_ZERO_INVERSE. */
int tstwo_quotients_accumulate(uint32_t half_initial, uint32_t log_size, const uint32_t *const *cols,
                               size_t n_cols, size_t n_batches, const uint32_t *batch_off,
                               const uint32_t *col_idx, const uint32_t *abc, const uint32_t *batch_coeff,
                               const uint32_t *prx, const uint32_t *pry, const uint32_t *pix,
                               const uint32_t *piy, uint32_t *const out[4]);
/* The same from the samples themselves: the quotient constants (quotientConstants, backend/cpu/quotients.ts:124-152,183-191;
 * complexConjugateLineCoeffs, constraints.ts:117-128; Rust conjugation semantics) are computed by the library.
 * points: 8 words per batch (QM31 x, QM31 y); values: 4 words per entry; batch b owns entries [batch_off[b], batch_off[b+1]).
 * A sample point equal to its own conjugate -> TSTWO_ERR_BAD_ARG "Cannot evaluate a line with a single point". */
int tstwo_quotients_accumulate_samples(uint32_t half_initial, uint32_t log_size, const uint32_t *const *cols, size_t n_cols,
                                       size_t n_batches, const uint32_t *batch_off, const uint32_t *col_idx,
                                       const uint32_t *points, const uint32_t *values, const uint32_t random_coeff[4],
                                       uint32_t *const out[4]);
/* The same two calls without the read-back: a vanishing denominator sets the sticky zero flag (tstwo_check_zero_flag). */
int tstwo_quotients_accumulate_async(uint32_t half_initial, uint32_t log_size, const uint32_t *const *cols,
                                     size_t n_cols, size_t n_batches, const uint32_t *batch_off,
                                     const uint32_t *col_idx, const uint32_t *abc, const uint32_t *batch_coeff,
                                     const uint32_t *prx, const uint32_t *pry, const uint32_t *pix,
                                     const uint32_t *piy, uint32_t *const out[4]);
int tstwo_quotients_accumulate_samples_async(uint32_t half_initial, uint32_t log_size, const uint32_t *const *cols,
                                             size_t n_cols, size_t n_batches, const uint32_t *batch_off,
                                             const uint32_t *col_idx, const uint32_t *points, const uint32_t *values,
                                             const uint32_t random_coeff[4], uint32_t *const out[4]);

/* ---------------------------------------------------------------- multi-GPU: the one exchange on the path
 * Column sharding: rank g commits its own Merkle tree over its own trace columns and the ranks all-gather the
 * 32-byte roots, which every rank then mixes into its channel in rank order (TreeVec order; pcs/prover.ts:62-64,227-228).
 * One process per GPU; the collective is RCCL's ncclAllGather over xGMI, enqueued on the library's stream behind the
 * kernels that produce the root (asynchronous: no host synchronisation).  RCCL is bound at run time (dlopen), so
 * single-GPU hosts need no librccl.
 *   rank 0: tstwo_comm_unique_id(id); the 128 bytes travel to the other ranks by any host channel (file, socket, env);
 *   every rank: tstwo_comm_init(rank, world, id)        — collective, returns when all ranks have joined;
 *   per commit: tstwo_allgather_roots(layers (byte 0 = root), roots_out (world * 32 bytes, device)).
 * Without a communicator (a world of one) the gathers degenerate to a device copy.  tstwo_allgather moves any small
 * per-rank record the same way (the subtree roots of a row-sharded FRI layer). */
#define TSTWO_COMM_ID_BYTES 128
int tstwo_comm_unique_id(uint8_t id[TSTWO_COMM_ID_BYTES]);
int tstwo_comm_init(int rank, int world, const uint8_t id[TSTWO_COMM_ID_BYTES]);
int tstwo_comm_destroy(void);
int tstwo_comm_info(int *rank, int *world);
int tstwo_allgather_roots(const uint8_t *root_dev, uint8_t *roots_out_dev);
int tstwo_allgather(const void *send_dev, void *recv_dev, size_t bytes_per_rank);
/* Overlapped form: the collective runs on a second stream of the library, behind everything enqueued so far, while later
 * calls (the next commit's CFFT) proceed on the main stream.  Neither buffer may be touched by later work until
 * tstwo_comm_wait() has been called: it makes the main stream wait (on the device, not the host) for the last async
 * collective; tstwo_sync() after it covers both. */
int tstwo_allgather_async(const void *send_dev, void *recv_dev, size_t bytes_per_rank);
int tstwo_comm_wait(void);

/* ---------------------------------------------------------------- GkrOps / MleOps (lookups, LogUp-GKR)
 * backend/index.ts:93-95 (GkrOps), backend/cpu/lookups/gkr.ts:84-358, backend/cpu/lookups/mle.ts:60-130.
 * An Mle<SecureField> is 4 SoA columns (SecureColumnByCoords layout), an Mle<BaseField> one column, of 2^log_n values; the
 * first variable is the most significant bit of the index.  Scalars (y entries, v, lambda, r) are QM31 as 4 host words.
 * Layer kinds (gkr_prover.ts Layer) for the `kind` arguments: */
#define TSTWO_GKR_GRAND_PRODUCT 0
#define TSTWO_GKR_LOGUP_GENERIC 1          /* secure numerators */
#define TSTWO_GKR_LOGUP_MULTIPLICITIES 2   /* base numerators: only num[0] is read */
#define TSTWO_GKR_LOGUP_SINGLES 3          /* numerators are 1: num is not read (may hold NULLs) */
/* GkrOps.genEqEvals (gkr.ts:90-104): out[x] = v * eq(x, y) for x in {0,1}^n_y, y = n_y QM31 values (4 words each, host),
 * n_y <= 28. */
int tstwo_gkr_gen_eq_evals(const uint32_t *y, uint32_t n_y, const uint32_t v[4], uint32_t *const out[4]);
/* GkrOps.nextLayer (gkr.ts:109-137, 317-358), log_n >= 1: out[i] from in[2i], in[2i+1].  Grand product: the QM31 product.
 * LogUp (kind 1-3): fraction addition (n0 d1 + n1 d0, d0 d1) into secure out_num / out_den — every LogUp kind yields
 * LogUpGeneric; nothing is inverted, zero denominators are legal. */
int tstwo_gkr_next_layer_grand_product(const uint32_t *const in[4], uint32_t log_n, uint32_t *const out[4]);
int tstwo_gkr_next_layer_logup(uint32_t kind, const uint32_t *const num[4], const uint32_t *const den[4], uint32_t log_n,
                               uint32_t *const out_num[4], uint32_t *const out_den[4]);
/* GkrOps.sumAsPolyInFirstVariable before its eq_fixed_var_correction and correct_sum_as_poly_in_first_variable steps (the
 * evalGrandProductSum / evalLogupSum / evalLogupSinglesSum loops of gkr.ts:185-311): out = (f(0), f(2)) as 8 words, f summed
 * over n_terms = 2^(n_vars-1) terms of a layer of 2^(n_vars+1) values (grand product: the layer is `den`), reading
 * eq[0 .. n_terms).  n_vars == 0 fails with TSTWO_ERR_ZERO_VARIABLES.  The synchronous form writes host memory; the async form
 * writes 8 words of device memory and returns with the launch enqueued. */
int tstwo_gkr_sum_poly(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                       uint32_t n_vars, const uint32_t lambda[4], uint32_t out[8]);
int tstwo_gkr_sum_poly_async(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                             uint32_t n_vars, const uint32_t lambda[4], uint32_t *out_dev);
/* One round of the batched sumcheck of prove_batch (gkr_prover.ts:313-336 fixFirstVariable, then sumAsPolyInFirstVariable) in
 * one launch: the layer num / den (2^(n_vars+2) values) has its first variable fixed to r, written to out_num / out_den (in place
 * when they are num / den; base numerators go to a separate secure out_num), and the (f(0), f(2)) of the folded layer with
 * n_vars variables goes to out_dev as in the async sum above. */
int tstwo_gkr_round(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                    uint32_t *const out_num[4], uint32_t *const out_den[4], uint32_t n_vars, const uint32_t r[4],
                    const uint32_t lambda[4], uint32_t *out_dev);
/* MleOps.fixFirstVariable (mle.ts:68-130, lookups/utils.ts:256 foldMleEvals): out[i] = in[i] + r (in[i + n/2] - in[i]),
 * 2^(log_n-1) secure outputs.  The secure form may run in place (out == in). */
int tstwo_mle_fix_first_variable_base(const uint32_t *in, uint32_t log_n, const uint32_t r[4], uint32_t *const out[4]);
int tstwo_mle_fix_first_variable_secure(const uint32_t *const in[4], uint32_t log_n, const uint32_t r[4], uint32_t *const out[4]);
/* The same three with the challenge r read from device memory: r_dev = 4 words, 16-byte aligned, written earlier on the stream
 * (the challenge_out of tstwo_gkr_round_finish).  Same contracts and results as the by-value calls; lambda stays by value. */
int tstwo_gkr_round_dev(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                        uint32_t *const out_num[4], uint32_t *const out_den[4], uint32_t n_vars, const uint32_t *r_dev,
                        const uint32_t lambda[4], uint32_t *out_dev);
int tstwo_mle_fix_first_variable_base_dev(const uint32_t *in, uint32_t log_n, const uint32_t *r_dev, uint32_t *const out[4]);
int tstwo_mle_fix_first_variable_secure_dev(const uint32_t *const in[4], uint32_t log_n, const uint32_t *r_dev, uint32_t *const out[4]);
/* Mle.evalAtPoint (lookups/mle.ts:81-114) of n_mles base MLEs of 2^log_n values at one point:
 * out[4k .. 4k+4) = sum_i mles[k][i] prod_j (bit_{n-1-j}(i) ? p_j : 1 - p_j), p_j = point[4j .. 4j+4) (host, 4 log_n words);
 * log_n = 0 gives mles[k][0] (mle.ts:83-88).  One pass over the input (4 bytes per value) and one read-back for the whole batch;
 * synchronous, `out` is host memory (4 n_mles words).  Columns may have any 4-byte alignment; one column may be named twice.
 * Refused with TSTWO_ERR_BAD_ARG before anything is enqueued ("mle eval_at_point: ..."): n_mles = 0 ("no MLE given") or above
 * 32768, log_n > 28 ("more than 28 variables"), a null pointer, a point word >= 2^31 - 1 ("point word out of range"), a call
 * during graph capture. */
int tstwo_mle_eval_at_point_base(const uint32_t *const *mles, size_t n_mles, uint32_t log_n, const uint32_t *point, uint32_t *out);
/* Mle.evalAtPoint (lookups/mle.ts:81-114) of n_mles secure MLEs: cols = 4 n_mles device pointers, MLE k = cols[4k .. 4k+4)
 * (SecureColumnByCoords); 16 bytes per value.  Everything else as the base form. */
int tstwo_mle_eval_at_point_secure(const uint32_t *const *cols, size_t n_mles, uint32_t log_n, const uint32_t *point, uint32_t *out);
/* The denominators of a LogUp-GKR input layer (gkr_prover.ts Layer, LogUp kinds) from trace columns; the reference does not
 * define this step, it follows Rust stwo's LookupElements::combine over whole columns:
 * out[r] = sum_t coeffs[4t .. 4t+4) * cols[t][r] + constant for r < 2^log_n,
 * the denominator of a tstwo_logup_frac written out as a secure MLE.  Elementwise: the row order of the inputs is the order of
 * the MLE.  1 <= n_terms <= TSTWO_LOGUP_MAX_TERMS ("1 to 16 terms"), log_n <= 28, host words < 2^31 - 1 ("... out of range"), an
 * output column that overlaps an input is refused ("an output column is also an input").  Asynchronous. */
int tstwo_gkr_logup_denominators(const uint32_t *const *cols, const uint32_t *coeffs, size_t n_terms, const uint32_t constant[4],
                                 uint32_t log_n, uint32_t *const out[4]);
/* The end of one round of the batched sum-check of prove_batch (sumcheck.ts:99-227 with the oracles of gkr_prover.ts:290-420), in
 * one single-wave launch and without a read-back: everything the host does between the sums of a round and the launches of the
 * next.  Asynchronous.
 *   chan             device: the Blake2s channel, 10 words (digest[8], n_challenges, n_sent), Rust draw semantics; updated
 *   sums             device: 8 words per instance, the (f(0), f(2)) slot of tstwo_gkr_sum_poly_async / tstwo_gkr_round[_dev]; read
 *                    for active instances only
 *   state            device: 8 words per instance, claim[4] then eq correction[4]; updated in place
 *   n_instances      1 .. 64;  active_mask: bit i set = instance i's oracle takes part in this round (else it contributes the
 *                    constant claim_i / 2)
 *   y_k, inv_eq0     host words: y[n - k] and a = 1 / eq({0}^(n-k+1), y[:n-k+1]) of correctSumAsPolyInFirstVariable
 *                    (gkr_prover.ts:609-660)
 *   alpha            host words: the sum-check's batching challenge
 *   round_poly_out   device, 20 words: word 0 = n_coeffs (index of the highest non-zero coefficient + 1: the coefficients the
 *                    channel mixed), words 1-3 = 0, words 4..19 = the 4 coefficients of sum_i alpha^i p_i (zero from n_coeffs on)
 *   challenge_out    device, 4 words: the challenge drawn after mixing the round polynomial (the next round's r_dev)
 * Per instance: p_i = the corrected round polynomial through (0, r0), (1, claim - r0), (2, r2), (b, 0) or claim_i / 2;
 * claim_i <- p_i(challenge); correction_i <- correction_i * eq(challenge, y_k) for active instances.  sums, state, round_poly_out
 * and challenge_out are 16-byte aligned.  A y_k for which the reference divides by zero (0, 1, 1/2, 1/3) fails with
 * TSTWO_ERR_BAD_ARG "sum-check: degenerate eq point" before anything is enqueued. */
int tstwo_gkr_round_finish(uint32_t *chan, const uint32_t *sums, uint32_t *state, uint32_t n_instances, uint64_t active_mask,
                           const uint32_t y_k[4], const uint32_t inv_eq0[4], const uint32_t alpha[4], uint32_t *round_poly_out,
                           uint32_t *challenge_out);

/* ---- prove_batch without a read-back between its layers (gkr_prover.ts:440-580).  The building blocks below take every scalar
 * the protocol produces (the out-of-domain point, alpha, lambda, the eq corrections) from DEVICE words an earlier launch on the
 * stream wrote; all are asynchronous, read nothing back, and give the words of their by-value twins.  Device scalars are 4 words,
 * 16-byte aligned; a null or misaligned one fails with TSTWO_ERR_BAD_ARG before anything is enqueued. */
/* tstwo_gkr_gen_eq_evals (gkr.ts:90-104) with y (4 n_y words; may be null for n_y = 0) and v in device memory. */
int tstwo_gkr_gen_eq_evals_dev(const uint32_t *y_dev, uint32_t n_y, const uint32_t *v_dev, uint32_t *const out[4]);
/* tstwo_gkr_sum_poly_async / tstwo_gkr_round_dev (gkr.ts:142-311, gkr_prover.ts:313-336) with lambda in device memory. */
int tstwo_gkr_sum_poly_async_ldev(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                                  uint32_t n_vars, const uint32_t *lambda_dev, uint32_t *out_dev);
int tstwo_gkr_round_dev_ldev(uint32_t kind, const uint32_t *const eq[4], const uint32_t *const num[4], const uint32_t *const den[4],
                             uint32_t *const out_num[4], uint32_t *const out_den[4], uint32_t n_vars, const uint32_t *r_dev,
                             const uint32_t *lambda_dev, uint32_t *out_dev);
/* The status word of the entries below: bits are ORed in, never cleared. */
#define TSTWO_GKR_STATUS_DEGENERATE 1u   /* an eq point at which correctSumAsPolyInFirstVariable divides by zero */
/* tstwo_gkr_round_finish (sumcheck.ts:99-227, gkr_prover.ts:609-660) with y_k, inv_eq0 and alpha in device memory.  A device y_k
 * cannot be refused before the launch: for y_k in {0, 1, 1/2, 1/3} the kernel sets TSTWO_GKR_STATUS_DEGENERATE in *status (one
 * device word) and still finishes — it stores nothing outside its outputs, whose contents are then unspecified. */
int tstwo_gkr_round_finish_dev(uint32_t *chan, const uint32_t *sums, uint32_t *state, uint32_t n_instances, uint64_t active_mask,
                               const uint32_t *y_k_dev, const uint32_t *inv_eq0_dev, const uint32_t *alpha_dev,
                               uint32_t *round_poly_out, uint32_t *challenge_out, uint32_t *status);
/* One LANE of the two transcript kernels: an instance that is active in the layer (lanes are the active instances in instance
 * order, as sumcheck.ts batches them).  An array of these lives in device memory.
 *   src      the columns the layer's mask is read from (numerators [0..4), denominators [4..8); words 0 and 1 of each): the
 *            folded 2-point layer, or the instance's 1-variable layer where it enters at this layer
 *   kind     of that layer: GRAND_PRODUCT (one column: src[4..8)), LOGUP_GENERIC (two), LOGUP_SINGLES ((1, 1), then src[4..8))
 *   inst     the instance's index: where its claims live in `claims` / `output_claims` (8 words per instance)
 *   shift    layer_begin: the sum-check claim is doubled n_rounds - n_variables times (any value: the factor is 2^(shift mod 31),
 *            which is 2^shift in M31)
 *   enter    layer_begin: non-zero = the instance enters here; its output values are word 0 of out_src (as src; numerators are
 *            read unless kind is GRAND_PRODUCT) */
typedef struct {
    const uint32_t *src[8];
    uint32_t inst, kind, shift, enter;
    const uint32_t *out_src[8];
} tstwo_gkr_lane;
/* The top of a layer of prove_batch (gkr_prover.ts:452-500) by one wave: the output values of the entering lanes (stored to
 * output_claims and taken as their claims to verify), mix_felts of every lane's claims to verify (one mix per lane, in order), the
 * draws of alpha then lambda (claims is only read: entering lanes store to output_claims), state[lane] = (rlc(claims, lambda) * 2^shift, 1), and from the n_y coordinates of the layer's
 * out-of-domain point y_dev: inv_eq0_out[r] = 1 / prod_{j <= r} (1 - y_j) for every round r (prefix products, one inversion step)
 * and scalars_out = alpha | lambda | 1 - y_0 (12 words; the last 4 only for n_y > 0: the v of the layer's eq table).
 * TSTWO_GKR_STATUS_DEGENERATE is set where the host raises (a y_j in {0, 1, 1/2, 1/3}).  1 <= n_lanes <= 64, n_y <= 28. */
int tstwo_gkr_layer_begin(uint32_t *chan, const tstwo_gkr_lane *lanes_dev, uint32_t n_lanes, const uint32_t *claims, uint32_t *output_claims,
                          uint32_t *state, uint32_t *scalars_out, const uint32_t *y_dev, uint32_t n_y, uint32_t *inv_eq0_out,
                          uint32_t *status);
/* The bottom of a layer (gkr_prover.ts:540-575) by one wave: every lane's mask read from src and written to masks_out (16 words a
 * lane: column 0 at 0 and 1, column 1 at 0 and 1; zero where the kind has one column), mix_felts of each mask in lane order
 * (mask.columns() flattened), the draw of the challenge (challenge_out, 4 words: appended to the next out-of-domain point), and
 * claims[inst] = the mask's columns reduced at the challenge (reduceAtPoint; 8 words an instance). */
int tstwo_gkr_layer_end(uint32_t *chan, const tstwo_gkr_lane *lanes_dev, uint32_t n_lanes, uint32_t *masks_out, uint32_t *claims,
                        uint32_t *challenge_out);
/* prove_batch (gkr_prover.ts:440-580) in ONE call: the layers are generated, every layer runs begin / eq table / rounds / last
 * folds / end on the device, and one read-back at the end fills `block` (host).  Synchronous.  chan = the Blake2s channel's 10
 * words (host; the Rust draw semantics).  instances: 1 to 64; num / den as for the `kind` arguments above (4-byte aligned, never
 * written).  The schedule and the block's layout come from csrc/gkr_plan.h (n = instances, n_layers = max log_n; word offsets):
 *   0    channel state after the proof (10 words)          16   status word
 *   32 + 16 n   claims to verify, 8 words per instance     32 + 24 n   output claims, 8 words per instance (one value for a
 *   32 + 32 n + 4 n_layers (n_layers & 1)   the final out-of-domain point (4 n_layers words)       grand product: words 0..3)
 *   then per layer L = 0 .. n_layers - 1, from 32 + 32 n + 12 n_layers on: L round polynomials of 20 words (the round_poly_out
 *   of tstwo_gkr_round_finish), then 16 words per active instance (log_n >= n_layers - L, in instance order): its mask.
 * Everything else in the block is working state.  tstwo_gkr_prove_batch_words gives the block's size in words.
 * Refused with TSTWO_ERR_BAD_ARG before anything is enqueued: no or more than 64 instances, log_n = 0 or > 28, a 1-variable
 * LogUpMultiplicities instance (it has no mask), null or misaligned pointers, a block that is too small, a call during graph
 * capture.  A set status bit fails with TSTWO_ERR_BAD_ARG "sum-check: degenerate eq point" after the read-back. */
typedef struct {
    uint32_t kind, log_n;
    const uint32_t *num[4];
    const uint32_t *den[4];
} tstwo_gkr_instance;
int tstwo_gkr_prove_batch_words(const tstwo_gkr_instance *instances, size_t n_instances, size_t *block_words);
int tstwo_gkr_prove_batch(const uint32_t chan[10], const tstwo_gkr_instance *instances, size_t n_instances, uint32_t *block,
                          size_t block_words);

/* ---------------------------------------------------------------- AIR (constraint evaluation, composition polynomial)
 * Rust stwo constraint_framework/component.rs (the reference's constraint_framework/index.ts, air/accumulator.ts,
 * examples/fibonacci.ts).  Constraints read only their own row (mask offset 0).  Kinds for the `kind` argument: */
#define TSTWO_AIR_WIDE_FIB 0               /* N >= 3 columns: c_i = x_{i+2} - (x_i^2 + x_{i+1}^2), i < N - 2 (WideFibonacciEval<N>) */
#define TSTWO_AIR_MUL_ADD 1                /* 3 columns: c_0 = x_0 x_1 + x_0 - x_2 (TestEval of the Rust tutorial's example 05) */
/* generateTrace (examples/fibonacci.ts; Rust examples/wide_fibonacci generate_trace): cols[0] = a, cols[1] = b,
 * cols[k] = cols[k-2]^2 + cols[k-1]^2 for k < n_cols; every column 2^log_n words (device), n_cols >= 2.  Column tables beyond
 * 64 pointers are refused during graph capture. */
int tstwo_air_wide_fib_trace(const uint32_t *a, const uint32_t *b, uint32_t log_n, uint32_t *const *cols, size_t n_cols);
/* FrameworkComponent::evaluate_constraint_quotients_on_domain (constraint_framework/component.rs, CPU/SIMD loop): cols = the
 * component's trace on CanonicCoset(trace_log_size + log_expand).circle_domain(), bit-reversed order (device).  For every row r:
 *   accum[r] += (sum_i coeffs_i c_i(r)) * denom_inv[r >> trace_log_size]
 * coeffs: n_constraints QM31 values (4 host words each, n_constraints <= 128); denom_inv: 2^log_expand M31 host words
 * (log_expand <= 4), the bit-reversed 1 / coset_vanishing(trace coset, eval_domain.at(j)); accum: SecureColumnByCoords of
 * 2^(trace_log_size + log_expand) values, added to (not overwritten).  Column tables beyond 64 pointers are refused during graph
 * capture. */
int tstwo_air_constraint_quotients(uint32_t kind, const uint32_t *const *cols, size_t n_cols, uint32_t trace_log_size,
                                   uint32_t log_expand, const uint32_t *coeffs, size_t n_constraints, const uint32_t *denom_inv,
                                   uint32_t *const accum[4]);
/* User-defined constraints as a straight-line program (tstwo_amd/constraint_framework.py compiles a FrameworkEval into it): the
 * contract of tstwo_air_constraint_quotients with e_k(r) = the value of the k-th ACC instruction at row r, and loads at row offsets.
 *   cols: n_cols device columns on CanonicCoset(trace_log_size + log_expand).circle_domain(), bit-reversed order (main-trace
 *   columns, then preprocessed ones: the program names them by position);  1 <= log_expand <= 4 (the neighbour index needs
 *   eval > trace);  coeffs: n_constraints QM31 values (4 host words each), coefficient k goes with the k-th ACC;  denom_inv, accum:
 *   as for tstwo_air_constraint_quotients.
 * Program: program_len instructions of two host words, w0 = op | dst << 8 | x << 16, w1:
 *   TSTWO_AIR_OP_LOAD   r[dst] = cols[x][offset_bit_reversed_circle_domain_index(r, trace_log, trace_log + log_expand, (int32_t)w1)]
 *                       (the row (int32_t)w1 trace steps away; |w1| <= TSTWO_AIR_PROGRAM_MAX_OFFSET, x < n_cols)
 *   TSTWO_AIR_OP_CONST  r[dst] = w1 (an M31 value < 2^31 - 1)
 *   TSTWO_AIR_OP_ADD / _SUB / _MUL   r[dst] = r[x] (+ | - | *) r[w1]
 *   TSTWO_AIR_OP_SQR    r[dst] = r[x]^2            TSTWO_AIR_OP_NEG   r[dst] = -r[x]          (w1 ignored)
 *   TSTWO_AIR_OP_ACC    constraint k (k counts ACCs from 0) = r[x]; dst, w1 ignored.  There are exactly n_constraints ACCs.
 * Every register read must have been written by an earlier instruction; registers are < TSTWO_AIR_PROGRAM_MAX_REGS.  The
 * registers live in LDS (n_regs KiB per 64-lane workgroup, n_regs = the highest register written + 1).  Every limit is checked
 * (TSTWO_ERR_BAD_ARG, text in tstwo_last_error).  The program and coefficients are uploaded through the small-upload ring:
 * refused during graph capture.  Asynchronous. */
#define TSTWO_AIR_OP_LOAD 0
#define TSTWO_AIR_OP_CONST 1
#define TSTWO_AIR_OP_ADD 2
#define TSTWO_AIR_OP_SUB 3
#define TSTWO_AIR_OP_MUL 4
#define TSTWO_AIR_OP_SQR 5
#define TSTWO_AIR_OP_NEG 6
#define TSTWO_AIR_OP_ACC 7
#define TSTWO_AIR_PROGRAM_MAX_INSTR 1536
#define TSTWO_AIR_PROGRAM_MAX_REGS 32
#define TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS 256
#define TSTWO_AIR_PROGRAM_MAX_COLS 4096
#define TSTWO_AIR_PROGRAM_MAX_OFFSET 64
int tstwo_air_eval_program(const uint32_t *const *cols, size_t n_cols, uint32_t trace_log_size, uint32_t log_expand,
                           const uint32_t *program, size_t program_len, const uint32_t *coeffs, size_t n_constraints,
                           const uint32_t *denom_inv, uint32_t *const accum[4]);
/* The same programs compiled to native kernels at run time, opt-in: tstwo_air_eval_compiled computes bit for bit what
 * tstwo_air_eval_program computes for the program the kernel was compiled from.
 * tstwo_air_program_compile: validates the program (the checks and texts of tstwo_air_eval_program), writes it as HIP source
 *   (straight-line code on local variables: no LDS register file, column and coefficient indices are constants), compiles that
 *   with hipRTC for the architecture of the current device and loads the code object.  *kernel_id names the kernel: an id into
 *   a table of the library, handed out once per process.  trace_log_size and log_expand are not part of a kernel: one kernel
 *   serves every domain size.  hipRTC is loaded at the first call (TSTWO_ERR_HIP "hipRTC is not available" without it); a
 *   compile failure is TSTWO_ERR_HIP with the compiler's log in tstwo_last_error.  Synchronous (seconds for programs of
 *   hundreds of instructions); refused during graph capture.
 * tstwo_air_eval_compiled: the arguments, limits and error texts of tstwo_air_eval_program without the program; n_cols and
 *   n_constraints must be those the kernel was compiled for.  An id that is unknown, destroyed or from before tstwo_shutdown is
 *   TSTWO_ERR_BAD_ARG "unknown air kernel".  The coefficients are uploaded through the small-upload ring: refused during graph
 *   capture.  Asynchronous.
 * tstwo_air_kernel_info: info[0..2] = VGPRs, SGPRs and private-segment bytes per lane of the kernel for 16-byte aligned columns
 *   (4 rows per lane), info[3..5] the same for the one-row kernel, info[6] the size of the code object in bytes.
 * tstwo_air_program_destroy: unloads one kernel (synchronises the stream first; refused during graph capture).  tstwo_shutdown
 *   unloads every kernel still alive. */
#define TSTWO_AIR_KERNEL_INFO_WORDS 7
int tstwo_air_program_compile(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_constraints, uint64_t *kernel_id);
int tstwo_air_eval_compiled(uint64_t kernel_id, const uint32_t *const *cols, size_t n_cols, uint32_t trace_log_size,
                            uint32_t log_expand, const uint32_t *coeffs, size_t n_constraints, const uint32_t *denom_inv,
                            uint32_t *const accum[4]);
int tstwo_air_kernel_info(uint64_t kernel_id, uint32_t info[TSTWO_AIR_KERNEL_INFO_WORDS]);
int tstwo_air_program_destroy(uint64_t kernel_id);
/* The same programs evaluated on the trace domain itself into output columns (the numerators and denominator terms of a LogUp
 * interaction trace derived from `evaluate`: tstwo_amd/logup.py derive_interaction_trace).
 *   cols: n_cols device columns of 2^log_size M31 words on CanonicCoset(log_size).circle_domain(), bit-reversed order (the
 *   committed trace: main columns, then preprocessed ones, named by position);  out: n_out device columns of the same length,
 *   each written with canonical M31 values;  1 <= log_size <= 28;  1 <= n_out <= TSTWO_AIR_COLUMNS_MAX_OUT.
 * Program: the encoding and limits of tstwo_air_eval_program, with
 *   TSTWO_AIR_OP_STORE  out[w1][r] = r[x]; dst ignored; writes no register.  Every output index < n_out is stored exactly once.
 *   TSTWO_AIR_OP_ACC is a bad opcode here (as TSTWO_AIR_OP_STORE is in tstwo_air_eval_program).
 *   TSTWO_AIR_OP_LOAD at offset o reads the row whose point is o steps of CanonicCoset(log_size) away: in coset order, row
 *   (k + o) mod 2^log_size (offset_bit_reversed_circle_domain_index with eval_log == trace_log).
 * An `out` pointer equal to a `cols` pointer (or to another `out` pointer) is refused: loads at offsets read rows that other
 * lanes store.  Every limit is checked (TSTWO_ERR_BAD_ARG, text in tstwo_last_error, prefix "air columns: ").  The program is
 * uploaded through the small-upload ring: refused during graph capture.  Asynchronous. */
#define TSTWO_AIR_OP_STORE 8
#define TSTWO_AIR_COLUMNS_MAX_OUT 64
int tstwo_air_eval_columns(const uint32_t *const *cols, size_t n_cols, uint32_t log_size, const uint32_t *program,
                           size_t program_len, uint32_t *const *out, size_t n_out);
/* The column programs compiled to native kernels at run time, opt-in: tstwo_air_eval_columns_compiled writes bit for bit what
 * tstwo_air_eval_columns writes for the program the kernel was compiled from.
 * tstwo_air_columns_compile: validates the program (the checks and texts of tstwo_air_eval_columns; TSTWO_AIR_OP_ACC is a bad
 *   opcode, as TSTWO_AIR_OP_STORE is for tstwo_air_program_compile), writes it as HIP source (every STORE is one 16-byte store per
 *   lane, or one word for unaligned columns), compiles it with hipRTC and loads it, as tstwo_air_program_compile does.
 *   *kernel_id comes from the same table and the same counter; log_size is not part of a kernel.  Synchronous; refused during
 *   graph capture; TSTWO_ERR_HIP "hipRTC is not available" without hipRTC.
 * tstwo_air_eval_columns_compiled: the arguments, limits and error texts of tstwo_air_eval_columns without the program; n_cols
 *   and n_out must be those the kernel was compiled for.  An id that is unknown, destroyed or from before tstwo_shutdown is
 *   TSTWO_ERR_BAD_ARG "unknown air kernel"; the id of a constraint kernel is TSTWO_ERR_BAD_ARG "air columns: the kernel was
 *   compiled from a constraint program" (and the id of a columns kernel given to tstwo_air_eval_compiled "air program: the
 *   kernel was compiled from a columns program").  Nothing is uploaded: with at most 64 input columns the call may be recorded
 *   during graph capture (more than 64 go through a table in device memory, which is refused there).  Asynchronous.
 * tstwo_air_kernel_info and tstwo_air_program_destroy serve kernels of both kinds. */
int tstwo_air_columns_compile(const uint32_t *program, size_t program_len, size_t n_cols, size_t n_out, uint64_t *kernel_id);
int tstwo_air_eval_columns_compiled(uint64_t kernel_id, const uint32_t *const *cols, size_t n_cols, uint32_t log_size,
                                    uint32_t *const *out, size_t n_out);
/* Which constraint fails on which trace row (Rust stwo assert_constraints_on_trace): the same programs on the trace domain, each
 * constraint ending in a reduction instead of a store.  A trace satisfies the AIR exactly when every constraint is zero on every
 * row of CanonicCoset(log_size).
 *   cols, n_cols, log_size: those of tstwo_air_eval_columns (main columns, then preprocessed, then interaction ones, named by
 *   position); the columns are never written.  1 <= log_size <= 28.
 * Program: the encoding, limits and error texts of tstwo_air_eval_program, TSTWO_AIR_OP_ACC the terminal, TSTWO_AIR_OP_LOAD at
 *   offset o reading what tstwo_air_eval_columns reads.  Here the ACC's w1 is the index of the constraint the ACC belongs to: the
 *   indices start at 0, never decrease, rise by at most 1 from one ACC to the next and end at n_constraints - 1 ("constraint
 *   index decreases", "... skips", "... out of range", "first constraint index is not 0", "last constraint index is not
 *   n_constraints - 1").  So a QM31 constraint lowered into four base-field ACCs is reported as one.
 *   1 <= n_constraints <= TSTWO_AIR_PROGRAM_MAX_CONSTRAINTS; there may be more ACCs.
 * report: 2 * n_constraints device words, 16-byte aligned, all overwritten on the stream: word 2c = the number of rows on which
 *   constraint c is non-zero as a field element (a row counts once, however many of its ACCs are non-zero there), word 2c + 1
 *   = the smallest such row in coset order (the k for which a load at offset o reads row k + o: the row of the trace as it was
 *   written), or 0xffffffff when there is none.  Both are order-independent integers: the report is exact whatever the schedule.
 * Every limit is checked before anything is enqueued (TSTWO_ERR_BAD_ARG, prefix "air check: ").  The program is uploaded through
 * the small-upload ring: refused during graph capture.  Asynchronous. */
int tstwo_air_check_constraints(const uint32_t *const *cols, size_t n_cols, uint32_t log_size, const uint32_t *program,
                                size_t program_len, size_t n_constraints, uint32_t *report);

/* ---------------------------------------------------------------- LogUp interaction trace
 * Rust stwo constraint_framework/logup.rs (LogupTraceGenerator, LogupColGenerator); tstwo_amd/logup.py drives it.
 * One fraction of an interaction column: numerator num[r] (a device column of M31 values) or, when num is NULL, num_const for
 * every row; denominator sum_t coeffs[4t .. 4t + 4) * cols[t][r] + constant (QM31 coefficients and constant, M31 columns).
 * Limits (TSTWO_ERR_BAD_ARG, text in tstwo_last_error): 1 .. TSTWO_LOGUP_MAX_FRACS fractions per column ("1 to 8 fractions per
 * column"), 1 .. TSTWO_LOGUP_MAX_TERMS terms per denominator ("1 to 16 terms per fraction"), log_size <= TSTWO_LOGUP_MAX_LOG,
 * every host word < 2^31 - 1 ("... out of range"), no null pointer.  Every column holds 2^log_size words. */
typedef struct {
    const uint32_t *num;
    uint32_t num_const;
    uint32_t n_terms;
    const uint32_t *const *cols;
    const uint32_t *coeffs;
    uint32_t constant[4];
} tstwo_logup_frac;
#define TSTWO_LOGUP_MAX_FRACS 8
#define TSTWO_LOGUP_MAX_TERMS 16
#define TSTWO_LOGUP_MAX_LOG 28
/* out[r] = (prev ? prev[r] : 0) + sum_b num_b[r] / den_b[r] for r < 2^log_size, one launch (out may be prev).  A zero denominator
 * raises the sticky zero flag (tstwo_check_zero_flag then fails with "0 has no inverse").  The descriptors are uploaded through
 * the small-upload ring: refused during graph capture.  Asynchronous. */
int tstwo_logup_column(const tstwo_logup_frac *fracs, size_t n_fracs, const uint32_t *const prev[4], uint32_t log_size,
                       uint32_t *const out[4]);
/* The last interaction column, in place: claimed = sum_r col[r]; then, in coset order (mask offset -1 is the previous coset row),
 * col[pos(k)] = sum_{k' <= k} (col[pos(k')] - claimed / 2^log_size), so the last coset row holds 0.  claimed_sum (host) receives
 * the 4 words of claimed.  1 <= log_size <= 28.  Synchronous; refused during graph capture. */
int tstwo_logup_finalize_last(uint32_t *const col[4], uint32_t log_size, uint32_t claimed_sum[4]);

/* ---------------------------------------------------------------- mle_eval component (GKR input claims inside the STARK)
 * The device steps of the AIR component that proves sum_p eq(p, r) L[p] = v for a linear form L over committed columns
 * (tstwo_amd/mle_eval.py; the reference has no such component, Rust stwo has one as an example).  Its interaction
 * trace is E = tstwo_gkr_gen_eq_evals(r, 1), then tstwo_mle_eval_terms, then tstwo_logup_finalize_last.
 * The preprocessed selector columns of log size n = log_size, 2n + 2 columns of 2^n words with values 0 / 1 that depend on n only.
 * With d = the bit reversal of the storage position p over n bits, h = 2^(n-1), d' = d mod h and t(p) = the number of trailing
 * one bits of d' (n - 1 when d' = h - 1):
 *   out[t]      = G_t[p] = [d <  h and t(p) = t]   t < n
 *   out[n + t]  = K_t[p] = [d >= h and t(p) = t]   t < n
 *   out[2n]     = F0[p]  = [d = 0]
 *   out[2n + 1] = F1[p]  = [d = h]
 * out: a host array of 2n + 2 device columns; every word of every column is written exactly once.  2 <= log_size <= 28
 * ("mle eval selectors: log_size must be 2 to 28"), no null pointer, no two columns overlapping.  Asynchronous. */
int tstwo_mle_eval_selectors(uint32_t log_size, uint32_t *const *out);
/* out[p] = eq[p] * (constant + sum_k coeffs[4k .. 4k+4) * cols[k][p]) for p < 2^log_size: a secure column times a linear form
 * with QM31 coefficients and constant over M31 columns (the form of a tstwo_logup_frac denominator).  Descriptor rules and
 * limits as there (TSTWO_ERR_BAD_ARG, text "mle eval terms: ..."): 1 <= n_terms <= TSTWO_LOGUP_MAX_TERMS ("1 to 16 terms"),
 * log_size <= 28, every host word < 2^31 - 1 ("... out of range"), no null pointer, an output column that overlaps a column of
 * the form is refused ("an output column is also an input").  out may be eq itself, column for column (out[j] == eq[j]); any
 * other overlap of out with eq is refused ("out may alias eq only column for column").  Nothing is inverted: the zero flag is
 * not touched.  Everything travels as kernel arguments: the call may be captured into a graph.  Asynchronous. */
int tstwo_mle_eval_terms(const uint32_t *const eq[4], const uint32_t *const *cols, const uint32_t *coeffs, size_t n_terms,
                         const uint32_t constant[4], uint32_t log_size, uint32_t *const out[4]);

/* ---------------------------------------------------------------- Lookup multiplicities
 * The multiplicity column of a lookup table, counted on the device: a histogram of M31 columns into a column of 2^log_range
 * words (tstwo_amd/logup.py lookup_multiplicities; the host version is constraint_framework.range_check_multiplicities). */
#define TSTWO_LOOKUP_ORDER_NATURAL 0   /* bin k at word k (an MLE / GKR LogUpMultiplicities numerator column) */
#define TSTWO_LOOKUP_ORDER_COSET   1   /* bin k at the storage position of coset row k: coset_pos(k) of coset_order.cuh,
                                          the order of range_check_table_column / range_check_multiplicities */
#define TSTWO_LOOKUP_MAX_COLS 64
#define TSTWO_LOOKUP_MAX_LOG  28
/* out[place(k)] = the number of words equal to k over all columns, k < 2^log_range.
 *   cols: a host array of n_cols device columns, column c of lens[c] words (lens: host; any length, 0 and lengths that are no
 *   power of two or multiple of 4 included; any 4-byte alignment);  out: 2^log_range device words, overwritten completely (the
 *   entry zeroes it itself).
 * A word >= 2^log_range is counted in no bin and never used as an index.  n_rejected (a device word, or NULL) receives the
 * number of such words, 0 when there are none; with NULL they are skipped silently.
 * Limits (TSTWO_ERR_BAD_ARG, text "lookup: ..." in tstwo_last_error): 1 <= log_range <= TSTWO_LOOKUP_MAX_LOG ("log_range must
 * be 1 to 28"), 1 <= n_cols <= TSTWO_LOOKUP_MAX_COLS ("1 to 64 columns"), sum(lens) <= 2^31 - 2 so that every count is a
 * canonical M31 value ("more than 2^31 - 2 values"), order 0 or 1 ("order must be 0 (natural) or 1 (coset)"), no null pointer
 * except n_rejected ("null ..."), out overlaps no column ("out is one of the columns") and does not hold n_rejected.
 * Counts are integer atomics: the result is the same bit for bit on every run.  The column table is uploaded through the
 * small-upload ring: refused during graph capture.  Asynchronous. */
int tstwo_lookup_multiplicities(const uint32_t *const *cols, const size_t *lens, size_t n_cols, uint32_t log_range, uint32_t order,
                                uint32_t *out, uint32_t *n_rejected);
/* The same column for keys joined from several columns and rows that carry a weight (tstwo_amd/logup.py
 * lookup_multiplicities_keyed): a table of tuples (a, b) -> bin a + 2^bits_a b, looked up by a component whose padded rows are
 * switched off by an `enabler` column.  One group is one set of rows: n_limbs limb columns and, optionally, a weight column. */
#define TSTWO_LOOKUP_MAX_LIMBS 4
#define TSTWO_LOOKUP_MAX_GROUPS 64
typedef struct {
    const uint32_t *limbs[TSTWO_LOOKUP_MAX_LIMBS]; /* device columns of len words; limbs[0] = least significant; unused entries NULL */
    uint32_t bits[TSTWO_LOOKUP_MAX_LIMBS];         /* limb j of a row must be < 2^bits[j]; 1 <= bits[j]; sum over the n_limbs used = log_range */
    uint32_t n_limbs;                              /* 1 .. TSTWO_LOOKUP_MAX_LIMBS */
    const uint32_t *weight;                        /* device column of len words, or NULL: every row weighs 1 */
    size_t len;                                    /* rows: any length, 0 included; any 4-byte alignment of every column */
} tstwo_lookup_group;
/* groups: a host array of n_groups descriptors.  out: 2^log_range device words, overwritten completely.
 * Key.  The key of row r of group g is sum_j limbs[j][r] << (bits[0] + ... + bits[j-1]).
 * Result.  out[place(k)] = (sum of weight[r] over all groups and rows with key k) mod P, canonical in [0, P); place is
 *   TSTWO_LOOKUP_ORDER_* as above.
 * Weights.  Weight words are added as the unsigned integers they are (M31 values, so P - 1 is -1).  A word >= P is not rejected:
 *   it is reduced with the sum.
 * Accumulators are exact: sum(len) <= 2^31 - 2 rows of weight < 2^32 stay below 2^63, and a call with any weight column
 *   accumulates in 64-bit integers (8 bytes per bin from the library's allocator for the duration of the call, reduced mod P by a
 *   second kernel; a table too large for that block fails with TSTWO_ERR_HIP and the allocator's text, before anything is zeroed
 *   or launched).  A call whose groups all have weight NULL counts in 32-bit words, which the row limit keeps canonical.
 * Zero weight.  A row whose weight is 0 is skipped before anything else: its limbs are not range-checked and it is counted
 *   nowhere, n_rejected included.  This is what gating means: padding may hold anything.
 * Rejection.  A row with non-zero weight is rejected when any limb is >= 2^bits[j]: it is counted in no bin and never forms an
 *   index.  Rejected rows add 1 each, per row and not per limb, to *n_rejected (a device word, or NULL).
 * Limits (TSTWO_ERR_BAD_ARG, text "lookup: ..." in tstwo_last_error, before anything is launched or zeroed):
 *   1 <= n_groups <= TSTWO_LOOKUP_MAX_GROUPS ("1 to 64 groups"), 1 <= n_limbs <= TSTWO_LOOKUP_MAX_LIMBS ("1 to 4 limbs per
 *   group"), every bits[j] >= 1 ("every limb needs at least 1 bit"), every group's sum of bits = log_range ("the bits of every
 *   group must add up to log_range"), 1 <= log_range <= TSTWO_LOOKUP_MAX_LOG ("log_range must be 1 to 28"), sum(len) <= 2^31 - 2
 *   ("more than 2^31 - 2 rows"), order 0 or 1 ("order must be 0 (natural) or 1 (coset)"), no null pointer except weight and
 *   n_rejected ("null ..."), out overlaps no limb or weight column ("out overlaps a limb or weight column") and does not
 *   contain n_rejected ("n_rejected lies inside out").
 * Integer atomics only: the result is the same bit for bit on every run.  The descriptor table is uploaded through the
 * small-upload ring: refused during graph capture.  Asynchronous, with one exception: a call with a weight column returns its
 * accumulator block through tstwo_free, which in TSTWO_ALLOC_DIRECT mode synchronises the stream before hipFree (pool and async
 * modes release in stream order and do not wait). */
int tstwo_lookup_multiplicities_keyed(const tstwo_lookup_group *groups, size_t n_groups, uint32_t log_range, uint32_t order,
                                      uint32_t *out, uint32_t *n_rejected);
/* out[coset_pos(k)] = k for k < 2^log_size: the preprocessed column of a range-check table (range_check_table_column).
 * 1 <= log_size <= TSTWO_LOOKUP_MAX_LOG ("lookup: log_size must be 1 to 28").  Asynchronous; refused during graph capture. */
int tstwo_coset_iota(uint32_t *out, uint32_t log_size);

#ifdef __cplusplus
}
#endif
#endif

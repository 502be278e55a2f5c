// air_native.h — between air.hip (argument checks, launch shape) and air_native.hip (hipRTC, the table of compiled kernels).
#pragma once
#include "common.h"

namespace tstwo {

// The second argument of a generated kernel, behind the ColPtrs table: field for field the NativeArgs of
// csrc/air_native_prelude.inc, the text the kernels are compiled from.
struct NativeArgs {
    const u32 *coeff;                        // device: 4 coefficient words per constraint
    u32 denom_inv[16];
    Soa4 acc;
    u32 n_rows, trace_log, eval_log, log_expand, n_denoms, stride;
};
static_assert(sizeof(NativeArgs) == 128 && sizeof(ColPtrs) == 520, "the layouts the prelude text states");

// What kernel `id` was compiled for; TSTWO_ERR_BAD_ARG "unknown air kernel" for an id that is not in the table.
__attribute__((visibility("hidden"))) int air_native_shape(uint64_t id, u32 &n_cols, u32 &n_constraints);
// Launches kernel `id` (W = 4 rows per lane when vec, else W = 1) with `grid` workgroups of kAirNativeThreads lanes on the
// library's stream.
__attribute__((visibility("hidden"))) int air_native_launch(uint64_t id, bool vec, unsigned grid, ColPtrs &cols, NativeArgs &args);

}  // namespace tstwo

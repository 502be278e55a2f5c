// air_native.h — between air.hip (argument checks, launch shape) and air_native.hip (hipRTC, the table of compiled kernels).
#pragma once
#include <cstddef>

#include "air_codegen.h"
#include "air_plan.h"
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

// The third argument of a generated columns kernel, behind the input and the output ColPtrs tables: field for field the
// ColumnsArgs of csrc/air_native_columns_prelude.inc.
struct ColumnsArgs { u32 n_rows, log, stride; };
static_assert(sizeof(ColumnsArgs) == 12 && offsetof(ColumnsArgs, log) == 4 && offsetof(ColumnsArgs, stride) == 8,
              "the layout the columns prelude text states");

// What a table entry was compiled from: a constraint (ACC) program or a columns (STORE) program.
enum AirKernelKind : u32 { kAirKernelConstraints = 0, kAirKernelColumns = 1 };

// What kernel `id` was compiled for (n_terminal: its constraints, or its outputs); TSTWO_ERR_BAD_ARG "unknown air kernel" for an
// id that is not in the table.
__attribute__((visibility("hidden"))) int air_native_shape(uint64_t id, AirKernelKind &kind, u32 &n_cols, u32 &n_terminal);
// Launches kernel `id` on the library's stream as the plan says: its W = 4 or its W = 1 kernel, plan.grid workgroups of
// kAirNativeThreads lanes, plan.stride into args.stride.
static_assert(kAirNativeThreads == (int)kAirWideThreads, "the plan counts the compiled kernels' workgroups at kAirNativeThreads lanes");
__attribute__((visibility("hidden"))) int air_native_launch(uint64_t id, const AirPlan &plan, ColPtrs &cols, NativeArgs &args);

// The same for a columns kernel: (cols, out, args).
__attribute__((visibility("hidden"))) int air_native_launch_columns(uint64_t id, const AirPlan &plan, ColPtrs &cols, ColPtrs &out, ColumnsArgs &args);

}  // namespace tstwo

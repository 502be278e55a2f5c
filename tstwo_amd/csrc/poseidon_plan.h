// poseidon_plan.h — which kernel hashes a Poseidon252 tree layer inside tstwo_fri_commit_layers_poseidon252 (host only: no HIP, no
// context).  tests/test_cpu_fri_plan_poseidon.py compiles this header and holds the GPU tests' shapes to both sides of the constant.
#pragma once
#include <cstdint>

namespace tstwo {

// Layers of at most 2^kP252CoopMaxLog nodes take the 8-lanes-per-node kernel (k_p252c_layer), larger ones the lane-per-node
// kernel (k_p252_layer).  Measured (profiles/poseidon_coop.jsonl): the largest log at which the cooperative kernel is
// faster by more than the two spreads, for children-only nodes and for 4-column leaves alike — up to 2^14 nodes (2^17 lanes) the
// cooperative layer still costs its two or one permutations of latency, 0.35 / 0.18 ms against 0.58 / 0.30 ms; at 2^15 it has
// filled the device and loses.  -1 would say "never".
constexpr int kP252CoopMaxLog = 14;

inline bool p252_layer_is_coop(uint32_t log_size) { return (int)log_size <= kP252CoopMaxLog; }

}  // namespace tstwo

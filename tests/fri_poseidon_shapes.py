"""The shapes of tests/test_gpu_fri_poseidon_commit.py: (circle log sizes, log_last_layer_degree_bound), all with log_blowup_factor 1,
so a circle evaluation of log size c has degree bound c - 1 and the last layer has 2^(bound + 1) rows.  Kept apart from the GPU file so
that tests/test_cpu_fri_plan_poseidon.py can hold them to both sides of kP252CoopMaxLog without a device."""

LOG_BLOWUP = 1
SHAPES = [
    ([5], 0),              # last layer of 2 rows
    ([5], 2),              # last layer of 8 rows
    ([5], 3),              # the last layer is the first line layer: no inner layer
    ([10, 8, 6], 1),       # columns joining on the way down
    ([15], 2),             # one column whose upper tree layers lie above kP252CoopMaxLog
]
MODEL_SHAPES = [s for s in SHAPES if s[0] == [5]]          # roots also against the integer model


def last_log(bound):
    return bound + LOG_BLOWUP


def tree_layer_logs(col_logs, bound):
    """log sizes of every tree layer a commit of the shape hashes: the first-layer tree and one tree per inner line layer"""
    logs = list(range(col_logs[0], -1, -1))
    for lg in range(col_logs[0] - 1, last_log(bound), -1):
        logs += list(range(lg, -1, -1))
    return logs

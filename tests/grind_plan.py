"""The batch schedule of the two proof-of-work searches (csrc/grind_plan.h), restated: which (first nonce, count) launches a search
from `start` issues until it has covered a given nonce, where the batch edges lie, and which nonces the idle lanes of a short last
workgroup would test if nothing stopped them.  tests/test_cpu_grind.py compares this with the header, compiled on its own."""
NONE = 2**64 - 1          # the "none found" value: never tested, never returned
LANES = 256               # lanes per workgroup of both kernels
BLAKE2S, P252 = "blake2s", "p252"
KINDS = {BLAKE2S: 0, P252: 1}          # the header's GrindKind


def batch_sizes(kind):
    """The batch sizes in launch order, unclamped, without end (the last one repeats)."""
    if kind == BLAKE2S:
        for _ in range(4):
            yield 1 << 20
        while True:
            yield 1 << 26
    else:
        for lg in (16, 18, 20):
            yield 1 << lg
        while True:
            yield 1 << 22


def batches(kind, start, n_max):
    """[(base, count)] of the first n_max launches of a search from `start` that finds nothing; it ends early, behind a last short
    batch, when the next launch would begin at NONE ("nonce space exhausted")."""
    out, base = [], start
    for size in batch_sizes(kind):
        count = min(size, NONE - base)
        if count == 0 or len(out) == n_max:
            break
        out.append((base, count))
        base += count
    return out


def edges(kind, limit):
    """Offsets from `start`, up to `limit`, at which a new batch begins when nothing is clamped: a hit at offset e - 1 is on the last
    lane of a batch, one at offset e on lane 0 of the next."""
    out, off = [], 0
    for size in batch_sizes(kind):
        off += size
        if off > limit:
            return out
        out.append(off)


def first_grown_edge(kind):
    """The offset at which the first batch larger than the first one begins."""
    off, first = 0, None
    for size in batch_sizes(kind):
        first = first or size
        if size > first:
            return off
        off += size


def idle_lane_nonces(base, count):
    """What lanes count .. (the launch's last lane) would compute as base + lane in 64-bit arithmetic."""
    lanes = -(-count // LANES) * LANES
    return [(base + i) % 2**64 for i in range(count, lanes)]

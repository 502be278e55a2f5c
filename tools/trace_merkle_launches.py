#!/usr/bin/env python3
"""The launch sequence of the Merkle / decommit code over a fixed set of workloads, to compare two builds of the library
(TSTWO_HIP_LIB selects one) launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trace_merkle_launches.py     (a run of its own: no counters)
    python tools/trace_merkle_launches.py --list DIR > launches.txt       one line per launch, in start order: name, grid, workgroup
    python tools/trace_merkle_launches.py --diff A.txt B.txt              exit 1 unless the lists agree line by line; the only
                                                                          difference let through: k_merkle_inner in A (one tree's
                                                                          leftover layer) as k_merkle_inner_set with the same grid in B

Workloads: tstwo_merkle_commit of 32 columns at log 16 / 17 / 22 / 23 (17 and 23 have a single leftover layer above 2^16 nodes), of
4 columns at log 9 / 12 / 17 / 24, of columns at three sizes (one below 2^16 rows); tstwo_merkle_commit_many of 8 x 32 x 2^22 and of
three unequal trees; one FriProver.commit with the device channel at log 20; decommit, decommit_many and the FRI decommit."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launches(root):
    import csv, glob
    rows = []
    for f in glob.glob(f"{root}/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{name} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']} wg {r['Workgroup_Size_X']}x{r['Workgroup_Size_Y']}x{r['Workgroup_Size_Z']}")


def diff(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad = abs(len(la) - len(lb))
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y and x.replace("k_merkle_inner grid", "k_merkle_inner_set grid") != y:
            bad += 1
            print(f"line {i + 1}: {x}  |  {y}")
    print(f"{len(la)} / {len(lb)} launches, {bad} differ")
    return 1 if bad else 0


def run():
    import numpy as np
    import tstwo_amd as T
    from tstwo_amd import _lib as L
    from tstwo_amd.vcs import MerkleProver
    L.init(0)
    rng = np.random.default_rng(0)
    data = {}

    def cols(n_cols, log):               # columns of one size share their words: only the launches matter here
        if log not in data:
            data[log] = rng.integers(0, T.P, size=1 << log, dtype=np.uint32)
        return [T.HipColumn(data[log]) for _ in range(n_cols)]

    for log in (16, 17, 22, 23):
        MerkleProver.commit(cols(32, log))
    for log in (9, 12, 17, 24):
        MerkleProver.commit(cols(4, log))
    mixed = cols(32, 20) + cols(8, 18) + cols(4, 12)
    tree = MerkleProver.commit(mixed)
    wide = cols(32, 22)
    MerkleProver.commit_many([wide] * 8)
    uneven = [cols(32, 18), cols(16, 17), cols(4, 10)]
    trees = MerkleProver.commit_many(uneven)
    L.sync()
    # FriProver.commit with the device channel, log 20 (tools/trace_fri_commit.py)
    blow = 2
    domain = T.CanonicCoset(18 + blow).circleDomain()
    tw = T.precompute_twiddles(domain.halfCoset)
    polys = [T.HipCirclePoly(rng.integers(0, T.P, size=1 << 18, dtype=np.uint32)) for _ in range(4)]
    evs = T.evaluate_polynomials(polys, domain, tw)
    col = T.SecureEvaluation(domain, T.SecureColumnByCoords([e.values for e in evs]))
    ch = T.Blake2sChannel()
    fp = T.FriProver.commit(ch, T.FriConfig(2, blow, 20), [col], tw, device_channel=True)
    L.sync()
    queries = {20: [3, 77, 1 << 19], 18: [5, 6], 12: [0, 4095]}
    tree.decommit(queries, mixed)
    MerkleProver.decommit_many([(tree, queries, mixed)] + [(t, {18: [1, 2], 17: [9], 10: [1000]}, c) for t, c in zip(trees, uneven)])
    fp.decommit(ch)
    L.sync()
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        launches(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        run()

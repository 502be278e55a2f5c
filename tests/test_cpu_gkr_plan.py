"""The schedule of tstwo_gkr_prove_batch (no GPU): csrc/gkr_plan.h, compiled on its own with the address and undefined behaviour
sanitizers, against tests/gkr_plan.py; what the batches of the -m gpu file reach; and the resource usage of the kernels of
csrc/gkr_ops.hip and csrc/gkr_transcript.hip, compiled for gfx950 without a device."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import gkr_plan as GP
from tstwo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")


def _library_lines(tmp_path, batches):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gkr_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "gkr_plan_main.cpp"), "-o", exe])
    text = "".join(" ".join(f"{k}:{n}" for k, n in b) + "\n" for b in batches)
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.splitlines()
    assert len(got) == len(batches)
    return got


def _own(batch):
    try:
        return GP.render(GP.Plan(batch))
    except GP.PlanError as e:
        return f"error: {e}"


def test_gkr_plan_matches_the_library(tmp_path):
    """Both statements give the same layers, rounds, lanes, folds, pool and block offsets for every batch of 1 to 3 instances over
    the four kinds with 1 to 6 variables, for the batches of the -m gpu files, and the same reason for every refusal."""
    one = [(k, n) for k in GP.KINDS for n in range(1, 7)]
    batches = [list(b) for r in (1, 2, 3) for b in itertools.product(one, repeat=r)]
    batches += [GP.named_batch(name) for name in ("mixed", "64", "small")]
    refused = {"empty": [], "65": GP.named_batch("65"), "zero": [(GP.GENERIC, 3), (GP.GP, 0)], "29": [(GP.SINGLES, 29)],
               "mult1": [(GP.GP, 5), (GP.MULT, 1)], "kind": [(4, 3)]}
    got = _library_lines(tmp_path, batches + list(refused.values()) + [[(GP.GENERIC, 28)]])
    for b, line in zip(batches + list(refused.values()), got):
        assert line == _own(b), b
    assert got[len(batches):-1] == ["error: no instances", "error: prove_batch: 1 to 64 instances",
                                    "error: Some output claims were not set during proving (an input layer of 0 variables is an output layer)",
                                    "error: GKR layer too large", "error: LogUpMultiplicities should never reach tryIntoMask",
                                    "error: unknown GKR layer kind"]
    assert got[-1] == _own([(GP.GENERIC, 28)]) and not got[-1].startswith("error")
    # what any statement of the plan must satisfy
    for b in batches:
        try:
            p = GP.Plan(b)
        except GP.PlanError:
            continue
        assert p.pool_words == sum(c * sum(GP.col_words(k) for k in range(n)) for (_, n), c in zip(b, p.gen_cols))
        assert len(p.layers[-1]["active"]) == p.n and p.layers[0]["enter"] == p.layers[0]["active"]
        prev_end = p.inv_off + 4 * p.n_layers
        for L, lay in enumerate(p.layers):
            assert lay["poly_off"] == prev_end and lay["mask_off"] == prev_end + 20 * L
            prev_end = lay["mask_off"] + 16 * len(lay["active"])
            for i in lay["active"]:
                n_v, log_n = p.n_v(i, L), b[i][1]
                kinds = [p.fold_kind(i, L, f) for f in range(n_v)]
                # the caller's layers are never written: an input's first fold leaves it, and only then
                assert all((k != GP.IN_PLACE) == (f == 0 and n_v + 1 == log_n) for f, k in enumerate(kinds))
                assert (GP.NEW_BASE in kinds) == (b[i][0] == GP.MULT and n_v + 1 == log_n and n_v >= 1)
                # a new buffer is the instance's dead layer of log_n - 1 variables: it holds the folded half
                assert GP.col_words(log_n - 1) >= 1 << (log_n - 1)
        assert prev_end == p.block_words


def test_gpu_batches_reach_every_branch():
    """The batches tests/test_gpu_gkr_one_call.py proves reach every branch of the plan: an instance entering at the first, a
    middle and the last layer (beside continuing ones), a layer without rounds, folds in place and into a new buffer, base
    numerators, claims doubled 0, 1 and 12 times, 1 and 64 instances."""
    reached = set()
    for name, batch in GP.gpu_batches().items():
        reached |= GP.branches(GP.Plan(batch))
    assert reached == GP.ALL_BRANCHES, sorted(GP.ALL_BRANCHES ^ reached)
    assert {"enters at a middle layer", "enters at the last layer", "shift 12", "base numerators"} <= GP.branches(GP.Plan(GP.named_batch("mixed")))
    assert "64 instances" in GP.branches(GP.Plan(GP.named_batch("64"))) and "shift 1" in GP.branches(GP.Plan(GP.named_batch("small")))


# Every kernel that takes a protocol scalar by value or from device words, by a pattern of its mangled name: (VGPRs, waves per SIMD)
# of whichever of its two former twins (one per scalar source) was worse.  The one kernel that serves both sources is held to that.
MERGED_KERNELS = {
    "5k_sumILi0ELb0E": (56, 8), "5k_sumILi1ELb0E": (89, 5), "5k_sumILi2ELb0E": (73, 6), "5k_sumILi3ELb0E": (62, 8),
    "5k_sumILi0ELb1E": (57, 8), "5k_sumILi1ELb1E": (88, 5), "5k_sumILi2ELb1E": (88, 5), "5k_sumILi3ELb1E": (61, 8),
    "18k_gkr_round_finishE": (77, 6),
    "11k_eq_tablesE": (64, 8),      # its twins had 30 each; a latency-bound kernel of a few blocks, held to what 8 waves per SIMD allow
}
KERNEL_COUNTS = {"k_eq_tables": 1, "k_eq_expand": 2, "k_next_layer": 4, "k_fold": 4, "k_sum": 8, "k_gkr_round_finish": 1, "k_gkr_layer_begin": 1,
                 "k_gkr_layer_end": 1}


def test_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The GKR translation units compile for gfx950 without a device; there is ONE kernel per operation whether its scalars come by
    value or from device memory, none reports scratch, and each kernel that serves both sources has no more registers and no fewer
    waves per SIMD than the worse of the two kernels it replaced."""
    usage = {}
    for unit in ("gkr_ops", "gkr_transcript", "gkr_prove"):
        p = subprocess.run([B._hipcc(), *B.FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(CSRC, unit + ".hip"), "-o", str(tmp_path / (unit + ".o"))], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        kernel = None
        for line in p.stderr.splitlines():
            m = re.search(r"remark: \s*(.+?): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                kernel = usage.setdefault(m.group(2), {})
            elif kernel is not None:
                kernel[m.group(1)] = m.group(2)
    for name, count in KERNEL_COUNTS.items():
        found = sorted(k for k in usage if re.search(rf"\d{name}(?![a-z_])", k))
        assert len(found) == count, (name, found)
    assert len(usage) == sum(KERNEL_COUNTS.values()), sorted(usage)
    for k, u in sorted(usage.items()):
        print(k, "VGPRs", u["VGPRs"], "SGPRs", u["TotalSGPRs"], "occupancy", u["Occupancy [waves/SIMD]"], "scratch", u["ScratchSize [bytes/lane]"])
        assert u["ScratchSize [bytes/lane]"] == "0", (k, u)
    for pattern, (vgprs, waves) in MERGED_KERNELS.items():
        (k,) = [k for k in usage if pattern in k]
        assert int(usage[k]["VGPRs"]) <= vgprs and int(usage[k]["Occupancy [waves/SIMD]"]) >= waves, (k, usage[k], vgprs, waves)

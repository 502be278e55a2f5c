"""The launch plan of tstwo_mle_eval_at_point_* (no GPU): csrc/mle_eval_plan.h, compiled on its own, against
tests/mle_eval_plan.py over every size, batch, kind and alignment; and what the shapes of the -m gpu file reach."""
import os
import shutil
import subprocess

import pytest

import mle_eval_plan as MP


def _library_plans(tmp_path, inputs):
    """One line of mle_eval_plan_main per input (log_n, n_mles, is_secure, aligned)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "mle_eval_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"),
                           os.path.join(here, "mle_eval_plan_main.cpp"), "-o", exe])
    text = "".join(f"{lg} {n} {int(s)} {int(a)}\n" for lg, n, s, a in inputs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(inputs)
    return got


def _own(lg, n, secure, aligned):
    try:
        return MP.render(MP.plan(lg, n, secure, aligned))
    except MP.PlanError as e:
        return f"error: {e}"


def test_mle_eval_plan_matches_the_library(tmp_path):
    """Both statements give the same launches, chunk sizes and scratch for every (log_n <= 28, n_mles in {1, 2, 64, 65}, kind,
    aligned / not), and the same reason for the inputs without a plan."""
    inputs = [(lg, n, s, a) for lg in range(MP.MAX_LOG + 1) for n in (1, 2, 3, 4, 64, 65, 128) for s in (False, True) for a in (False, True)]
    rejected = [(29, 1, False, True), (5, 0, True, True), (5, MP.MAX_MLES + 1, False, True), (28, MP.MAX_MLES, True, False)]
    got = _library_plans(tmp_path, inputs + rejected)
    for args, line in zip(inputs + rejected, got):
        assert line == _own(*args), args
    assert got[-4:-1] == ["error: more than 28 variables", "error: no MLE given", "error: more than 32768 MLEs in one call"]
    assert not got[-1].startswith("error")
    for lg, n, s, a in inputs:
        p = MP.plan(lg, n, s, a)
        # what any statement of the plan must satisfy
        assert p.chunks << p.chunk_log == max(1 << lg, 1 << p.chunk_log)        # the chunks tile the MLE; a small MLE has one
        assert p.fast <= (a and lg >= p.chunk_log)                             # 16-byte loads never leave the MLE
        assert p.chunks <= 1 << 16 and p.blocks * MP.FOLD_BLOCK >= (p.chunks if p.passes == 2 else 0)
        assert (p.passes == 2) == (p.chunks > 1) and p.grid_y == n
        assert p.groups == 4 if s else p.groups in (1, 4)
        assert p.chunks << p.chunk_log <= 1 << 28                              # word offsets inside a column stay below 2^30


def test_gpu_shapes_reach_every_branch():
    """The coverage condition: the calls tests/test_gpu_mle_eval.py makes, none over 2^22 values, reach every pass-1 kernel on
    every load path it has, every way pass 2 can run, and the pointer table in device memory.  No shape of the plan exists only
    above 2^22 values: pass 2 is one workgroup per MLE whatever the size (csrc/mle_eval_plan.h)."""
    reached = set()
    for name, (lg, n, secure, offset) in MP.gpu_shapes().items():
        assert n << lg <= MP.MAX_GPU_VALUES, name
        reached |= MP.branches(lg, n, secure, offset == 0)
    want = MP.reachable_branches()
    assert want == {"base1:fast", "base1:small", "base1:unaligned", "base4:fast", "base4:unaligned", "secure:fast", "secure:small",
                    "secure:unaligned", "fold:none", "fold:part", "fold:full", "fold:multi", "table"}
    assert reached == want, sorted(want - reached)
    # the switch points for one MLE, and their neighbours, are among the sizes
    one = {lg: MP.plan(lg, 1, False, True) for lg in range(MP.MAX_LOG + 1)}
    first_two_pass = min(lg for lg, p in one.items() if p.passes == 2)
    first_multi = min(lg for lg, p in one.items() if p.blocks > 1)
    first_wide = min(lg for lg, p in one.items() if p.groups == 4)
    sizes = {lg for lg, n, secure, _ in MP.gpu_shapes().values() if n == 1 and not secure}
    for lg in (first_two_pass, first_multi, first_wide):
        assert {lg - 1, lg, lg + 1} & set(range(MP.MAX_GPU_VALUES.bit_length())) <= sizes, lg

"""The source generator of the native AIR kernels (no GPU): csrc/air_codegen.h compiled on its own around
tests/air_codegen_main.cpp.  The text is deterministic and has one statement per instruction; programs the interpreter refuses are
refused with the same reasons; the text compiles through hipRTC with the library's option list and through hipcc for gfx950
without a device, and neither kernel of any program here uses private (scratch) memory."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import air_program_model as X
from tstwo_amd import build as B
from tstwo_amd import constraint_framework as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")
P = X.P


def _rocm():
    """The ROCm tree hipcc belongs to (ROCM_PATH, else two levels above the compiler build.py uses)."""
    hipcc = shutil.which(B._hipcc()) or B._hipcc()
    return os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """air_codegen_main with hipRTC linked in"""
    out = str(tmp_path_factory.mktemp("air_codegen") / "air_codegen_main")
    lib = os.path.join(_rocm(), "lib")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-DAIR_CODEGEN_HIPRTC", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(_rocm(), "include"), os.path.join(HERE, "air_codegen_main.cpp"), "-o", out,
                           "-L", lib, "-lhiprtc", "-Wl,-rpath," + lib])
    return out


def _line(n_cols, n_constraints, words):
    return f"{n_cols} {n_constraints} " + " ".join(str(w & 0xffffffff) for w in words) + "\n"


def _run(exe, cases, compile_=False):
    """One answer per case (n_cols, n_constraints, words): the reason of a refusal (str) or (source text, numbers of the ok line)."""
    text = "".join(_line(*c) for c in cases)
    out = subprocess.run([exe] + (["compile"] if compile_ else []), input=text.encode(), capture_output=True, check=True).stdout
    got, at = [], 0
    for _ in cases:
        end = out.index(b"\n", at)
        head = out[at:end].decode()
        at = end + 1
        if head.startswith("error: "):
            got.append(head[len("error: "):])
            continue
        nums = [int(x) for x in head.split()[1:]]
        got.append((out[at:at + nums[0]].decode(), nums[1:]))
        at += nums[0] + 1
    assert at == len(out)
    return got


def _n_cols(words):
    return 1 + max(words[i] >> 16 for i in range(0, len(words), 2) if words[i] & 0xff == X.LOAD)


def golden_programs():
    with open(os.path.join(HERE, "golden", "air_program_words.json")) as f:
        g = json.load(f)
    assert sorted(g) == ["fibonacci_rows", "permutation", "wide_fibonacci_8"]
    return {k: (_n_cols(v["words"]), v["n_constraints"], v["words"]) for k, v in g.items()}


class ProgramWideFibonacciEval(F.WideFibonacciEval):
    """WideFibonacciEval under another type: the program path"""


def wide_fibonacci_100():
    comp = F.FrameworkComponent(ProgramWideFibonacciEval(10, 100))
    return 100, comp.program.n_constraints, list(comp.program.words)


def offsets_64():
    """loads 64 rows ahead and 64 behind, and the largest constant"""
    w = (X.encode(X.LOAD, 0, 0, 64) + X.encode(X.LOAD, 1, 1, -64) + X.encode(X.CONST, 2, 0, P - 1) + X.encode(X.MUL, 0, 0, 1)
         + X.encode(X.ADD, 0, 0, 2) + X.encode(X.ACC, 0, 0))
    return 2, 1, w


def random_programs():
    out = []
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        n_cols, n_constraints = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        out.append((n_cols, n_constraints, X.random_program(rng, n_cols, n_constraints, int(rng.integers(5, 80)), max_offset=3)))
    return out


def check_text(case, src):
    """one statement per instruction, each on a fresh name; one neighbour statement per distinct offset; the fold schedule"""
    n_cols, n_constraints, words = case
    ops = [words[i] & 0xff for i in range(0, len(words), 2)]
    names = re.findall(r"^        const V (t\d+) = ", src, flags=re.M)
    assert names == [f"t{pc}" for pc, op in enumerate(ops) if op != X.ACC]
    assert len(re.findall(r"^        accumulate<W>\(acc, t\d+, ", src, flags=re.M)) == n_constraints == ops.count(X.ACC)
    assert src.count("        fold_all<W>(acc);\n") == n_constraints // 4
    offs = {w - (1 << 32) if w >= 1 << 31 else w for i, w in zip(range(0, len(words), 2), words[1::2]) if words[i] & 0xff == X.LOAD} - {0}
    assert len(re.findall(r"= neighbour_rows<W>\(", src)) == len(offs)
    assert len(re.findall(r"= load_rows<W>\(", src)) == sum(1 for i in range(0, len(words), 2) if words[i] & 0xff == X.LOAD and words[i + 1] == 0)
    assert "__shared__" not in src and src.count('extern "C" __global__') == 2
    assert "air_native_w4" in src and "air_native_w1" in src


def test_text_is_deterministic_and_one_statement_per_instruction(exe):
    cases = list(golden_programs().values()) + random_programs() + [offsets_64()]
    first, second = _run(exe, cases), _run(exe, cases + cases)
    assert [s for s, _ in first] * 2 == [s for s, _ in second]
    for case, (src, _) in zip(cases, first):
        check_text(case, src)
    assert len({s for s, _ in first}) == len(cases)
    # a register written twice: the second value has its own name, and the ACC reads that one
    w = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.SQR, 0, 0) + X.encode(X.ACC, 0, 0)
    [(src, _)] = _run(exe, [(1, 1, w)])
    assert "const V t1 = r_sqr<W>(t0);" in src and "accumulate<W>(acc, t1, coeff[0]," in src


def test_refused_programs_give_the_interpreters_reasons(exe):
    ok = X.encode(X.LOAD, 0, 1, -2) + X.encode(X.ACC, 0, 0)
    bad = [
        ("bad opcode", (2, 1, X.encode(X.LOAD, 0, 0, 0) + X.encode(9, 1, 0, 0) + X.encode(X.ACC, 0, 0))),
        ("bad opcode", (2, 1, X.encode(X.LOAD, 0, 0, 0) + X.encode(8, 0, 0, 0) + X.encode(X.ACC, 0, 0))),          # STORE
        ("register out of range or read before written", (2, 1, X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ADD, 1, 0, 5) + X.encode(X.ACC, 0, 1))),
        ("register out of range or read before written", (2, 1, X.encode(X.LOAD, 40, 0, 0) + X.encode(X.ACC, 0, 40))),
        ("column out of range", (2, 1, X.encode(X.LOAD, 0, 2, 0) + X.encode(X.ACC, 0, 0))),
        ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, F.MAX_OFFSET + 1) + X.encode(X.ACC, 0, 0))),
        ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, -F.MAX_OFFSET - 1) + X.encode(X.ACC, 0, 0))),
        ("constant out of range", (2, 1, X.encode(X.CONST, 0, 0, P) + X.encode(X.ACC, 0, 0))),
        ("the number of ACC instructions differs from n_constraints", (2, 2, ok)),
        ("number of columns out of range", (0, 1, ok)),
        ("number of columns out of range", (F.MAX_COLS + 1, 1, ok)),
        ("program length out of range", (2, 1, [])),
        ("program length out of range", (2, 1, X.encode(X.CONST, 0, 0, 1) * F.MAX_INSTR + X.encode(X.ACC, 0, 0))),
        ("number of constraints out of range", (2, 0, ok)),
        ("number of constraints out of range", (2, F.MAX_CONSTRAINTS + 1, ok)),
    ]
    got = _run(exe, [c for _, c in bad] + [(2, 1, ok)])
    assert got[:-1] == [why for why, _ in bad]
    assert not isinstance(got[-1], str)


# ROCm 7.2's clang reports, for the gfx950 text of each program (air_native_w4 / air_native_w1): wide_fibonacci_8 90 / 23 VGPRs,
# fibonacci_rows 76 / 31, permutation 107 / 49, offsets of +-64 66 / 15, wide Fibonacci with 100 columns 193 / 51; no scratch.
def test_text_compiles_through_hiprtc_without_a_device(exe):
    cases = list(golden_programs().values()) + [offsets_64()]
    for case, (src, nums) in zip(cases, _run(exe, cases, compile_=True)):
        code_bytes, _ms, v4, s4, p4, v1, s1, p1 = nums
        assert code_bytes > 0
        assert 0 < v1 <= v4 <= 512 and 0 < s4 <= 108 and 0 < s1 <= 108, nums
        assert p4 == 0 and p1 == 0, nums              # no private segment in either kernel


def _resource_usage(src, tmp_path, name):
    """{kernel: {remark name: value}} of hipcc's kernel-resource-usage remarks for the device code of `src`"""
    path = tmp_path / (name + ".hip")
    path.write_text(src)
    p = subprocess.run([B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--offload-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", str(path), "-o", str(tmp_path / (name + ".o"))],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, kernel = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: \s*(.+?): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            kernel = usage.setdefault(m.group(2), {})
        elif kernel is not None:
            kernel[m.group(1)] = m.group(2)
    return usage


def test_no_kernel_uses_scratch(exe, tmp_path):
    cases = dict(golden_programs(), wide_fibonacci_100=wide_fibonacci_100(), offsets_64=offsets_64())
    for (name, case), (src, _) in zip(cases.items(), _run(exe, list(cases.values()))):
        usage = _resource_usage(src, tmp_path, name)
        assert sorted(usage) == ["air_native_w1", "air_native_w4"], (name, usage)
        for kernel, u in usage.items():
            print(name, kernel, "VGPRs", u["VGPRs"], "SGPRs", u["TotalSGPRs"], "scratch", u["ScratchSize [bytes/lane]"])
            assert u["ScratchSize [bytes/lane]"] == "0", (name, kernel, u)
            assert u["LDS Size [bytes/block]"] == "0", (name, kernel, u)


def test_generator_under_address_and_undefined_sanitizers(tmp_path):
    """the host code alone (no hipRTC): accepted programs up to the largest, and every refusal"""
    out = str(tmp_path / "air_codegen_san")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "air_codegen_main.cpp"), "-o", out])
    rng = np.random.default_rng(3)
    largest = (F.MAX_COLS, F.MAX_CONSTRAINTS, X.random_program(rng, F.MAX_COLS, F.MAX_CONSTRAINTS, F.MAX_INSTR - F.MAX_CONSTRAINTS, max_offset=F.MAX_OFFSET))
    cases = list(golden_programs().values()) + [offsets_64(), largest,
                                                (2, 1, X.encode(X.LOAD, 40, 0, 0) + X.encode(X.ACC, 0, 40)),
                                                (2, 1, X.encode(X.ADD, 0, 31, 0xffffffff) + X.encode(X.ACC, 0, 0)),
                                                (2, 1, [7])]                                # half an instruction
    p = subprocess.run([out], input="".join(_line(*c) for c in cases).encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    heads = [ln for ln in p.stdout.decode().splitlines() if ln.startswith(("ok ", "error: "))]
    assert [h.split()[0] for h in heads] == ["ok"] * 5 + ["error:"] * 3

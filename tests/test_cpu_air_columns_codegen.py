"""The source generator of the native column kernels (no GPU): air_columns_codegen of csrc/air_codegen.h compiled on its own
around tests/air_columns_codegen_main.cpp.  The text is deterministic, has one statement per instruction, one store_rows per STORE
and one neighbour computation per distinct offset; programs tstwo_air_eval_columns refuses are refused with the same reasons; the
text compiles through hipRTC with the library's option list and through hipcc for gfx950 without a device, and neither kernel of
any program here uses private (scratch) memory.  The text of an ACC program does not contain the column helpers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import air_program_model as X
import columns_model as CM
import interaction_evals as E
from tstwo_amd import build as B
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tstwo_amd", "csrc")
P = X.P
STORE = CM.STORE


def _rocm():
    """The ROCm tree hipcc belongs to (ROCM_PATH, else two levels above the compiler build.py uses)."""
    hipcc = shutil.which(B._hipcc()) or B._hipcc()
    return os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(tmp, main, name):
    out = str(tmp / name)
    lib = os.path.join(_rocm(), "lib")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-DAIR_CODEGEN_HIPRTC", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(_rocm(), "include"), os.path.join(HERE, main), "-o", out,
                           "-L", lib, "-lhiprtc", "-Wl,-rpath," + lib])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """air_columns_codegen_main with hipRTC linked in"""
    return _build(tmp_path_factory.mktemp("air_columns_codegen"), "air_columns_codegen_main.cpp", "air_columns_codegen_main")


def _line(n_cols, n_out, words):
    return f"{n_cols} {n_out} " + " ".join(str(w & 0xffffffff) for w in words) + "\n"


def _run(exe, cases, compile_=False):
    """One answer per case (n_cols, n_out, words): the reason of a refusal (str) or (source text, numbers of the ok line)."""
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


def general_eval():
    """compile_columns of the expressions derive_interaction_trace finds in interaction_evals.GeneralEval: 5 input columns"""
    plan = LG.plan_interaction_trace(E.GeneralEval(6, E.elements()))
    assert len(plan.exprs) == 5 and plan.n_main == 4 and plan.n_pre == 1          # m s, a b - c@-1, a^2, -m, c@+2
    program = F.compile_columns(plan.exprs, plan.n_main, plan.n_pre)
    return plan.n_main + plan.n_pre, program.n_out, list(program.words)


def outputs_64():
    """64 outputs: col0 + k for every k"""
    w = X.encode(X.LOAD, 0, 0, 0)
    for k in range(64):
        w += X.encode(X.CONST, 1, 0, k) + X.encode(X.ADD, 2, 0, 1) + X.encode(STORE, 0, 2, 63 - k)
    return 1, 64, w


def offsets_64():
    """loads 64 rows ahead and 64 behind, and the largest constant"""
    w = (X.encode(X.LOAD, 0, 0, 64) + X.encode(X.LOAD, 1, 1, -64) + X.encode(X.CONST, 2, 0, P - 1) + X.encode(X.MUL, 0, 0, 1)
         + X.encode(X.ADD, 0, 0, 2) + X.encode(STORE, 0, 0, 1) + X.encode(STORE, 0, 1, 0))
    return 2, 2, w


def random_programs():
    out = []
    for seed in range(6):
        rng = np.random.default_rng(1900 + seed)
        n_cols, n_out = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        words, k = CM.stores_for_accs(X.random_program(rng, n_cols, n_out, int(rng.integers(5, 80)), max_offset=3))
        assert k == n_out
        out.append((n_cols, n_out, words))
    return out


def check_text(case, src):
    """one statement per register-writing instruction, each on a fresh name; one store_rows per STORE; one neighbour statement per
    distinct non-zero offset"""
    n_cols, n_out, words = case
    ops = [words[i] & 0xff for i in range(0, len(words), 2)]
    names = re.findall(r"^        const V (t\d+) = ", src, flags=re.M)
    assert names == [f"t{pc}" for pc, op in enumerate(ops) if op != STORE]
    stores = re.findall(r"^        store_rows<W>\(out_at\(otab, (\d+)\), row, t\d+\);$", src, flags=re.M)
    assert len(stores) == ops.count(STORE) == n_out and sorted(int(k) for k in stores) == list(range(n_out))
    assert [int(k) for k in stores] == [words[2 * pc + 1] for pc, op in enumerate(ops) if op == STORE]
    offs = {w - (1 << 32) if w >= 1 << 31 else w for i, w in zip(range(0, len(words), 2), words[1::2]) if words[i] & 0xff == X.LOAD} - {0}
    assert len(re.findall(r"= trace_neighbour_rows<W>\(row, a\.log, ", src)) == len(offs)
    body = src[src.index("AIRN_DEV void air_columns_rows("):]         # behind the two preludes
    assert "neighbour_rows<W>(row, a.eval_log" not in body and "accumulate<W>(" not in body and "AIRN_ADD_ROWS(" not in body
    assert len(re.findall(r"= load_rows<W>\(", src)) == sum(1 for i in range(0, len(words), 2) if words[i] & 0xff == X.LOAD and words[i + 1] == 0)
    assert "__shared__" not in src and src.count('extern "C" __global__') == 2
    assert "air_columns_w4(airn::ColPtrs cols, airn::ColPtrs out, airn::ColumnsArgs a)" in src
    assert "air_columns_w1(airn::ColPtrs cols, airn::ColPtrs out, airn::ColumnsArgs a)" in src
    assert src.count("amdgpu_flat_work_group_size(1, 256)") == 2


def test_text_is_deterministic_and_one_statement_per_instruction(exe):
    cases = [general_eval(), outputs_64(), offsets_64()] + random_programs()
    first, second = _run(exe, cases), _run(exe, cases + cases)
    assert [s for s, _ in first] * 2 == [s for s, _ in second]
    for case, (src, _) in zip(cases, first):
        check_text(case, src)
    assert len({s for s, _ in first}) == len(cases)
    # a register written twice: the second value has its own name, and the STORE reads that one
    w = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.SQR, 0, 0) + X.encode(STORE, 0, 0, 0)
    [(src, _)] = _run(exe, [(1, 1, w)])
    assert "const V t1 = r_sqr<W>(t0);" in src and "store_rows<W>(out_at(otab, 0), row, t1);" in src
    # the same offset twice is one neighbour computation, and the offsets come in ascending order
    w = (X.encode(X.LOAD, 0, 0, 2) + X.encode(X.LOAD, 1, 1, 2) + X.encode(X.LOAD, 2, 0, -3) + X.encode(X.ADD, 0, 0, 1)
         + X.encode(X.ADD, 0, 0, 2) + X.encode(STORE, 0, 0, 0))
    [(src, _)] = _run(exe, [(2, 1, w)])
    assert re.findall(r"const V (n_[pm]\d+) = trace_neighbour_rows<W>\(row, a\.log, (-?\d+)\);", src) == [("n_m3", "-3"), ("n_p2", "2")]
    # log_size is an argument of the kernel, not part of the text: nothing but the program decides it
    assert "a.n_rows / W" in src and "t += a.stride" in src


def test_refused_programs_give_the_interpreters_reasons(exe):
    load = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)
    store = lambda k, reg=0: X.encode(STORE, 0, reg, k)
    ok = X.encode(X.LOAD, 0, 1, -2) + store(0)
    bad = [
        ("bad opcode", (2, 1, load + X.encode(X.ACC, 0, 0))),                                  # ACC
        ("bad opcode", (2, 1, load + X.encode(9, 1, 0, 0) + store(0))),
        ("output index out of range", (2, 2, load + store(0) + store(2, 1))),
        ("output stored twice", (2, 2, load + store(0) + store(0, 1))),
        ("an output is never stored", (2, 2, load + store(1))),
        ("register out of range or read before written", (2, 1, load + store(0, 2))),
        ("register out of range or read before written", (2, 1, X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ADD, 1, 0, 5) + store(0, 1))),
        ("register out of range or read before written", (2, 1, X.encode(X.LOAD, 40, 0, 0) + store(0, 40))),
        ("column out of range", (2, 1, X.encode(X.LOAD, 0, 2, 0) + store(0))),
        ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, F.MAX_OFFSET + 1) + store(0))),
        ("row offset beyond the limit", (2, 1, X.encode(X.LOAD, 0, 0, -F.MAX_OFFSET - 1) + store(0))),
        ("constant out of range", (2, 1, X.encode(X.CONST, 0, 0, P) + store(0))),
        ("program length out of range", (2, 1, [])),
        ("program length out of range", (2, 1, X.encode(X.CONST, 0, 0, 1) * F.MAX_INSTR + store(0))),
        ("number of columns out of range", (0, 1, ok)),
        ("number of columns out of range", (F.MAX_COLS + 1, 1, ok)),
        ("number of outputs out of range", (2, 0, ok)),
        ("number of outputs out of range", (2, F.MAX_OUT + 1, ok)),
    ]
    got = _run(exe, [c for _, c in bad] + [(2, 1, ok)])
    assert got[:-1] == [why for why, _ in bad]
    assert not isinstance(got[-1], str)


def test_text_compiles_through_hiprtc_without_a_device(exe):
    cases = [general_eval(), outputs_64(), offsets_64()] + random_programs()[:3]
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
    cases = dict(general_eval=general_eval(), outputs_64=outputs_64(), offsets_64=offsets_64(), random=random_programs()[0])
    for (name, case), (src, _) in zip(cases.items(), _run(exe, list(cases.values()))):
        usage = _resource_usage(src, tmp_path, name)
        assert sorted(usage) == ["air_columns_w1", "air_columns_w4"], (name, usage)
        for kernel, u in usage.items():
            print(name, kernel, "VGPRs", u["VGPRs"], "SGPRs", u["TotalSGPRs"], "scratch", u["ScratchSize [bytes/lane]"])
            assert u["ScratchSize [bytes/lane]"] == "0", (name, kernel, u)
            assert u["LDS Size [bytes/block]"] == "0", (name, kernel, u)


def test_the_text_of_an_acc_program_is_unchanged(exe, tmp_path):
    """air_codegen of the same build, through the existing main: the prelude and the kernels alone, none of the column helpers"""
    acc_exe = _build(tmp_path, "air_codegen_main.cpp", "air_codegen_main")
    words = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, -1) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.ACC, 0, 2))
    out = subprocess.run([acc_exe], input=_line(2, 1, words).encode(), capture_output=True, check=True).stdout.decode()
    head, acc_src = out.split("\n", 1)
    acc_src = acc_src[:int(head.split()[1])]
    with open(os.path.join(CSRC, "air_native_prelude.inc")) as f:
        prelude = f.read()
    prelude = prelude[len('R"AIRN('):prelude.rindex(')AIRN"')]
    assert acc_src.startswith(prelude + "\n// 4 instructions, 2 columns, 1 constraints\ntemplate <int W>\nAIRN_DEV void air_native_rows(")
    for helper in ("ColumnsArgs", "store_rows", "trace_neighbour_row", "out_table", "out_at"):
        assert helper not in acc_src, helper
    # and a columns text is the same prelude, then the column helpers, then its kernels
    store_words, _ = CM.stores_for_accs(words)
    [(col_src, _)] = _run(exe, [(2, 1, store_words)])
    with open(os.path.join(CSRC, "air_native_columns_prelude.inc")) as f:
        columns = f.read()
    columns = columns[len('R"AIRN('):columns.rindex(')AIRN"')]
    assert col_src.startswith(prelude + columns + "\n// 4 instructions, 2 columns, 1 outputs\ntemplate <int W>\nAIRN_DEV void air_columns_rows(")


def test_generator_under_address_and_undefined_sanitizers(tmp_path):
    """the host code alone (no hipRTC): accepted programs up to the largest, and every refusal"""
    out = str(tmp_path / "air_columns_codegen_san")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "air_columns_codegen_main.cpp"), "-o", out])
    rng = np.random.default_rng(3)
    words, k = CM.stores_for_accs(X.random_program(rng, F.MAX_COLS, F.MAX_OUT, F.MAX_INSTR - F.MAX_OUT, max_offset=F.MAX_OFFSET))
    largest = (F.MAX_COLS, k, words)
    store = lambda k, reg=0: X.encode(STORE, 0, reg, k)
    load = X.encode(X.LOAD, 0, 0, 0)
    cases = [general_eval(), outputs_64(), offsets_64(), largest,
             (2, 1, X.encode(X.LOAD, 40, 0, 0) + store(0, 40)),
             (2, 1, X.encode(X.ADD, 0, 31, 0xffffffff) + store(0)),
             (2, 1, load + store(0xffffffff)),                         # an output index far outside the table
             (2, 64, load + store(64)),
             (2, 2, load + store(1) + store(1)),
             (2, 2, load + store(1)),
             (2, 1, load + X.encode(X.ACC, 0, 0)),
             (2, 65, load + store(0)),
             (2, 1, [7])]                                              # half an instruction
    p = subprocess.run([out], input="".join(_line(*c) for c in cases).encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    heads = [ln for ln in p.stdout.decode().splitlines() if ln.startswith(("ok ", "error: "))]
    assert [h.split()[0] for h in heads] == ["ok"] * 4 + ["error:"] * 9

"""Constraint programs compiled to native kernels on the MI355X (tstwo_air_program_compile / tstwo_air_eval_compiled): bit-exact
against the integer model (tests/air_program_model.py) on random programs, on both widths, at every fold count and with every
operand at P - 1; against the interpreter where the grid strides; a FrameworkComponent with native=True against the same
component without it, up to identical proofs; kernel ids, refusals, resource figures and guard bands."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import air_model as M
import air_plan as AP
import air_program_model as X
import saturation as S
from arena import Arena, rin, rinout
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier
from tstwo_amd.poly import HipCircleEvaluation, interpolate_columns, precompute_twiddles
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel
from tstwo_amd.prover import ConstraintsNotSatisfied, prove, verify

pytestmark = pytest.mark.gpu

P = M.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 7                               # TSTWO_ERR_BAD_ARG

_kernels = {}                             # (words, n_cols, n_constraints) -> kernel id: one compilation per program in this module


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()
    for kid in _kernels.values():
        L.call("tstwo_air_program_destroy", kid)
    _kernels.clear()


def kernel_info(kid):
    w = (C.c_uint32 * 7)()
    L.call("tstwo_air_kernel_info", kid, w)
    return list(w)


def compile_words(words, n_cols, n_constraints):
    """The kernel of a program (compiled once); neither width of any kernel of this module has a private segment."""
    key = (tuple(words), n_cols, n_constraints)
    if key not in _kernels:
        kid = C.c_uint64(0)
        L.call("tstwo_air_program_compile", L.u32x(words), len(words) // 2, n_cols, n_constraints, C.byref(kid))
        info = kernel_info(kid.value)
        assert info[2] == 0 and info[5] == 0 and info[0] > 0 and info[3] > 0 and info[6] > 0, info
        _kernels[key] = kid.value
    return _kernels[key]


def rand_felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def col(a):
    return HipColumn(np.asarray(a, dtype=np.uint32))


def call_native(kid, col_ptrs, trace_log, log_expand, coeffs, dinv, acc_ptrs):
    cw = L.u32x([w for c in coeffs for w in c])
    L.call("tstwo_air_eval_compiled", kid, L.ptr_array(col_ptrs), len(col_ptrs), trace_log, log_expand, cw,
           len(coeffs), L.u32x([int(d) for d in dinv]), L.p4(acc_ptrs))


def call_interpreter(words, col_ptrs, trace_log, log_expand, coeffs, dinv, acc_ptrs):
    cw = L.u32x([w for c in coeffs for w in c])
    L.call("tstwo_air_eval_program", L.ptr_array(col_ptrs), len(col_ptrs), trace_log, log_expand, L.u32x(words), len(words) // 2,
           cw, len(coeffs), L.u32x([int(d) for d in dinv]), L.p4(acc_ptrs))


def check_against_model(words, cols, trace_log, log_expand, coeffs, dinv, pre, aligned=True):
    """accum (non-zero on entry: `pre`) after the native kernel == the model's; unaligned: every column and accumulator starts one
    word into its buffer, which takes the W = 1 kernel."""
    kid = compile_words(words, len(cols), len(coeffs))
    want = X.eval_program_on_domain(words, cols, trace_log, log_expand, coeffs, dinv, pre)
    k = 0 if aligned else 1
    dcols = [col(np.concatenate([np.zeros(k, dtype=np.uint64), c])) for c in cols]
    dacc = [col(np.concatenate([np.zeros(k, dtype=np.uint64), pre[j]])) for j in range(4)]
    call_native(kid, [c.ptr + 4 * k for c in dcols], trace_log, log_expand, coeffs, dinv, [a.ptr + 4 * k for a in dacc])
    for j in range(4):
        got = dacc[j].to_numpy()[k:]
        bad = np.flatnonzero(got != want[j].astype(np.uint32))
        assert bad.size == 0, ("coordinate", j, "first wrong row", int(bad[0]), "wrong rows", int(bad.size))


def random_case(seed, trace_log, log_expand, n_cols, n_constraints, n_ops, aligned=True, program_seed=None):
    """Random columns, coefficients and a non-zero accumulator for the random program of `program_seed` (default: seed)."""
    words = X.random_program(np.random.default_rng(seed if program_seed is None else program_seed), n_cols, n_constraints, n_ops, max_offset=3)
    rng = np.random.default_rng(10_000 + seed)
    n = 1 << (trace_log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    coeffs = [rand_felt(rng) for _ in range(n_constraints)]
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    check_against_model(words, cols, trace_log, log_expand, coeffs, M.denom_inv(trace_log, trace_log + log_expand), pre, aligned)


# ------------------------------------------------------------------ the kernels against the model
SHAPES = [(1, 1), (2, 1), (3, 4), (6, 2), (10, 3)]


@pytest.mark.parametrize("trace_log,log_expand", SHAPES)
def test_random_programs_match_the_model(trace_log, log_expand):
    """three programs (offsets up to 3), each compiled once and run at every shape: the accumulator is added to"""
    for program_seed in (41, 42, 43):
        random_case(100 * trace_log + log_expand + program_seed, trace_log, log_expand, n_cols=6, n_constraints=5, n_ops=40,
                    program_seed=program_seed)


def test_offsets_of_64_rows_and_a_negative_constant():
    trace_log, log_expand = 8, 2
    w = (X.encode(X.LOAD, 0, 0, 64) + X.encode(X.LOAD, 1, 1, -64) + X.encode(X.CONST, 2, 0, P - 5) + X.encode(X.MUL, 3, 0, 1)
         + X.encode(X.ADD, 3, 3, 2) + X.encode(X.LOAD, 4, 0, 0) + X.encode(X.SUB, 4, 4, 3) + X.encode(X.ACC, 0, 3) + X.encode(X.ACC, 0, 4))
    rng = np.random.default_rng(64)
    n = 1 << (trace_log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2)]
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    for aligned in (True, False):
        check_against_model(w, cols, trace_log, log_expand, [rand_felt(rng), rand_felt(rng)], M.denom_inv(trace_log, trace_log + log_expand), pre, aligned)


@pytest.mark.parametrize("trace_log,log_expand", [(2, 1), (6, 2), (10, 3), (13, 1)])
def test_one_row_kernel_for_unaligned_columns(trace_log, log_expand):
    """columns and accumulators one word off a 16-byte boundary: W = 1"""
    random_case(200 + trace_log, trace_log, log_expand, n_cols=5, n_constraints=3, n_ops=30, aligned=False, program_seed=44)


def test_two_rows_in_all():
    """trace_log 0, log_expand 1: two rows, not a multiple of four, so W = 1 on aligned columns"""
    random_case(557, 0, 1, n_cols=3, n_constraints=2, n_ops=12)


def test_more_than_64_columns():
    """the column table in device memory (`ext`)"""
    random_case(555, 9, 2, n_cols=90, n_constraints=7, n_ops=120)
    random_case(556, 5, 1, n_cols=90, n_constraints=7, n_ops=120, aligned=False, program_seed=555)


# ------------------------------------------------------------------ the fold schedule, at saturating operands
# Compile time grows faster than the number of ACCs (16 multiply-add chains each, one scheduling region): 64 ACCs take 3.5 s,
# 100 take 6 s, the limit of 256 takes 25 s and a program of 1536 random instructions 17 s, so 64 is the large count run here.
@pytest.mark.parametrize("n_constraints", [1, 3, 4, 5, 8, 9, 64])
def test_fold_schedule_at_saturating_operands(n_constraints):
    """every column word, coefficient word, denominator and accumulator word is P - 1: each product is the largest there is, and
    the 64-bit sums reach the bound the fold after every fourth ACC keeps them under"""
    trace_log, log_expand = 3, 1
    n = 1 << (trace_log + log_expand)
    words = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)
    for k in range(n_constraints):
        words += X.encode(X.ACC, 0, k & 1)
    cols = [np.full(n, S.SAT, dtype=np.uint64) for _ in range(2)]
    pre = np.full((4, n), S.SAT, dtype=np.uint64)
    for aligned in (True, False):
        check_against_model(words, cols, trace_log, log_expand, [S.SAT4] * n_constraints, [S.SAT] * (1 << log_expand), pre, aligned)


@pytest.mark.parametrize("n_acc,way", [(k, w) for k in (1, 3, 4, 5, 8, 9) for w in ("load0", "load-1", "mul")] + [(0, "opcodes")])
def test_saturation_cases_of_the_interpreter(n_acc, way):
    """the operands tests/saturation.py gives the interpreter (P - 1 on the masked rows, sums of exactly P, NEG 0), on both widths"""
    for aligned in (True, False):
        c = S.program_case(n_acc, way, 2, aligned)
        check_against_model(c["words"], [np.asarray(x, dtype=np.uint64) for x in c["cols"]], c["trace_log"], c["log_expand"], c["coeffs"],
                            c["dinv"], np.asarray(c["accum"], dtype=np.uint64), aligned)


# ------------------------------------------------------------------ the stride loop
def _n_cus():
    return int(re.search(r"(\d+) CUs", L.device_name()).group(1))


@pytest.mark.parametrize("aligned", [True, False], ids=["23-True", "21-False"])
def test_rows_beyond_the_grid_cap_match_the_interpreter(aligned):
    """More rows than the compiled kernel's grid covers at W rows per lane (tests/air_plan.py, for this part's CUs): lanes stride.
    3 columns, the smallest log that gets there (23 and 21 on 256 CUs); compared against the interpreter on the device."""
    log_expand = 2
    eval_log = AP.first_striding_log("eval_compiled", 4 if aligned else 1, _n_cus())
    shape = AP.Input("eval_compiled", 0, eval_log, log_expand, 3, 2, 0, 0, aligned, _n_cus())
    assert AP.plan(shape).w == (4 if aligned else 1) and AP.strides(shape) and not AP.strides(shape._replace(log=eval_log - 1))
    assert AP.strides(shape._replace(entry="eval_program", program_len=8, n_regs=5))      # and the interpreter beside it
    trace_log = eval_log - log_expand
    n, k = 1 << eval_log, 0 if aligned else 1
    words = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1) + X.encode(X.LOAD, 2, 2, -1) + X.encode(X.MUL, 3, 0, 1)
             + X.encode(X.SUB, 3, 3, 2) + X.encode(X.SQR, 4, 2) + X.encode(X.ACC, 0, 3) + X.encode(X.ACC, 0, 4))
    rng = np.random.default_rng(eval_log)
    dcols = [col(rng.integers(0, P, size=n + k, dtype=np.uint32)) for _ in range(3)]
    pre = rng.integers(0, P, size=n + k, dtype=np.uint32)
    coeffs, dinv = [rand_felt(rng), rand_felt(rng)], M.denom_inv(trace_log, eval_log)
    kid = compile_words(words, 3, 2)
    out = []
    for run in (lambda ptrs: call_interpreter(words, [c.ptr + 4 * k for c in dcols], trace_log, log_expand, coeffs, dinv, ptrs),
                lambda ptrs: call_native(kid, [c.ptr + 4 * k for c in dcols], trace_log, log_expand, coeffs, dinv, ptrs)):
        acc = [col(pre) for _ in range(4)]
        run([a.ptr + 4 * k for a in acc])
        out.append([a.to_numpy() for a in acc])
    for j in range(4):
        assert np.array_equal(out[0][j], out[1][j]), j
        assert not np.array_equal(out[1][j][k:], pre[k:])


# ------------------------------------------------------------------ ids, refusals
OK_WORDS = X.encode(X.LOAD, 0, 0, -1) + X.encode(X.LOAD, 1, 1, 1) + X.encode(X.MUL, 0, 0, 1) + X.encode(X.ACC, 0, 0)


def _small_io(n_cols=2, log=6):
    return [col(np.arange(1 << log)) for _ in range(n_cols)], [col(np.zeros(1 << log)) for _ in range(4)]


def test_unknown_and_destroyed_ids_are_refused():
    cols, acc = _small_io()
    dinv = M.denom_inv(4, 6)
    fresh = C.c_uint64(0)
    L.call("tstwo_air_program_compile", L.u32x(OK_WORDS), 4, 2, 1, C.byref(fresh))
    call_native(fresh.value, [c.ptr for c in cols], 4, 2, [(1, 0, 0, 0)], dinv, [a.ptr for a in acc])
    L.call("tstwo_air_program_destroy", fresh.value)
    for kid in (0, fresh.value, fresh.value + 1000, (1 << 64) - 1):
        for call in (lambda: call_native(kid, [c.ptr for c in cols], 4, 2, [(1, 0, 0, 0)], dinv, [a.ptr for a in acc]),
                     lambda: kernel_info(kid), lambda: L.call("tstwo_air_program_destroy", kid)):
            with pytest.raises(L.TstwoError, match="unknown air kernel") as e:
                call()
            assert e.value.code == BAD_ARG
    again = C.c_uint64(0)
    L.call("tstwo_air_program_compile", L.u32x(OK_WORDS), 4, 2, 1, C.byref(again))
    assert again.value != fresh.value                       # an id is handed out once
    L.call("tstwo_air_program_destroy", again.value)


def test_ids_from_before_a_shutdown_are_unknown():
    """tstwo_shutdown unloads every kernel; in a process of its own, because it also frees every device buffer of the process"""
    code = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
        import ctypes as C
        import numpy as np
        import air_program_model as X
        from tstwo_amd import _lib as L
        from tstwo_amd import constraint_framework as F
        L.init(0)
        program = F.Program({OK_WORDS!r}, 2, 1, 2)
        old = F.compile_native(program, 2)
        assert F.compile_native(program, 2) is old              # cached
        L.call("tstwo_shutdown")
        L.init(0)
        w = (C.c_uint32 * 7)()
        try:
            L.call("tstwo_air_kernel_info", old.id, w)
            raise SystemExit("a kernel id survived tstwo_shutdown")
        except L.TstwoError as e:
            assert e.code == 7 and "unknown air kernel" in str(e), e
        new = F.compile_native(program, 2)                      # the cache notices
        assert new is not old and new.id != old.id
        assert new.info()["w4"]["private_bytes"] == 0
        print("shutdown ok")
    """)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "shutdown ok" in p.stdout, p.stderr[-2000:]


def test_mismatched_shapes_and_bad_arguments_are_refused():
    kid = compile_words(OK_WORDS, 2, 1)
    cols, acc = _small_io(3)
    dinv = M.denom_inv(4, 6)
    ptrs, accp = [c.ptr for c in cols], [a.ptr for a in acc]
    with pytest.raises(L.TstwoError, match="another number of columns"):
        call_native(kid, ptrs, 4, 2, [(1, 0, 0, 0)], dinv, accp)
    with pytest.raises(L.TstwoError, match="another number of constraints"):
        call_native(kid, ptrs[:2], 4, 2, [(1, 0, 0, 0)] * 2, dinv, accp)
    with pytest.raises(L.TstwoError, match="log_expand"):
        call_native(kid, ptrs[:2], 6, 0, [(1, 0, 0, 0)], [1], accp)
    with pytest.raises(L.TstwoError, match="log_expand too large"):
        call_native(kid, ptrs[:2], 1, 5, [(1, 0, 0, 0)], [1] * 32, accp)
    with pytest.raises(L.TstwoError, match="evaluation domain too large"):
        call_native(kid, ptrs[:2], 27, 2, [(1, 0, 0, 0)], dinv, accp)
    with pytest.raises(L.TstwoError, match="coefficient word out of range"):
        call_native(kid, ptrs[:2], 4, 2, [(P, 0, 0, 0)], dinv, accp)
    with pytest.raises(L.TstwoError, match="denominator out of range"):
        call_native(kid, ptrs[:2], 4, 2, [(1, 0, 0, 0)], [P] * 4, accp)
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        call_native(kid, [ptrs[0], 0], 4, 2, [(1, 0, 0, 0)], dinv, accp)
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        call_native(kid, ptrs[:2], 4, 2, [(1, 0, 0, 0)], dinv, accp[:3] + [0])
    call_native(kid, ptrs[:2], 4, 2, [(1, 0, 0, 0)], dinv, accp)                 # still works


def test_compile_refuses_what_the_interpreter_refuses():
    kid = C.c_uint64(0)
    bad = {
        "air program: bad opcode": X.encode(X.LOAD, 0, 0, 0) + X.encode(9, 1, 0, 0) + X.encode(X.ACC, 0, 0),
        "air program: register out of range or read before written": X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ADD, 1, 0, 5) + X.encode(X.ACC, 0, 1),
        "air program: column out of range": X.encode(X.LOAD, 0, 2, 0) + X.encode(X.ACC, 0, 0),
        "air program: row offset beyond the limit": X.encode(X.LOAD, 0, 0, F.MAX_OFFSET + 1) + X.encode(X.ACC, 0, 0),
        "air program: constant out of range": X.encode(X.CONST, 0, 0, P) + X.encode(X.ACC, 0, 0),
        "air program: the number of ACC instructions differs from n_constraints": X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ACC, 0, 0) * 2,
    }
    for what, words in bad.items():
        with pytest.raises(L.TstwoError, match=what) as e:
            L.call("tstwo_air_program_compile", L.u32x(words), len(words) // 2, 2, 1, C.byref(kid))
        assert e.value.code == BAD_ARG and kid.value == 0


def test_entries_are_refused_during_graph_capture():
    kid = compile_words(OK_WORDS, 2, 1)
    rng = np.random.default_rng(9)
    n = 1 << 6
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2)]
    coeffs, dinv = [rand_felt(rng)], M.denom_inv(4, 6)
    dcols, acc = [col(c) for c in cols], [col(np.zeros(n)) for _ in range(4)]
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="host-array upload during graph capture \\(the air program and its coefficients cannot be recorded\\)"):
            call_native(kid, [c.ptr for c in dcols], 4, 2, coeffs, dinv, [a.ptr for a in acc])
        with pytest.raises(L.TstwoError, match="refused during graph capture"):
            L.call("tstwo_air_program_compile", L.u32x(OK_WORDS), 4, 2, 1, C.byref(C.c_uint64(0)))
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)
    call_native(kid, [c.ptr for c in dcols], 4, 2, coeffs, dinv, [a.ptr for a in acc])
    want = X.eval_program_on_domain(OK_WORDS, cols, 4, 2, coeffs, dinv)
    for j in range(4):
        assert np.array_equal(acc[j].to_numpy(), want[j].astype(np.uint32))


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("log", [1, 5, 9])
def test_nothing_but_the_accumulators_is_written(log, offset):
    """every column is unchanged and no byte outside the four accumulator columns is written: W = 4 (offset 0) and W = 1"""
    log_expand, n_cols, n_constraints = 1, 6, 5
    rng = np.random.default_rng(7 * log + log_expand)
    n = 1 << (log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    words = X.random_program(rng, n_cols, n_constraints, 40, max_offset=3)
    coeffs = [rand_felt(rng) for _ in range(n_constraints)]
    dinv = M.denom_inv(log, log + log_expand)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    c_, a_ = [f"col{i}" for i in range(n_cols)], [f"acc{j}" for j in range(4)]
    regs = [rin(x, c.astype(np.uint32), offset) for x, c in zip(c_, cols)] + [rinout(x, pre[j].astype(np.uint32), offset) for j, x in enumerate(a_)]
    kid = compile_words(words, n_cols, n_constraints)
    with Arena(regs) as arena:
        L.call("tstwo_air_eval_compiled", kid, arena.ptrs(c_), n_cols, log, log_expand, L.u32x([w for c in coeffs for w in c]),
               n_constraints, L.u32x([int(d) for d in dinv]), arena.p4(a_))
        got = arena.check()
    want = X.eval_program_on_domain(words, cols, log, log_expand, coeffs, dinv, pre)
    for j, x in enumerate(a_):
        assert np.array_equal(got[x], want[j].astype(np.uint32)), x


# ------------------------------------------------------------------ FrameworkComponent(native=True)
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, col(c)) for c in cols]


def _trace(trees, twiddles):
    """A.Trace of the committed evaluations per tree and their polynomials (the components evaluate those on their own domain)"""
    polys = [interpolate_columns(evs, twiddles) if evs else [] for evs in trees]
    return A.Trace(polys, [list(evs) for evs in trees])


def _same_composition(plain, native, trace, twiddles, seed=5):
    assert all(c.native is None for c in plain) and all(c.native is not None for c in native)
    for c in native:
        info = c.native_info()
        assert info["w4"]["private_bytes"] == 0 and info["w1"]["private_bytes"] == 0 and info["compile_seconds"] > 0, info
    alpha = QM31.from_u32_unchecked(*rand_felt(np.random.default_rng(seed)))
    n_pre = len(trace.polys[0])
    want = A.ComponentProvers(plain, n_pre).compute_composition_polynomial(alpha, trace, twiddles)
    got = A.ComponentProvers(native, n_pre).compute_composition_polynomial(alpha, trace, twiddles)
    for j in range(4):
        assert np.array_equal(got[j].coeffs.to_numpy(), want[j].coeffs.to_numpy()), j
        assert got[j].coeffs.to_numpy().any()


def test_fibonacci_rows_composition_is_identical():
    log = 8
    a, b = F.fibonacci_rows_trace(log, 3, 5)
    a = (a.astype(np.uint64) * 7 + 1) % P                   # constraints that do not vanish: every word of the composition counts
    tw = precompute_twiddles(CanonicCoset(log + 3).circleDomain().halfCoset)
    trace = _trace([_evals([F.is_first_column(log)], log), _evals([a, b], log)], tw)
    comps = [F.FrameworkComponent(F.FibonacciRowsEval(log, 3, 5), None, [0], native=nat) for nat in (False, True)]
    _same_composition([comps[0]], [comps[1]], trace, tw)
    # the same eval at another size shares the kernel: one compilation per program
    assert F.FrameworkComponent(F.FibonacciRowsEval(log + 3, 3, 5), None, [0], native=True).native is comps[1].native
    # the hand-written kinds keep their kernels
    assert F.WideFibonacciComponent(log, 8).native is None and F.FrameworkComponent(F.MulAddEval(log), native=True).native is None


def test_permutation_composition_is_identical():
    log = 7
    rng = np.random.default_rng(log)
    a = rng.integers(0, P, size=1 << log, dtype=np.uint32)
    b = rng.integers(0, P, size=1 << log, dtype=np.uint32)          # not a permutation: the LogUp constraints do not vanish
    le = LG.LookupElements.draw(Blake2sChannel(), 1)
    inter, claimed = F.permutation_interaction_trace(log, a, rng.permutation(a), le)
    tw = precompute_twiddles(CanonicCoset(log + 3).circleDomain().halfCoset)
    trace = _trace([[], _evals([a, b], log), inter], tw)
    comps = [F.FrameworkComponent(F.PermutationEval(log, le), claimed_sum=claimed, native=nat) for nat in (False, True)]
    assert any(comps[1].secure_flags)                               # secure constraints: expand_coeffs on the native path too
    _same_composition([comps[0]], [comps[1]], trace, tw)


def test_range_check_compositions_are_identical():
    log_range, log_values = 6, 7
    rng = np.random.default_rng(3)
    v0 = rng.integers(0, 1 << log_range, size=1 << log_values)
    v1 = rng.integers(0, 1 << log_range, size=1 << log_values)
    mult = F.range_check_multiplicities(log_range, v0, v1)
    le = LG.LookupElements.draw(Blake2sChannel(), 1)
    t_inter, t_sum = F.range_check_table_interaction_trace(log_range, mult, le)
    v_inter, v_sum = F.range_check_values_interaction_trace(log_values, v0.astype(np.uint32), v1.astype(np.uint32), le)
    v1_broken = (v1 + 1).astype(np.uint32)                          # the values component's constraints do not vanish
    tw = precompute_twiddles(CanonicCoset(log_values + 3).circleDomain().halfCoset)
    trace = _trace([_evals([F.range_check_table_column(log_range)], log_range),
                    _evals([mult], log_range) + _evals([v0, v1_broken], log_values), t_inter + v_inter], tw)

    def components(native):
        alloc = A.TraceLocationAllocator()
        return [F.FrameworkComponent(F.RangeCheckTableEval(log_range, le), alloc, [0], claimed_sum=t_sum, native=native),
                F.FrameworkComponent(F.RangeCheckValuesEval(log_values, le), alloc, claimed_sum=v_sum, native=native)]
    _same_composition(components(False), components(True), trace, tw)


def _prove_fibonacci_rows(log, native, channel_cls, merkle=None, break_at=None):
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, 3, 5), None, [0], native=native)
    a, b = F.fibonacci_rows_trace(log, 3, 5)
    if break_at is not None:
        pos = F.coset_order_positions(log)[break_at]
        b = b.copy()
        b[pos] = (int(b[pos]) + 1) % P
    config = PcsConfig()
    tw = precompute_twiddles(CanonicCoset(comp.max_constraint_log_degree_bound() + config.fri_config.log_blowup_factor).circleDomain().halfCoset)
    scheme, ch = CommitmentSchemeProver(config, tw, merkle), channel_cls()
    for evs in (_evals([F.is_first_column(log)], log), _evals([a, b], log)):
        tb = scheme.tree_builder()
        tb.extend_evals(evs)
        tb.commit(ch)
    return comp, prove([comp], ch, scheme), config


@pytest.mark.parametrize("log,channel_cls,merkle", [(5, Blake2sChannel, None), (9, Blake2sChannel, None),
                                                    (4, Poseidon252Channel, Poseidon252MerkleChannel)])
def test_proofs_are_identical_and_verify(log, channel_cls, merkle):
    _, plain, _ = _prove_fibonacci_rows(log, False, channel_cls, merkle)
    comp, proof, config = _prove_fibonacci_rows(log, True, channel_cls, merkle)
    assert comp.native is not None
    assert proof.commitments == plain.commitments
    assert proof.sampled_values == plain.sampled_values
    assert proof.proof_of_work == plain.proof_of_work
    ch, v = channel_cls(), CommitmentSchemeVerifier(config, merkle)
    sizes = A.Components([comp], 1).column_log_sizes()
    v.commit(proof.commitments[0], [log], ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    verify([comp], ch, v, proof)


def test_a_broken_trace_is_still_refused():
    with pytest.raises(ConstraintsNotSatisfied):
        _prove_fibonacci_rows(7, True, Blake2sChannel, break_at=40)

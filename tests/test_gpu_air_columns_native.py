"""Column programs compiled to native kernels on the MI355X (tstwo_air_columns_compile / tstwo_air_eval_columns_compiled): bit
for bit against the integer model (tests/columns_model.py run_columns) and against the interpreter tstwo_air_eval_columns on the
same buffers, with every device argument inside a guarded arena (tests/arena.py: nothing written outside the n_out outputs,
nothing into the inputs); against the interpreter alone where the grid strides; argument errors, kernel kinds and ids, each with
its text; one launch recorded into a graph and replayed on other data; one call sequence behind a plug (tests/sequence.py).

Shapes, those of tests/test_gpu_air_columns.py: log 1 and 2 (one row per lane; the bit reversal over 0 and 1 bits), log 3 (four
rows per lane, two lanes), log 8 and 9, log 12 with every column one word off a 16-byte boundary (one row per lane at a size that
would vectorise), each at all four placements; programs of 1 and of 32 registers; 1 and 64 outputs; 65 input columns (the column
table in device memory); offsets of +-64 rows; log 23 aligned and log 21 one word off, where lanes stride."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import P

pytestmark = pytest.mark.gpu

import air_model as M  # noqa: E402
import air_plan as AP  # noqa: E402
import air_program_model as X  # noqa: E402
import columns_model as CM  # noqa: E402
import sequence as SQ  # noqa: E402
from arena import Arena, rin, rout  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd.backend import HipColumn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 7                               # TSTWO_ERR_BAD_ARG
PLACEMENTS = ("aligned", "all+4", "out+4", "in+4")
STORE = CM.STORE

_kernels = {}                             # (words, n_cols, n_out) -> kernel id: one compilation per program in this module


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


def compile_raw(words, n_cols, n_out):
    kid = C.c_uint64(0)
    L.call("tstwo_air_columns_compile", L.u32x(words), len(words) // 2, n_cols, n_out, C.byref(kid))
    return kid.value


def compile_words(words, n_cols, n_out):
    """The kernel of a columns program (compiled once); neither width of any kernel of this module has a private segment."""
    key = (tuple(words), n_cols, n_out)
    if key not in _kernels:
        kid = compile_raw(words, n_cols, n_out)
        info = kernel_info(kid)
        assert info[2] == 0 and info[5] == 0 and info[0] > 0 and info[3] > 0 and info[6] > 0, info
        _kernels[key] = kid
    return _kernels[key]


def call_native(kid, col_ptrs, log, out_ptrs):
    L.call("tstwo_air_eval_columns_compiled", kid, L.ptr_array(col_ptrs), len(col_ptrs), log, L.ptr_array(out_ptrs), len(out_ptrs))


def call_interpreter(words, col_ptrs, log, out_ptrs):
    L.call("tstwo_air_eval_columns", L.ptr_array(col_ptrs), len(col_ptrs), log, L.u32x(words), len(words) // 2,
           L.ptr_array(out_ptrs), len(out_ptrs))


def random_columns_program(rng, n_cols, n_out, n_ops, max_regs=32, max_offset=3):
    words, k = CM.stores_for_accs(X.random_program(rng, n_cols, n_out, n_ops, max_regs=max_regs, max_offset=max_offset))
    assert k == n_out
    return words


def registers_written(words):
    return 1 + max((w >> 8) & 0xff for w in words[::2] if w & 0xff not in (X.ACC, STORE))


def in_arena(words, cols, log, n_out, place="aligned"):
    """The native kernel, then the interpreter, each with every column in a guarded arena of its own (the same layout, so the
    same addresses modulo 16); returns both sets of outputs after the guards and the inputs were checked."""
    c_, o_ = [f"col{i}" for i in range(len(cols))], [f"out{k}" for k in range(n_out)]
    off = {x: 0 for x in c_ + o_}
    if place == "all+4":
        off = {x: 4 for x in off}
    elif place == "out+4":
        off.update({x: 4 for x in o_})
    elif place == "in+4":
        off[c_[0]] = 4
    kid = compile_words(words, len(cols), n_out)
    both = []
    for native in (True, False):
        regs = [rin(x, c.astype(np.uint32), off[x]) for x, c in zip(c_, cols)] + [rout(x, 1 << log, off[x]) for x in o_]
        with Arena(regs) as A:
            if native:
                L.call("tstwo_air_eval_columns_compiled", kid, A.ptrs(c_), len(cols), log, A.ptrs(o_), n_out)
            else:
                L.call("tstwo_air_eval_columns", A.ptrs(c_), len(cols), log, L.u32x(words), len(words) // 2, A.ptrs(o_), n_out)
            got = A.check()
        both.append([got[x] for x in o_])
    return both


def check_words(words, cols, log, n_out, place="aligned"):
    got, interpreted = in_arena(words, cols, log, n_out, place)
    want = CM.run_columns(words, cols, log, n_out)
    for k in range(n_out):
        assert np.array_equal(got[k], want[k].astype(np.uint32)), f"output {k} against the model"
        assert np.array_equal(got[k], interpreted[k]), f"output {k} against the interpreter"
    return got


def check_case(seed, log, n_cols, n_out, n_ops, max_regs=32, max_offset=3, place="aligned", first_load=None, program_seed=None):
    """first_load: the column the program's first LOAD is made to read.  program_seed: the program (default: seed); the columns
    always come from `seed`, so one compiled program serves several shapes and placements."""
    words = random_columns_program(np.random.default_rng(seed if program_seed is None else program_seed), n_cols, n_out, n_ops, max_regs, max_offset)
    rng = np.random.default_rng(20_000 + seed)
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(n_cols)]
    if first_load is not None:
        assert words[0] & 0xff == X.LOAD
        words[0] = (words[0] & 0xffff) | (first_load << 16)
    check_words(words, cols, log, n_out, place)
    return words


# ------------------------------------------------------------------ the kernels against the model and the interpreter
# (id, log, input columns, outputs, operations): the program of a shape is one for all its placements
SHAPES = [("log1", 1, 3, 2, 24), ("log2", 2, 3, 2, 24), ("log3", 3, 4, 3, 30), ("log8", 8, 6, 5, 40), ("log9", 9, 6, 5, 40)]


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("name,log,n_cols,n_out,n_ops", SHAPES, ids=[s[0] for s in SHAPES])
def test_random_programs_match_the_model_and_the_interpreter(name, log, n_cols, n_out, n_ops, place):
    """the arena asserts the guard bands around every region and the input regions: a store outside an output, or into an input,
    fails"""
    words = check_case(500 + log + 100 * PLACEMENTS.index(place), log, n_cols, n_out, n_ops, place=place, program_seed=700 + n_cols)
    assert any(w & 0xff == X.LOAD and words[2 * i + 1] != 0 for i, w in enumerate(words[::2])), "no load at an offset"


def test_one_row_kernel_at_a_size_that_would_vectorise():
    """log 12 with every column one word off a 16-byte boundary: W = 1"""
    check_case(512, 12, 4, 3, 30, place="all+4", program_seed=704)


def test_a_program_of_one_register():
    words = check_case(41, 5, 3, 1, 12, max_regs=1)
    assert registers_written(words) == 1


def test_a_program_of_32_registers():
    words = check_case(42, 5, 6, 4, 80)
    assert registers_written(words) == 32


def test_one_output_and_64_outputs():
    check_case(43, 4, 5, 1, 30)
    check_case(44, 4, 5, 64, 40)


def test_65_input_columns():
    """the column table in device memory (`ext`); the first load reads column 64"""
    check_case(45, 4, 65, 3, 120, first_load=64)


@pytest.mark.parametrize("log", [4, 9])
@pytest.mark.parametrize("offset", [64, -64])
def test_the_largest_offsets(log, offset):
    """+-64 rows: within the trace at log 9, four whole turns at log 4."""
    rng = np.random.default_rng(46 + log)
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(2)]
    words = (X.encode(X.LOAD, 0, 0, offset) + X.encode(X.LOAD, 1, 1, -offset) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.LOAD, 3, 1, 0)
             + X.encode(X.SUB, 2, 2, 3) + X.encode(STORE, 0, 2, 1) + X.encode(STORE, 0, 0, 0))
    got = check_words(words, cols, log, 2)
    assert np.array_equal(got[0], cols[0][X.neighbour_map(log, log, offset)].astype(np.uint32))


# ------------------------------------------------------------------ the stride loop
def _n_cus():
    return int(re.search(r"(\d+) CUs", L.device_name()).group(1))


@pytest.mark.parametrize("aligned", [True, False], ids=["23-True", "21-False"])
def test_rows_beyond_the_grid_cap_match_the_interpreter(aligned):
    """More rows than the compiled kernel's grid covers at W rows per lane (tests/air_plan.py, for this part's CUs): lanes stride.
    A 7-instruction program over 2 columns, the smallest log that gets there (23 and 21 on 256 CUs); compared against the
    interpreter on the device."""
    log = AP.first_striding_log("eval_columns_compiled", 4 if aligned else 1, _n_cus())
    shape = AP.Input("eval_columns_compiled", 0, log, 0, 2, 1, 0, 0, aligned, _n_cus())
    assert AP.plan(shape).w == (4 if aligned else 1) and AP.strides(shape) and not AP.strides(shape._replace(log=log - 1))
    assert AP.strides(shape._replace(entry="eval_columns", program_len=7, n_regs=3))      # and the interpreter beside it
    n, k = 1 << log, 0 if aligned else 1
    words = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, -1) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.LOAD, 1, 0, 2)
             + X.encode(X.ADD, 2, 2, 1) + X.encode(X.NEG, 2, 2) + X.encode(STORE, 0, 2, 0))
    rng = np.random.default_rng(log)
    dcols = [HipColumn(rng.integers(0, P, size=n + k, dtype=np.uint32)) for _ in range(2)]
    kid = compile_words(words, 2, 1)
    outs = []
    for run in (lambda ptrs: call_interpreter(words, [c.ptr + 4 * k for c in dcols], log, ptrs),
                lambda ptrs: call_native(kid, [c.ptr + 4 * k for c in dcols], log, ptrs)):
        out = HipColumn.zeros(n + k)
        run([out.ptr + 4 * k])
        outs.append(out.to_numpy())
    assert np.array_equal(outs[0], outs[1])
    assert outs[1][k:].any() and (outs[1][k:] < P).all() and not outs[1][:k].any()


# ------------------------------------------------------------------ argument errors, kinds and ids
LOAD2 = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)


def store(k, reg=0):
    return X.encode(STORE, 0, reg, k)


OK_WORDS = LOAD2 + store(0) + store(1, 1)                # 2 columns, 2 outputs: out0 = a, out1 = b one row further
ACC_WORDS = X.encode(X.LOAD, 0, 0, -1) + X.encode(X.LOAD, 1, 1, 1) + X.encode(X.MUL, 0, 0, 1) + X.encode(X.ACC, 0, 0)


def _small_io(n=16):
    a, b = HipColumn(np.arange(n, dtype=np.uint32)), HipColumn(np.arange(n, dtype=np.uint32) + 5)
    return a, b, HipColumn.zeros(n), HipColumn.zeros(n)


def test_argument_errors():
    a, b, o0, o1 = _small_io()
    kid = compile_words(OK_WORDS, 2, 2)
    cases = [
        ("air columns: log_size out of range", [a, b], 0, [o0, o1]),
        ("air columns: log_size out of range", [a, b], 29, [o0, o1]),
        ("air columns: number of columns out of range", [], 4, [o0, o1]),
        ("air columns: number of outputs out of range", [a, b], 4, []),
        ("air columns: number of outputs out of range", [a, b], 4, [o0] * 65),
        ("null device pointer in table", [a, None], 4, [o0, o1]),
        ("null device pointer in table", [a, b], 4, [o0, None]),
        ("air columns: an output column is also an input column", [a, b], 4, [o0, b]),
        ("air columns: two outputs are the same column", [a, b], 4, [o0, o0]),
        ("air kernel: compiled for another number of columns", [a, b, a], 4, [o0, o1]),
        ("air kernel: compiled for another number of columns", [a], 4, [o0, o1]),
        ("air kernel: compiled for another number of outputs", [a, b], 4, [o0]),
    ]
    for text, cols, log, outs in cases:
        with pytest.raises(L.TstwoError) as e:
            call_native(kid, [c.ptr if c is not None else None for c in cols], log, [c.ptr if c is not None else None for c in outs])
        assert str(e.value) == text and e.value.code == BAD_ARG, (text, str(e.value))
    call_native(kid, [a.ptr, b.ptr], 4, [o0.ptr, o1.ptr])                 # and the same arguments without a mistake pass
    assert np.array_equal(o0.to_numpy(), a.to_numpy())
    assert np.array_equal(o1.to_numpy(), b.to_numpy()[X.neighbour_map(4, 4, 1)])


def test_compile_refuses_what_the_interpreter_refuses():
    kid = C.c_uint64(0)
    bad = [
        ("air columns: bad opcode", 2, 1, LOAD2 + X.encode(X.ACC, 0, 0)),
        ("air columns: bad opcode", 2, 1, LOAD2 + X.encode(9, 0, 0) + store(0)),
        ("air columns: output index out of range", 2, 2, LOAD2 + store(0) + store(2, 1)),
        ("air columns: output stored twice", 2, 2, LOAD2 + store(0) + store(0, 1)),
        ("air columns: an output is never stored", 2, 2, LOAD2 + store(1)),
        ("air columns: register out of range or read before written", 2, 1, LOAD2 + store(0, 2)),
        ("air columns: column out of range", 2, 1, X.encode(X.LOAD, 0, 2, 0) + store(0)),
        ("air columns: row offset beyond the limit", 2, 1, X.encode(X.LOAD, 0, 0, 65) + store(0)),
        ("air columns: constant out of range", 2, 1, X.encode(X.CONST, 0, 0, P) + store(0)),
        ("air columns: number of columns out of range", 0, 1, LOAD2 + store(0)),
        ("air columns: number of outputs out of range", 2, 65, LOAD2 + store(0)),
    ]
    for text, n_cols, n_out, words in bad:
        with pytest.raises(L.TstwoError) as e:
            L.call("tstwo_air_columns_compile", L.u32x(words), len(words) // 2, n_cols, n_out, C.byref(kid))
        assert str(e.value) == text and e.value.code == BAD_ARG and kid.value == 0, (text, str(e.value))
    with pytest.raises(L.TstwoError, match="air columns: program length out of range"):
        L.call("tstwo_air_columns_compile", L.u32x(OK_WORDS), 0, 2, 2, C.byref(kid))
    # the constraint compiler keeps refusing STORE
    with pytest.raises(L.TstwoError) as e:
        L.call("tstwo_air_program_compile", L.u32x(OK_WORDS), len(OK_WORDS) // 2, 2, 2, C.byref(kid))
    assert str(e.value) == "air program: bad opcode" and kid.value == 0


def test_a_kernel_of_the_other_kind_is_refused():
    a, b, o0, o1 = _small_io(64)
    acc = [HipColumn.zeros(64) for _ in range(4)]
    columns = compile_words(OK_WORDS, 2, 2)
    constraint = C.c_uint64(0)
    L.call("tstwo_air_program_compile", L.u32x(ACC_WORDS), len(ACC_WORDS) // 2, 2, 1, C.byref(constraint))
    try:
        assert constraint.value != columns                       # one table, one counter
        with pytest.raises(L.TstwoError) as e:
            call_native(constraint.value, [a.ptr, b.ptr], 6, [o0.ptr, o1.ptr])
        assert str(e.value) == "air columns: the kernel was compiled from a constraint program" and e.value.code == BAD_ARG
        with pytest.raises(L.TstwoError) as e:
            L.call("tstwo_air_eval_compiled", columns, L.ptr_array([a.ptr, b.ptr]), 2, 4, 2, L.u32x([1, 0, 0, 0]), 1,
                   L.u32x([int(d) for d in M.denom_inv(4, 6)]), L.p4([c.ptr for c in acc]))
        assert str(e.value) == "air program: the kernel was compiled from a columns program" and e.value.code == BAD_ARG
        assert not o0.to_numpy().any() and not any(c.to_numpy().any() for c in acc)          # nothing ran
        # tstwo_air_kernel_info serves both kinds
        assert kernel_info(columns)[6] > 0 and kernel_info(constraint.value)[6] > 0
    finally:
        L.call("tstwo_air_program_destroy", constraint.value)


def test_unknown_and_destroyed_ids_are_refused():
    a, b, o0, o1 = _small_io()
    fresh = compile_raw(OK_WORDS, 2, 2)
    call_native(fresh, [a.ptr, b.ptr], 4, [o0.ptr, o1.ptr])
    L.call("tstwo_air_program_destroy", fresh)
    for kid in (0, fresh, fresh + 1000, (1 << 64) - 1):
        for call in (lambda: call_native(kid, [a.ptr, b.ptr], 4, [o0.ptr, o1.ptr]), lambda: kernel_info(kid),
                     lambda: L.call("tstwo_air_program_destroy", kid)):
            with pytest.raises(L.TstwoError, match="unknown air kernel") as e:
                call()
            assert e.value.code == BAD_ARG
    again = compile_raw(OK_WORDS, 2, 2)
    assert again != fresh                                   # an id is handed out once
    L.call("tstwo_air_program_destroy", again)


def test_ids_from_before_a_shutdown_are_unknown():
    """tstwo_shutdown unloads every kernel; in a process of its own, because it also frees every device buffer of the process"""
    code = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
        import ctypes as C
        import numpy as np
        from tstwo_amd import _lib as L
        from tstwo_amd import constraint_framework as F
        from tstwo_amd.backend import HipColumn
        L.init(0)
        program = F.Program({OK_WORDS!r}, 2, 2, 2)
        old = F.compile_columns_native(program, 2)
        assert F.compile_columns_native(program, 2) is old      # cached
        assert old.n_out == 2 and old.n_cols == 2
        L.call("tstwo_shutdown")
        L.init(0)
        a, b, o0, o1 = (HipColumn(np.arange(16, dtype=np.uint32) + k) for k in range(4))
        try:
            L.call("tstwo_air_eval_columns_compiled", old.id, L.ptr_array([a.ptr, b.ptr]), 2, 4, L.ptr_array([o0.ptr, o1.ptr]), 2)
            raise SystemExit("a kernel id survived tstwo_shutdown")
        except L.TstwoError as e:
            assert e.code == 7 and "unknown air kernel" in str(e), e
        out = F.evaluate_columns([a, b], 4, program, 2, native=True)           # the cache notices
        new = F.compile_columns_native(program, 2)
        assert new is not old and new.id != old.id
        assert new.info()["w4"]["private_bytes"] == 0 and new.info()["w1"]["private_bytes"] == 0
        assert np.array_equal(out[0].to_numpy(), a.to_numpy())
        print("shutdown ok")
    """)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "shutdown ok" in p.stdout, p.stderr[-2000:]


# ------------------------------------------------------------------ graph capture
def _end_capture():
    h = C.c_void_p()
    try:
        L.call("tstwo_graph_end_capture", C.byref(h))
    except L.TstwoError:
        pass
    return h


def test_one_launch_is_captured_and_replayed_on_other_data():
    """The entry uploads nothing, so with at most 64 input columns it is recorded; the graph then serves whatever the columns hold."""
    log, n_cols, n_out = 9, 3, 2
    n = 1 << log
    words = random_columns_program(np.random.default_rng(81), n_cols, n_out, 24)
    kid = compile_words(words, n_cols, n_out)
    rng = np.random.default_rng(82)
    data = [[rng.integers(0, P, size=n, dtype=np.uint32) for _ in range(n_cols)] for _ in range(2)]
    cols = [HipColumn(c) for c in data[0]]
    staged = [HipColumn(c) for c in data[1]]
    outs = [HipColumn.zeros(n) for _ in range(n_out)]
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        call_native(kid, [c.ptr for c in cols], log, [o.ptr for o in outs])
    finally:
        h = _end_capture()
    assert h.value
    try:
        L.sync()
        assert not any(o.to_numpy().any() for o in outs)            # recorded, not run
        for step in range(2):
            if step:                                                # rewrite the inputs, on the stream
                for c, s in zip(cols, staged):
                    L.call("tstwo_copy", C.c_void_p(c.ptr), C.c_void_p(s.ptr), 4 * n)
            L.call("tstwo_graph_launch", h)
            want = CM.run_columns(words, [c.astype(np.uint64) for c in data[step]], log, n_out)
            for k in range(n_out):
                assert np.array_equal(outs[k].to_numpy(), want[k].astype(np.uint32)), (step, k)
    finally:
        L.call("tstwo_graph_destroy", h)


def test_65_columns_and_compile_are_refused_during_capture():
    log, n_cols = 4, 65
    words = random_columns_program(np.random.default_rng(45), n_cols, 3, 120)       # the program of test_65_input_columns
    words[0] = (words[0] & 0xffff) | (64 << 16)
    kid = compile_words(words, n_cols, 3)
    rng = np.random.default_rng(83)
    data = [rng.integers(0, P, size=1 << log, dtype=np.uint32) for _ in range(n_cols)]
    cols, outs = [HipColumn(c) for c in data], [HipColumn.zeros(1 << log) for _ in range(3)]
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="host-array upload during graph capture \\(column tables beyond 64 pointers") as e:
            call_native(kid, [c.ptr for c in cols], log, [o.ptr for o in outs])
        assert e.value.code == BAD_ARG
        with pytest.raises(L.TstwoError, match="air columns compile: refused during graph capture"):
            L.call("tstwo_air_columns_compile", L.u32x(OK_WORDS), len(OK_WORDS) // 2, 2, 2, C.byref(C.c_uint64(0)))
    finally:
        h = _end_capture()
        if h.value:
            L.call("tstwo_graph_destroy", h)
    call_native(kid, [c.ptr for c in cols], log, [o.ptr for o in outs])         # outside a capture the same call runs
    want = CM.run_columns(words, [c.astype(np.uint64) for c in data], log, 3)
    for k in range(3):
        assert np.array_equal(outs[k].to_numpy(), want[k].astype(np.uint32)), k


# ------------------------------------------------------------------ a call sequence behind a plug
def _columns_op(s, cols, log, n_out, n_ops, seed, native):
    """The op of tests/sequence.py for either entry: a random program over `cols` into n_out new buffers."""
    rng = np.random.default_rng(9500 + seed)
    words = random_columns_program(rng, len(cols), n_out, n_ops)
    outs = [s.buf(1 << log, kind="m31") for _ in range(n_out)]
    model = lambda S: dict(zip(outs, CM.run_columns(words, [S[c].astype(np.uint64) for c in cols], log, n_out)))
    if native:
        kid = compile_words(words, len(cols), n_out)
        s.add(SQ.Op("tstwo_air_eval_columns_compiled", cols, outs,
                    lambda A: SQ._call("tstwo_air_eval_columns_compiled", kid, SQ._ptrs(A, cols), len(cols), log, SQ._ptrs(A, outs), n_out),
                    model, capturable=len(cols) <= 64))
    else:
        s.add(SQ.Op("tstwo_air_eval_columns", cols, outs,
                    lambda A: SQ._call("tstwo_air_eval_columns", SQ._ptrs(A, cols), len(cols), log, L.u32x(words), len(words) // 2,
                                       SQ._ptrs(A, outs), n_out),
                    model, capturable=False, scratch="air columns program"))
    return outs


def test_compiled_columns_then_logup_then_interpreted_columns_behind_a_plug():
    """tstwo_air_eval_columns_compiled -> tstwo_logup_column on its outputs -> tstwo_air_eval_columns over everything, enqueued back
    to back behind the plug with no synchronisation: the compiled call touches neither the upload ring nor the scratch block the
    other two stage through, and every buffer is checked against chained references."""
    log = 9
    s = SQ.Seq()
    cols = SQ.rand_cols(s, np.random.default_rng(78), 4, 1 << log)
    first = _columns_op(s, cols, log, 3, 20, seed=1, native=True)
    logup = SQ.logup_column(s, [(first[:2], first[2]), ([cols[0]], None)], None, log, seed=1)
    _columns_op(s, cols + first + logup, log, 5, 60, seed=2, native=False)
    assert [op.entry for op in s.ops] == ["tstwo_air_eval_columns_compiled", "tstwo_logup_column", "tstwo_air_eval_columns"]
    plug = SQ.Plug()
    try:
        plug.enqueue(); plug.host_done(); L.sync()         # once unchecked: the first launches load the transform's code objects
        _, ratio = SQ.run(s, plug)
        print(f"plug ratio {ratio:.1f}")
        L.call("tstwo_check_zero_flag")
    finally:
        L.sync()
        plug.free()

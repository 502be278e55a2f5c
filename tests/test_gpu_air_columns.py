"""tstwo_air_eval_columns on the MI355X: bit for bit against the integer model (tests/columns_model.py run_columns, whose row
neighbours come from the geometry) on random straight-line programs, with every device argument inside a guarded arena
(tests/arena.py: nothing written outside the n_out outputs, nothing into the inputs); its argument errors, each with its text;
and one call sequence behind a plug (tests/sequence.py) with tstwo_logup_column between two calls, which all stage through the
upload ring into the scratch block.

Shapes: log 1 and 2 (one row per lane; the bit reversal over 0 and 1 bits), log 3 (four rows per lane, two lanes), log 8 (exactly
one wave of four-row lanes), log 9 (two workgroups), log 12 with every column one word off a 16-byte boundary (one row per lane
at a size that would vectorise), log 22 (above the grid cap of 32 workgroups per CU on a 256-CU part: the kernel strides);
programs of 1 and of 32 registers; 1 and 64 outputs; 65 input columns (the column table in device memory)."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import P

pytestmark = pytest.mark.gpu

import air_plan as AP  # noqa: E402
import air_program_model as X  # noqa: E402
import columns_model as CM  # noqa: E402
import sequence as SQ  # noqa: E402
from arena import Arena, rin, rout  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd.backend import HipColumn  # noqa: E402

PLACEMENTS = ("aligned", "all+4", "out+4", "in+4")


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def random_columns_program(rng, n_cols, n_out, n_ops, max_regs=32, max_offset=3):
    words, k = CM.stores_for_accs(X.random_program(rng, n_cols, n_out, n_ops, max_regs=max_regs, max_offset=max_offset))
    assert k == n_out
    return words


def registers_written(words):
    return 1 + max((w >> 8) & 0xff for w in words[::2] if w & 0xff not in (X.ACC, CM.STORE))


def in_arena(words, cols, log, n_out, place="aligned"):
    """One call with every column in a guarded arena; returns the outputs after the guards and the inputs were checked."""
    c_, o_ = [f"col{i}" for i in range(len(cols))], [f"out{k}" for k in range(n_out)]
    off = {x: 0 for x in c_ + o_}
    if place == "all+4":
        off = {x: 4 for x in off}
    elif place == "out+4":
        off.update({x: 4 for x in o_})
    elif place == "in+4":
        off[c_[0]] = 4
    regs = [rin(x, c.astype(np.uint32), off[x]) for x, c in zip(c_, cols)] + [rout(x, 1 << log, off[x]) for x in o_]
    with Arena(regs) as A:
        L.call("tstwo_air_eval_columns", A.ptrs(c_), len(cols), log, L.u32x(words), len(words) // 2, A.ptrs(o_), n_out)
        got = A.check()
    return [got[x] for x in o_]


def check_case(seed, log, n_cols, n_out, n_ops, max_regs=32, max_offset=3, place="aligned", first_load=None):
    """first_load: the column the program's first LOAD is made to read."""
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(n_cols)]
    words = random_columns_program(rng, n_cols, n_out, n_ops, max_regs, max_offset)
    if first_load is not None:
        assert words[0] & 0xff == X.LOAD
        words[0] = (words[0] & 0xffff) | (first_load << 16)
    got = in_arena(words, cols, log, n_out, place)
    want = CM.run_columns(words, cols, log, n_out)
    for k in range(n_out):
        assert np.array_equal(got[k], want[k]), f"output {k}"
    return words


# (id, log, input columns, outputs, operations, place)
SHAPES = [("log1", 1, 3, 2, 24, "aligned"), ("log2", 2, 3, 2, 24, "aligned"), ("log3", 3, 4, 3, 30, "aligned"),
          ("log8", 8, 6, 5, 40, "aligned"), ("log9", 9, 6, 5, 40, "aligned"), ("log12-off-by-a-word", 12, 4, 3, 30, "all+4")]


@pytest.mark.parametrize("name,log,n_cols,n_out,n_ops,place", SHAPES, ids=[s[0] for s in SHAPES])
def test_random_programs_match_the_model(name, log, n_cols, n_out, n_ops, place):
    words = check_case(500 + log, log, n_cols, n_out, n_ops, place=place)
    assert any(w & 0xff == X.LOAD and words[2 * i + 1] != 0 for i, w in enumerate(words[::2])), "no load at an offset"


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
    check_case(45, 4, 65, 3, 120, first_load=64)


@pytest.mark.parametrize("log", [4, 9])
@pytest.mark.parametrize("offset", [64, -64])
def test_the_largest_offsets(log, offset):
    """+-64 rows: within the trace at log 9, four whole turns at log 4."""
    rng = np.random.default_rng(46 + log)
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(2)]
    words = (X.encode(X.LOAD, 0, 0, offset) + X.encode(X.LOAD, 1, 1, -offset) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.LOAD, 3, 1, 0)
             + X.encode(X.SUB, 2, 2, 3) + X.encode(CM.STORE, 0, 2, 1) + X.encode(CM.STORE, 0, 0, 0))
    got = in_arena(words, cols, log, 2)
    want = CM.run_columns(words, cols, log, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    nb = X.neighbour_map(log, log, offset)
    assert np.array_equal(want[0], cols[0][nb])


def test_above_the_grid_cap():
    """The smallest log whose rows, in fours, the grid does not cover (tests/air_plan.py, for this part's CUs): on a 256-CU part
    2^22 rows, 2^20 lanes, 16384 one-wave workgroups, twice the grid."""
    n_cus = int(re.search(r"(\d+) CUs", L.device_name()).group(1))
    log = AP.first_striding_log("eval_columns", 4, n_cus)
    shape = AP.Input("eval_columns", 0, log, 0, 2, 1, 7, 3, True, n_cus)
    assert AP.plan(shape).w == 4 and AP.strides(shape) and not AP.strides(shape._replace(log=log - 1))
    rng = np.random.default_rng(47)
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint32) for _ in range(2)]
    words = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, -1) + X.encode(X.MUL, 2, 0, 1) + X.encode(X.LOAD, 1, 0, 2)
             + X.encode(X.ADD, 2, 2, 1) + X.encode(X.NEG, 2, 2) + X.encode(CM.STORE, 0, 2, 0))
    dev = [HipColumn(c) for c in cols]
    out = HipColumn.uninitialized(1 << log)
    L.call("tstwo_air_eval_columns", L.ptr_array([c.ptr for c in dev]), 2, log, L.u32x(words), len(words) // 2, L.ptr_array([out.ptr]), 1)
    want, = CM.run_columns(words, cols, log, 1)
    assert np.array_equal(out.to_numpy(), want)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("log", [3, 9])
def test_nothing_is_written_outside_the_outputs(log, place):
    """The arena asserts the guard bands around every region and the input regions; the outputs are compared as well."""
    check_case(600 + log, log, 5, 4, 40, place=place)


# ------------------------------------------------------------------ argument errors
def _call(words, cols, log, outs):
    L.call("tstwo_air_eval_columns", L.ptr_array([c.ptr for c in cols]), len(cols), log, L.u32x(words), len(words) // 2,
           L.ptr_array([c.ptr for c in outs]), len(outs))


def test_argument_errors():
    n = 16
    a, b = HipColumn(np.arange(n, dtype=np.uint32)), HipColumn(np.arange(n, dtype=np.uint32) + 5)
    o0, o1 = HipColumn.zeros(n), HipColumn.zeros(n)
    load = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)
    store = lambda k, reg=0: X.encode(CM.STORE, 0, reg, k)
    cases = [
        ("air columns: bad opcode", load + X.encode(X.ACC, 0, 0), [a, b], 4, [o0]),
        ("air columns: bad opcode", load + X.encode(9, 0, 0) + store(0), [a, b], 4, [o0]),
        ("air columns: output index out of range", load + store(0) + store(2, 1), [a, b], 4, [o0, o1]),
        ("air columns: output stored twice", load + store(0) + store(0, 1), [a, b], 4, [o0, o1]),
        ("air columns: an output is never stored", load + store(1), [a, b], 4, [o0, o1]),
        ("air columns: an output column is also an input column", load + store(0), [a, b], 4, [b]),
        ("air columns: two outputs are the same column", load + store(0) + store(1), [a, b], 4, [o0, o0]),
        ("air columns: log_size out of range", load + store(0), [a, b], 0, [o0]),
        ("air columns: log_size out of range", load + store(0), [a, b], 29, [o0]),
        ("air columns: register out of range or read before written", load + store(0, 2), [a, b], 4, [o0]),
        ("air columns: column out of range", X.encode(X.LOAD, 0, 2, 0) + store(0), [a, b], 4, [o0]),
        ("air columns: row offset beyond the limit", X.encode(X.LOAD, 0, 0, 65) + store(0), [a, b], 4, [o0]),
        ("air columns: constant out of range", X.encode(X.CONST, 0, 0, P) + store(0), [a, b], 4, [o0]),
    ]
    for text, words, cols, log, outs in cases:
        with pytest.raises(L.TstwoError, match=text) as e:
            _call(words, cols, log, outs)
        assert str(e.value) == text
    with pytest.raises(L.TstwoError, match="air columns: number of outputs out of range"):
        L.call("tstwo_air_eval_columns", L.ptr_array([a.ptr]), 1, 4, L.u32x(load), 1, L.ptr_array([o0.ptr] * 65), 65)
    with pytest.raises(L.TstwoError, match="air columns: number of outputs out of range"):
        L.call("tstwo_air_eval_columns", L.ptr_array([a.ptr]), 1, 4, L.u32x(load), 1, L.ptr_array([]), 0)
    with pytest.raises(L.TstwoError, match="null device pointer in table"):
        L.call("tstwo_air_eval_columns", L.ptr_array([a.ptr]), 1, 4, L.u32x(load), 1, L.ptr_array([None]), 1)
    _call(load + store(0) + store(1, 1), [a, b], 4, [o0, o1])             # and the same arguments without a mistake pass
    assert np.array_equal(o0.to_numpy(), a.to_numpy())


def test_store_stays_a_bad_opcode_of_the_constraint_program():
    n = 32
    cols = [HipColumn(np.arange(n, dtype=np.uint32))]
    acc = [HipColumn.zeros(n) for _ in range(4)]
    words = X.encode(X.LOAD, 0, 0, 0) + X.encode(CM.STORE, 0, 0, 0)
    with pytest.raises(L.TstwoError, match="air program: bad opcode"):
        L.call("tstwo_air_eval_program", L.ptr_array([c.ptr for c in cols]), 1, 4, 1, L.u32x(words), 2, L.u32x([1, 0, 0, 0]), 1,
               L.u32x([1, 1]), L.p4([c.ptr for c in acc]))


def test_refused_during_graph_capture():
    n = 64
    a, out = HipColumn(np.arange(n, dtype=np.uint32)), HipColumn.zeros(n)
    words = X.encode(X.LOAD, 0, 0, 1) + X.encode(CM.STORE, 0, 0, 0)
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="host-array upload during graph capture"):
            _call(words, [a], 6, [out])
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)
    _call(words, [a], 6, [out])
    assert np.array_equal(out.to_numpy(), a.to_numpy()[X.neighbour_map(6, 6, 1)])


# ------------------------------------------------------------------ a call sequence behind a plug
def air_eval_columns(s, cols, log, n_out, n_ops, seed):
    """The op of tests/sequence.py for tstwo_air_eval_columns: a random program over `cols` into n_out new buffers."""
    rng = np.random.default_rng(9400 + seed)
    words = random_columns_program(rng, len(cols), n_out, n_ops)
    outs = [s.buf(1 << log, kind="m31") for _ in range(n_out)]
    model = lambda S: dict(zip(outs, CM.run_columns(words, [S[c].astype(np.uint64) for c in cols], log, n_out)))
    s.add(SQ.Op("tstwo_air_eval_columns", cols, outs,
                lambda A: SQ._call("tstwo_air_eval_columns", SQ._ptrs(A, cols), len(cols), log, L.u32x(words), len(words) // 2,
                                   SQ._ptrs(A, outs), n_out),
                model, capturable=False, scratch="air columns program"))
    return outs


def test_columns_then_logup_then_columns_behind_a_plug():
    """tstwo_air_eval_columns -> tstwo_logup_column on its outputs -> tstwo_air_eval_columns with another, longer program, enqueued
    back to back behind the plug with no synchronisation: each stages through the upload ring into the same scratch words, so a
    program overwritten before its kernel ran, or read before its upload landed, is a wrong word in some buffer."""
    log = 9
    s = SQ.Seq()
    cols = SQ.rand_cols(s, np.random.default_rng(77), 4, 1 << log)
    first = air_eval_columns(s, cols, log, 3, 20, seed=1)
    logup = SQ.logup_column(s, [(first[:2], first[2]), ([cols[0]], None)], None, log, seed=1)
    air_eval_columns(s, cols + first + logup, log, 5, 60, seed=2)
    assert [op.entry for op in s.ops] == ["tstwo_air_eval_columns", "tstwo_logup_column", "tstwo_air_eval_columns"]
    plug = SQ.Plug()
    try:
        plug.enqueue(); plug.host_done(); L.sync()         # once unchecked: the first launches load the transform's code objects
        _, ratio = SQ.run(s, plug)
        print(f"plug ratio {ratio:.1f}")
        L.call("tstwo_check_zero_flag")
    finally:
        L.sync()
        plug.free()

"""tstwo_air_check_constraints on the MI355X: per constraint the number of rows on which it is non-zero and the first of them in
coset order, bit for bit against the integer model (tests/air_check_model.py).  Every device argument of a model comparison lies
in a guarded arena (tests/arena.py): the report between sentinel bands, the columns as inputs.

Clean traces of every example eval through FrameworkComponent.constraint_failures (the wrap-around rows and the claimed_sum
constraint); random programs grouped 1 / 4 / mixed on dense and on sparse columns at log 1 and 2 (fewer rows than one four-row
lane), 5 (half a wave of one-row lanes), 8 and 9 (one and two workgroups of four-row lanes) and 10 one word off a 16-byte
boundary (the one-row kernel); the grid-stride wrap; changed cells at the row edges of a lane and of a wave; grouping; a column
word 2^31 - 1; two calls behind a plug; the refusals."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import P

pytestmark = pytest.mark.gpu

import air_check_model as CK  # noqa: E402
import air_plan as AP  # noqa: E402
import air_program_model as X  # noqa: E402
import interaction_evals as E  # noqa: E402
import logup_model as LM  # noqa: E402
import sequence as SQ  # noqa: E402
from arena import SENTINEL, Arena, rin, rout  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import air as A  # noqa: E402
from tstwo_amd import constraint_framework as F  # noqa: E402
from tstwo_amd import logup as LG  # noqa: E402
from tstwo_amd.backend import HipColumn  # noqa: E402

ENTRY = "tstwo_air_check_constraints"
LE = E.elements()
STORE = 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def in_arena(words, cols, log, groups, place="aligned"):
    """One call with the columns and the report in a guarded arena; the report after guards and inputs were checked."""
    names = [f"col{i}" for i in range(len(cols))]
    off = 4 if place == "all+4" else 0
    n_constraints = groups[-1] + 1
    regs = [rin(x, np.asarray(c).astype(np.uint32), off) for x, c in zip(names, cols)] + [rout("report", 2 * n_constraints)]
    words = CK.with_groups(words, groups)
    with Arena(regs) as ar:
        L.call(ENTRY, ar.ptrs(names), len(cols), log, L.u32x(words), len(words) // 2, n_constraints, ar.ptr("report"))
        got = ar.check()
    return got["report"]


def against_model(words, cols, log, groups, place="aligned"):
    want = CK.report_words(words, cols, log, groups)
    got = in_arena(words, cols, log, groups, place)
    assert np.array_equal(got, want), (list(got), list(want))
    return CK.report(words, cols, log, groups)


# ------------------------------------------------------------------ clean traces of the example evals
def _clean(monkeypatch, comp, main, pre=(), inter=()):
    """constraint_failures finds nothing, and the report it read says so constraint by constraint."""
    seen = []
    real = F.check_program

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(F, "check_program", spy)
    assert comp.constraint_failures(main, pre, inter) == []
    assert comp.assert_constraints(main, pre, inter) is None
    assert seen[0] == [(0, None)] * comp.n_constraints and comp.n_constraints > 0
    raw = HipColumn.uninitialized(2 * comp.n_constraints)          # and the words themselves: 0 and 0xffffffff
    cols = [F._trace_column(c) for c in list(main) + list(pre) + list(inter)]
    prog = comp._constraint_program()
    groups = [c for c, s in enumerate(comp.secure_flags) for _ in range(4 if s else 1)]
    words = CK.with_groups(prog.words, groups)
    L.call(ENTRY, L.ptr_array([c.ptr for c in cols]), len(cols), comp.log_size, L.u32x(words), prog.n_instr, comp.n_constraints, L.vp(raw.ptr))
    assert raw.to_numpy().tolist() == [0, 0xffffffff] * comp.n_constraints


def test_clean_wide_fibonacci(monkeypatch):
    log, n = 8, 20
    rng = np.random.default_rng(1)
    comp = F.WideFibonacciComponent(log, n)
    assert comp.program is None
    _clean(monkeypatch, comp, A.generate_wide_fib_trace(log, rng.integers(0, P, size=1 << log), rng.integers(0, P, size=1 << log), n))
    assert comp.program is None and comp._check_program.n_constraints == n - 2          # proving still takes the hand-written kernel


def test_clean_mul_add(monkeypatch):
    log = 6
    rng = np.random.default_rng(2)
    x0, x1 = (rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(2))
    _clean(monkeypatch, F.MulAddComponent(log), [x0, x1, (x0 * x1 + x0) % P])


def test_clean_fibonacci_rows(monkeypatch):
    log = 6
    comp = F.FrameworkComponent(F.FibonacciRowsEval(log, 3, 5), None, [0])
    _clean(monkeypatch, comp, F.fibonacci_rows_trace(log, 3, 5), [F.is_first_column(log)])


def test_clean_permutation(monkeypatch):
    log = 6
    rng = np.random.default_rng(3)
    a = rng.integers(0, P, size=1 << log, dtype=np.uint32)
    b = rng.permutation(a)
    inter, claimed = F.permutation_interaction_trace(log, a, b, LE)
    _clean(monkeypatch, F.FrameworkComponent(F.PermutationEval(log, LE), claimed_sum=claimed), [a, b], (), inter)


def test_clean_range_check_table_and_values(monkeypatch):
    log_range, log_values = 6, 7
    rng = np.random.default_rng(4)
    v0, v1 = (rng.integers(0, 1 << log_range, size=1 << log_values).astype(np.uint32) for _ in range(2))
    mult = F.range_check_multiplicities(log_range, v0, v1)
    t_inter, t_sum = F.range_check_table_interaction_trace(log_range, mult, LE)
    v_inter, v_sum = F.range_check_values_interaction_trace(log_values, v0, v1, LE)
    _clean(monkeypatch, F.FrameworkComponent(F.RangeCheckTableEval(log_range, LE), None, [0], claimed_sum=t_sum), [mult],
           [F.range_check_table_column(log_range)], t_inter)
    _clean(monkeypatch, F.FrameworkComponent(F.RangeCheckValuesEval(log_values, LE), claimed_sum=v_sum), [v0, v1], (), v_inter)


def test_clean_state_machine(monkeypatch):
    log = 6
    x, y = F.state_machine_trace(log, P - 5, 77)
    inter, claimed = LG.derive_interaction_trace(F.StateMachineEval(log, LE), [x, y])
    _clean(monkeypatch, F.FrameworkComponent(F.StateMachineEval(log, LE), claimed_sum=claimed), [x, y], (), inter)


def test_clean_xor_table_and_values(monkeypatch):
    log_bits, log_rows = 3, 7
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 1 << log_bits, size=1 << log_rows, dtype=np.uint32) for _ in range(2))
    enabler = rng.integers(0, 2, size=1 << log_rows, dtype=np.uint32)
    a, b, c, enabler = (HipColumn(x) for x in (a, b, a ^ b, enabler))
    mult = F.xor_multiplicities_device(log_bits, a, b, enabler)
    table = [HipColumn(t) for t in F.xor_table_columns(log_bits)]
    t_inter, t_sum = LG.derive_interaction_trace(F.XorTableEval(log_bits, LE), [mult], table)
    v_inter, v_sum = LG.derive_interaction_trace(F.XorValuesEval(log_rows, LE), [a, b, c, enabler])
    _clean(monkeypatch, F.FrameworkComponent(F.XorTableEval(log_bits, LE), None, [0, 1, 2], claimed_sum=t_sum), [mult], table, t_inter)
    _clean(monkeypatch, F.FrameworkComponent(F.XorValuesEval(log_rows, LE), claimed_sum=v_sum), [a, b, c, enabler], (), v_inter)


def test_a_broken_trace_is_named_by_constraint_and_row():
    """constraint_failures and assert_constraints on a wide Fibonacci trace with cell (column 5, coset row 77) changed"""
    from tstwo_amd.prover import ConstraintsNotSatisfied, ConstraintViolation
    log, n = 8, 10
    rng = np.random.default_rng(6)
    trace = [e.values.to_numpy() for e in A.generate_wide_fib_trace(log, rng.integers(1, P, size=1 << log), rng.integers(1, P, size=1 << log), n)]
    pos = int(LM.positions(log)[77])
    trace[5][pos] = (int(trace[5][pos]) + 1) % P
    comp = F.WideFibonacciComponent(log, n)
    assert comp.constraint_failures(trace) == [(3, 1, 77), (4, 1, 77), (5, 1, 77)]
    with pytest.raises(ConstraintViolation) as e:
        comp.assert_constraints(trace)
    v = e.value
    assert isinstance(v, ConstraintsNotSatisfied) and (v.component, v.constraint, v.row, v.n_rows) == (None, 3, 77, 1)
    assert v.failures == [(3, 1, 77), (4, 1, 77), (5, 1, 77)]
    assert str(v) == "constraint 3 is non-zero on 1 of 256 rows, first at row 77"
    with pytest.raises(ValueError, match="the component reads 10 main, 0 preprocessed and 0 interaction columns"):
        comp.constraint_failures(trace[:9])


# ------------------------------------------------------------------ random programs against the model
N_ACC = 8
GROUPINGS = {"one": CK.grouping([1] * N_ACC), "four": CK.grouping([4, 4]), "mixed": CK.grouping([1, 4, 1, 2])}
# (id, log, columns, operations, place)
SHAPES = [("log1", 1, 3, 24, "aligned"), ("log2", 2, 3, 24, "aligned"), ("log5", 5, 4, 30, "aligned"), ("log8", 8, 6, 40, "aligned"),
          ("log9", 9, 6, 40, "aligned"), ("log10-off-by-a-word", 10, 4, 30, "all+4")]


def _columns(rng, n_cols, log, fill):
    cols = [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(n_cols)]
    if fill == "sparse":                    # zero except a few rows
        keep = np.zeros(1 << log, dtype=bool)
        keep[rng.choice(1 << log, size=min(3, 1 << log), replace=False)] = True
        cols = [np.where(keep, c, 0) for c in cols]
    return cols


@pytest.mark.parametrize("fill", ["dense", "sparse"])
@pytest.mark.parametrize("grouping", list(GROUPINGS))
@pytest.mark.parametrize("name,log,n_cols,n_ops,place", SHAPES, ids=[s[0] for s in SHAPES])
def test_random_programs_match_the_model(name, log, n_cols, n_ops, place, grouping, fill):
    rng = np.random.default_rng(700 + log)
    words = X.random_program(rng, n_cols, N_ACC, n_ops)
    assert any(w & 0xff == X.LOAD and words[2 * i + 1] != 0 for i, w in enumerate(words[::2])), "no load at an offset"
    rep = against_model(words, _columns(rng, n_cols, log, fill), log, GROUPINGS[grouping], place)
    print(name, grouping, fill, rep)
    if fill == "dense" and log >= 5:
        assert any(n > (1 << log) // 2 for n, _ in rep), "nearly every row should fail some constraint"


def test_sparse_counts_on_a_program_without_constants():
    """a program whose constraints vanish on zero rows: the counts are those of the few non-zero rows and their neighbours"""
    log = 9
    rng = np.random.default_rng(31)
    cols = _columns(rng, 3, log, "sparse")
    words = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, -1) + X.encode(X.MUL, 2, 0, 0) + X.encode(X.ACC, 0, 2) + X.encode(X.ACC, 0, 1)
             + X.encode(X.LOAD, 3, 2, 2) + X.encode(X.ADD, 3, 3, 1) + X.encode(X.ACC, 0, 3) + X.encode(X.NEG, 3, 0) + X.encode(X.ACC, 0, 3))
    for groups in ([0, 1, 2, 3], [0, 0, 1, 1], [0, 0, 0, 0]):
        rep = against_model(words, cols, log, groups)
        assert all(0 < n <= 12 for n, _ in rep), rep          # 3 rows, seen through at most 4 loads


def test_a_column_word_of_2_pow_31_minus_1_is_zero():
    """P is zero as a field element: a LOAD puts it into a register as it is, and the ACC reduces before it tests"""
    log = 8
    col = np.zeros(1 << log, dtype=np.uint64)
    col[::3] = P
    col[LM.positions(log)[200]] = 9
    words = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.ACC, 0, 0) + X.encode(X.LOAD, 1, 0, 1) + X.encode(X.ACC, 0, 1)
    assert against_model(words, [col], log, [0, 1]) == [(1, 200), (1, 199)]
    assert against_model(words, [col], log, [0, 0], "all+4") == [(2, 199)]


# ------------------------------------------------------------------ the grid-stride wrap
MUL_ADD = (X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 0) + X.encode(X.MUL, 1, 0, 1) + X.encode(X.ADD, 0, 0, 1) + X.encode(X.LOAD, 1, 2, 0)
           + X.encode(X.SUB, 0, 0, 1) + X.encode(X.ACC, 0, 0))


def n_cus():
    m = re.search(r"(\d+) CUs", L.device_name())
    assert m, L.device_name()
    return int(m.group(1))


def _raw_check(ptrs, log, words, n_constraints=1):
    report = HipColumn.uninitialized(2 * n_constraints)
    L.call(ENTRY, L.ptr_array(ptrs), len(ptrs), log, L.u32x(words), len(words) // 2, n_constraints, L.vp(report.ptr))
    return report.to_numpy().tolist()


@pytest.mark.parametrize("rows_per_lane,unaligned", [(1, True), (4, False)], ids=["one-row-unaligned", "four-rows-aligned"])
def test_above_the_grid_cap(rows_per_lane, unaligned):
    """The smallest log whose rows exceed what the launch's grid covers (tests/air_plan.py, for this part's CUs), so that every
    workgroup strides: log 20 at W = 1 and log 22 at W = 4 on a 256-CU part.  One changed cell in the last quarter of the rows
    (reached only by a workgroup's later iterations), then every row changed."""
    log = AP.first_striding_log("check", rows_per_lane, n_cus())
    shape = AP.Input("check", 0, log, 0, 3, 1, len(MUL_ADD) // 2, 2, not unaligned, n_cus())
    assert AP.plan(shape).w == rows_per_lane and AP.strides(shape) and not AP.strides(shape._replace(log=log - 1))
    n = 1 << log
    rng = np.random.default_rng(48)
    x0, x1 = (rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2))
    x2 = (x0 * x1 + x0) % P
    k = 3 * n // 4 + 12345
    pos = int(LM.positions(log)[k])
    bad = x2.copy()
    bad[pos] = (bad[pos] + 1) % P
    pad = 1 if unaligned else 0                                       # one word into the buffer: not 16-byte aligned
    bufs = [HipColumn(np.concatenate([np.zeros(pad, dtype=np.uint32), c.astype(np.uint32)])) for c in (x0, x1, x2, bad, (x2 + 1) % P)]
    p = [b.ptr + 4 * pad for b in bufs]
    assert _raw_check(p[:3], log, MUL_ADD) == [0, 0xffffffff]
    assert _raw_check([p[0], p[1], p[3]], log, MUL_ADD) == [1, k]
    assert _raw_check([p[0], p[1], p[4]], log, MUL_ADD) == [n, 0]


# ------------------------------------------------------------------ row edges
def _running_sum_trace(log, rng):
    """a[k + 1] = a[k] + b[k] in coset order, closing the circle; (a, b) in storage order"""
    n = 1 << log
    b_seq = rng.integers(0, P, size=n, dtype=np.uint64)
    b_seq[-1] = (P - int(b_seq[:-1].sum() % P)) % P
    a_seq = (7 + np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(b_seq[:-1])])) % P
    pos = LM.positions(log)
    a, b = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    a[pos], b[pos] = a_seq.astype(np.uint64), b_seq
    return a, b


RUNNING_SUM = (X.encode(X.LOAD, 0, 0, 1) + X.encode(X.LOAD, 1, 0, 0) + X.encode(X.SUB, 0, 0, 1) + X.encode(X.LOAD, 1, 1, 0)
               + X.encode(X.SUB, 0, 0, 1) + X.encode(X.ACC, 0, 0))


@pytest.mark.parametrize("place", ["aligned", "all+4"])
def test_changed_cells_at_the_row_edges(place):
    """a[k + 1] - a[k] - b[k] with one cell of `a` changed: coset rows 0, 1 and 2^log - 1, and the storage positions either side of
    a lane's four rows (3 / 4), of a wave of one-row lanes (63 / 64) and of a wave of four-row lanes (255 / 256).  Each breaks its
    own row and the row before it, across the wrap for row 0."""
    log = 10
    n = 1 << log
    a, b = _running_sum_trace(log, np.random.default_rng(49))
    assert against_model(RUNNING_SUM, [a, b], log, [0], place) == [(0, CK.NO_ROW)]
    pos, rows = LM.positions(log), CK.coset_rows(log)
    cells = [int(pos[k]) for k in (0, 1, n - 1)] + [3, 4, 63, 64, 255, 256, n - 1]
    for r in cells:
        bad = a.copy()
        bad[r] = (bad[r] + 1) % P
        k = int(rows[r])
        want = [(2, min(k, (k - 1) % n))]
        assert against_model(RUNNING_SUM, [bad, b], log, [0], place) == want, (r, k)


# ------------------------------------------------------------------ grouping
def test_a_secure_constraint_counts_a_row_once():
    """four ACCs, one constraint: a row on which only the last coordinate is non-zero counts once; two rows that fail in different
    coordinates count 2; a row that fails in two coordinates counts once"""
    log = 8
    pos = LM.positions(log)
    cols = [np.zeros(1 << log, dtype=np.uint64) for _ in range(4)]
    words = [w for i in range(4) for w in X.encode(X.LOAD, i, i, 0)] + [w for i in range(4) for w in X.encode(X.ACC, 0, i)]
    cols[3][pos[201]] = 5
    assert against_model(words, cols, log, [0, 0, 0, 0]) == [(1, 201)]
    cols[1][pos[17]] = 1
    assert against_model(words, cols, log, [0, 0, 0, 0]) == [(2, 17)]
    cols[0][pos[201]] = 7
    assert against_model(words, cols, log, [0, 0, 0, 0]) == [(2, 17)]
    assert against_model(words, cols, log, [0, 1, 2, 3]) == [(1, 201), (1, 17), (0, CK.NO_ROW), (1, 201)]
    assert against_model(words, cols, log, [0, 1, 1, 1], "all+4") == [(1, 201), (2, 17)]


def test_256_constraints():
    log = 6
    rng = np.random.default_rng(50)
    cols = _columns(rng, 2, log, "dense")
    words = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 3)
    for c in range(256):
        words += X.encode(X.CONST, 2, 0, int(cols[c % 2][c % 64])) + X.encode(X.SUB, 2, c % 2, 2) + X.encode(X.ACC, 0, 2)
    rep = against_model(words, cols, log, list(range(256)))
    assert all(n >= (1 << log) - 2 for n, _ in rep)


@pytest.mark.parametrize("place", ["aligned", "all+4"])
@pytest.mark.parametrize("n_regs", [1, 32])
def test_the_tally_behind_one_register_and_behind_32(n_regs, place):
    """REGISTER_CASES: the (count, first row) pairs lie in LDS directly behind the registers, at the smallest and at the largest
    register file, four rows per lane and one.  Constraint 0 is the sum of every register, constraint 1 a single one."""
    log = 5
    words = AP.register_program(n_regs, 3, [0, 1])
    assert 1 + max((w >> 8) & 0xff for w in words[::2] if w & 0xff != X.ACC) == n_regs
    cols = _columns(np.random.default_rng(51 + n_regs), 3, log, "sparse")
    rep = against_model(words, cols, log, [0, 1], place)
    assert all(0 < n < 1 << log for n, _ in rep), rep


# ------------------------------------------------------------------ two calls behind a plug
def air_check(s, cols, log, n_ops, groups, seed):
    """The op of tests/sequence.py for tstwo_air_check_constraints: a random program over `cols` into a new report buffer."""
    rng = np.random.default_rng(9500 + seed)
    words = CK.with_groups(X.random_program(rng, len(cols), len(groups), n_ops), groups)
    n_constraints = groups[-1] + 1
    report = s.buf(2 * n_constraints)
    model = lambda S: {report: CK.report_words(words, [S[c].astype(np.uint64) for c in cols], log, groups)}
    s.add(SQ.Op(ENTRY, cols, [report],
                lambda A_: SQ._call(ENTRY, SQ._ptrs(A_, cols), len(cols), log, L.u32x(words), len(words) // 2, n_constraints,
                                    C.c_void_p(A_(report))),
                model, capturable=False, scratch="air check program"))
    return report


def test_two_checks_behind_a_plug():
    """Two checks with different programs (the second longer) enqueued back to back behind the plug: both stage their program
    through the upload ring into the same scratch words, and the first report is read only after the second launch."""
    log = 9
    s = SQ.Seq()
    cols = SQ.rand_cols(s, np.random.default_rng(78), 4, 1 << log)
    air_check(s, cols, log, 20, CK.grouping([1, 1, 1]), seed=1)
    air_check(s, cols, log, 60, CK.grouping([1, 4, 2]), seed=2)
    assert [op.entry for op in s.ops] == [ENTRY, ENTRY]
    plug = SQ.Plug()
    try:
        plug.enqueue(); plug.host_done(); L.sync()         # once unchecked: the first launches load the transform's code objects
        _, ratio = SQ.run(s, plug)
        print(f"plug ratio {ratio:.1f}")
    finally:
        L.sync()
        plug.free()


# ------------------------------------------------------------------ refusals
def test_refusals_enqueue_nothing():
    """every limit, with its text; the report keeps its sentinel words through all of them"""
    n = 16
    a, b = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) + 5
    load = X.encode(X.LOAD, 0, 0, 0) + X.encode(X.LOAD, 1, 1, 1)
    acc = lambda c, reg=0: X.encode(X.ACC, 0, reg, c)
    ok = load + acc(0) + acc(1, 1)
    with Arena([rin("a", a), rin("b", b), rout("report", 2 * 256)]) as ar:
        cols, rep = ar.ptrs(["a", "b"]), ar.ptr("report")
        call = lambda words, log=4, k=2, report=rep, n_cols=2: L.call(ENTRY, cols, n_cols, log, L.u32x(words), len(words) // 2, k, report)
        cases = [
            ("air check: null or misaligned report", lambda: call(ok, report=None)),
            ("air check: null or misaligned report", lambda: call(ok, report=ar.ptr("report", 4))),
            ("air check: null or misaligned report", lambda: call(ok, report=ar.ptr("report", 8))),
            ("air check: log_size out of range", lambda: call(ok, log=0)),
            ("air check: log_size out of range", lambda: call(ok, log=29)),
            ("air check: number of constraints out of range", lambda: call(ok, k=0)),
            ("air check: number of constraints out of range", lambda: call(ok, k=257)),
            ("air check: number of columns out of range", lambda: call(ok, n_cols=0)),
            ("air check: program length out of range", lambda: call([])),
            ("air check: bad opcode", lambda: call(load + X.encode(STORE, 0, 0, 0), k=1)),
            ("air check: bad opcode", lambda: call(load + X.encode(9, 0, 0) + acc(0), k=1)),
            ("air check: first constraint index is not 0", lambda: call(load + acc(1) + acc(1, 1))),
            ("air check: constraint index decreases", lambda: call(load + acc(0) + acc(1) + acc(0, 1))),
            ("air check: constraint index skips", lambda: call(load + acc(0) + acc(2, 1), k=3)),
            ("air check: constraint index out of range", lambda: call(load + acc(0) + acc(1) + acc(2, 1))),
            ("air check: last constraint index is not n_constraints - 1", lambda: call(load + acc(0) + acc(0, 1))),
            ("air check: last constraint index is not n_constraints - 1", lambda: call(load, k=1)),
            ("air check: register out of range or read before written", lambda: call(load + acc(0, 2), k=1)),
            ("air check: column out of range", lambda: call(X.encode(X.LOAD, 0, 2, 0) + acc(0), k=1)),
            ("air check: row offset beyond the limit", lambda: call(X.encode(X.LOAD, 0, 0, 65) + acc(0), k=1)),
            ("air check: constant out of range", lambda: call(X.encode(X.CONST, 0, 0, P) + acc(0), k=1)),
            ("null device pointer in table", lambda: L.call(ENTRY, L.ptr_array([None, None]), 2, 4, L.u32x(ok), len(ok) // 2, 2, rep)),
        ]
        for text, f in cases:
            with pytest.raises(L.TstwoError) as e:
                f()
            assert str(e.value) == text
        L.sync()
        L.call("tstwo_graph_begin_capture")
        try:
            with pytest.raises(L.TstwoError, match="host-array upload during graph capture"):
                call(ok)
        finally:
            h = C.c_void_p()
            try:
                L.call("tstwo_graph_end_capture", C.byref(h))
            except L.TstwoError:
                pass
            if h.value:
                L.call("tstwo_graph_destroy", h)
        got = ar.check()
        assert (got["report"] == SENTINEL).all()
    # and the same arguments without a mistake pass: constraint 0 = a (zero at storage position 0 = coset row 0), constraint 1 = b at +1
    with Arena([rin("a", a), rin("b", b), rout("report", 4)]) as ar:
        L.call(ENTRY, ar.ptrs(["a", "b"]), 2, 4, L.u32x(ok), len(ok) // 2, 2, ar.ptr("report"))
        assert ar.check()["report"].tolist() == [15, 1, 16, 0]

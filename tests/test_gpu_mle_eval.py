"""-m gpu: Mle.evalAtPoint on the device (tstwo_mle_eval_at_point_base / _secure, csrc/mle_eval.hip) bit for bit against the integer
model (gkr_model.eval_mle_at), for n <= 8 also against the reference's recursion written out here, over the shapes of
tests/mle_eval_plan.py::gpu_shapes (every branch of the launch plan: tests/test_cpu_mle_eval_plan.py), between guard bands, at the
operands that saturate the lazy accumulators, and with the refusals of the entry points."""
import ctypes as C

import numpy as np
import pytest

import gkr_model as M
import mle_eval_plan as MP
from arena import Arena, rin
from tstwo_amd import _lib as L
from tstwo_amd import gkr as G
from tstwo_amd.fields import QM31

pytestmark = pytest.mark.gpu

P = M.P
BAD_ARG = 7                     # TSTWO_ERR_BAD_ARG
SHAPES = MP.gpu_shapes()


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def q(t):
    return QM31.from_u32_unchecked(*t)


# ------------------------------------------------------------------ references
def model_values(cols, point):
    """gkr_model.eval_mle_at for every column, with its eq table built once for all of them (eval_mle_at builds the same table
    per call): sum_x eq(x, point) col[x]."""
    e = M.gen_eq_evals(list(point), M.ONE)
    return [M.vsum(M.vmul_base(e, c) if c.ndim == 1 else M.vmul(c, e)) for c in cols]


def reference_recursion(evals, point):
    """Mle.evalAtPoint of the reference (lookups/mle.ts:81-114) as it is written there: split in halves, recurse on the rest
    of the point, p_0 (rhs - lhs) + lhs."""
    if not point:
        return evals[0]
    mid = len(evals) // 2
    lhs, rhs = reference_recursion(evals[:mid], point[1:]), reference_recursion(evals[mid:], point[1:])
    return M.qadd(M.qmul(point[0], M.qsub(rhs, lhs)), lhs)


# ------------------------------------------------------------------ device side
class Columns:
    """n_cols columns of n words in ONE device block, every column `offset` bytes past a 16-byte boundary."""

    def __init__(self, cols, offset=0):
        n = len(cols[0])
        pitch = (4 * n + 15) // 16 * 16
        self.buf = L.DeviceBuffer(pitch * len(cols) + 16)
        img = np.zeros((len(cols), pitch // 4), dtype=np.uint32)
        for k, c in enumerate(cols):
            img[k, :n] = c
        self.buf.upload(img, offset)
        self.ptrs = [self.buf.ptr + offset + k * pitch for k in range(len(cols))]

    def free(self):
        self.buf.free()


def call(secure, ptrs, n_mles, log_n, point):
    out = (C.c_uint32 * (4 * n_mles))()
    L.call("tstwo_mle_eval_at_point_secure" if secure else "tstwo_mle_eval_at_point_base", L.ptr_array(ptrs), n_mles, log_n,
           L.u32x([w for p in point for w in p]), out)
    return [tuple(int(w) for w in out[4 * k:4 * k + 4]) for k in range(n_mles)]


def make(rng, log_n, n_mles, secure):
    n = 1 << log_n
    return [M.random_secure(rng, n) if secure else M.random_base(rng, n) for _ in range(n_mles)]


def flat(mles):
    """The device columns of a list of model MLEs: 4 per secure MLE."""
    return [c for m in mles for c in (m if m.ndim == 2 else [m])]


# ------------------------------------------------------------------ every plan branch, against the model
@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_at_point_matches_the_model(name):
    log_n, n_mles, secure, offset = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()) + 7000)
    # a batch repeats few distinct MLEs (a batch may name one column twice, and the model runs once per distinct MLE)
    distinct = make(rng, log_n, min(n_mles, 3), secure)
    order = [k % len(distinct) for k in range(n_mles)]
    point = [M.random_felt(rng) for _ in range(log_n)]
    cols = Columns(flat(distinct), offset)
    per = 4 if secure else 1
    ptrs = [cols.ptrs[per * k + j] for k in order for j in range(per)]
    got = call(secure, ptrs, n_mles, log_n, point)
    want = model_values(distinct, point)
    assert got == [want[k] for k in order]
    if log_n <= 14:
        assert want[0] == M.eval_mle_at(distinct[0], point)
    if log_n <= 8:
        evals = [M.at(distinct[0], i) for i in range(1 << log_n)]
        assert want[0] == reference_recursion(evals, point)
    cols.free()


@pytest.mark.parametrize("secure", [False, True])
@pytest.mark.parametrize("log_n", [0, 1, 5, 12, 13, 15])
def test_vertices_select_one_value(secure, log_n):
    """All 0 and all 1 select f[0] and f[2^n - 1]; a 0/1 vertex returns exactly f[index] (first variable = top bit)."""
    rng = np.random.default_rng(7100 + log_n)
    mles = make(rng, log_n, 2, secure)
    cols = Columns(flat(mles))
    n = 1 << log_n
    for index in sorted({0, n - 1, int(rng.integers(0, n)), int(rng.integers(0, n))}):
        point = [M.qm((index >> (log_n - 1 - j)) & 1) for j in range(log_n)]
        assert call(secure, cols.ptrs, 2, log_n, point) == [M.at(m, index) for m in mles], index
    cols.free()


@pytest.mark.parametrize("secure", [False, True])
@pytest.mark.parametrize("log_n", [3, 12, 14, 16])
def test_saturated_operands(secure, log_n):
    """tests/saturation.py family S: every value and every point word P - 1, the largest terms the lazy 64-bit sums of
    k_mle_first can meet (4 products of (P - 1)^2 and a carry)."""
    from saturation import SAT, SAT4
    n = 1 << log_n
    # base MLEs of 2^16 values take the 4-group kernel from 64 MLEs on: the one column is named 64 times
    n_mles = 64 if (log_n == 16 and not secure) else 2
    mle = np.full((4, n) if secure else n, SAT, dtype=np.uint64)
    point = [SAT4] * log_n
    cols = Columns(flat([mle]))
    got = call(secure, cols.ptrs * n_mles, n_mles, log_n, point)
    assert got == model_values([mle], point) * n_mles
    cols.free()


@pytest.mark.parametrize("secure", [False, True])
@pytest.mark.parametrize("log_n,offset", [(0, 0), (2, 4), (7, 0), (12, 0), (13, 8), (14, 0)])
def test_between_guard_bands(secure, log_n, offset):
    """Inputs untouched, nothing stored outside the library's own scratch: the columns sit in an arena of guard bands
    (tests/arena.py), 2 MLEs, the second at its own offset."""
    rng = np.random.default_rng(7200 + log_n)
    mles = make(rng, log_n, 2, secure)
    point = [M.random_felt(rng) for _ in range(log_n)]
    fc = flat(mles)
    names = [f"c{k}" for k in range(len(fc))]
    with Arena([rin(nm, c.astype(np.uint32), offset) for nm, c in zip(names, fc)]) as A:
        got = call(secure, [A.addr(nm) for nm in names], 2, log_n, point)
        A.check()
    assert got == model_values(mles, point)


def test_refusals():
    """The five refusals, each TSTWO_ERR_BAD_ARG with its text, before anything is enqueued; then the same arguments within
    the limits work."""
    col = Columns([np.arange(16, dtype=np.uint64)] * 4)
    point = L.u32x([1, 2, 3, 4] * 4)
    out = (C.c_uint32 * 8)()
    one, four = L.ptr_array(col.ptrs[:1]), L.ptr_array(col.ptrs)
    bad_point = L.u32x([1, 2, 3, 4] * 3 + [1, 2, P, 4])
    for fn, tab in (("tstwo_mle_eval_at_point_base", one), ("tstwo_mle_eval_at_point_secure", four)):
        cases = {"no MLE given": (tab, 0, 4, point, out), "more than 28 variables": (tab, 1, 29, point, out),
                 "null argument": (None, 1, 4, point, out), "null argument.": (tab, 1, 4, None, out), "null argument..": (tab, 1, 4, point, None),
                 "null device pointer in table": (L.ptr_array([0] * 4), 1, 4, point, out),
                 "point word out of range": (tab, 1, 4, bad_point, out)}
        for text, args in cases.items():
            with pytest.raises(L.TstwoError, match="^mle eval_at_point: " + text.rstrip(".")) as e:
                L.call(fn, *args)
            assert e.value.code == BAD_ARG, text
        L.sync()
        L.call("tstwo_graph_begin_capture")
        try:
            with pytest.raises(L.TstwoError, match="^mle eval_at_point: .*graph capture") as e:
                L.call(fn, tab, 1, 4, point, out)
            assert e.value.code == BAD_ARG
        finally:
            h = C.c_void_p()
            try:
                L.call("tstwo_graph_end_capture", C.byref(h))
            except L.TstwoError:
                pass
            if h.value:
                L.call("tstwo_graph_destroy", h)
        L.call(fn, tab, 1, 4, point, out)
    pt = [(1, 2, 3, 4)] * 4
    assert tuple(out[:4]) == model_values([np.stack([np.arange(16, dtype=np.uint64)] * 4)], pt)[0]
    col.free()


# ------------------------------------------------------------------ the Python mirror
@pytest.mark.parametrize("is_base", [False, True])
@pytest.mark.parametrize("n", [0, 1, 6, 13])
def test_eval_at_point_is_the_chain_of_fix_first_variable(is_base, n):
    rng = np.random.default_rng(7300 + n)
    col = M.random_base(rng, 1 << n) if is_base else M.random_secure(rng, 1 << n)
    mle = G.Mle.base(col.astype(np.uint32)) if is_base else G.Mle.secure([c.astype(np.uint32) for c in col])
    point = [q(M.random_felt(rng)) for _ in range(n)]
    got = mle.eval_at_point(point)
    assert got.tup() == G.HipMleOps.evalAtPoint(mle, point).tup() == mle.evalAtPoint(point).tup()
    cur = mle
    for p in point:
        cur = cur.fix_first_variable(p)
    assert got.tup() == cur.at(0).tup() == M.eval_mle_at(col, [p.tup() for p in point])


def test_eval_mles_at_point_groups_by_kind_and_keeps_the_order():
    rng = np.random.default_rng(7400)
    cols = [M.random_base(rng, 64), M.random_secure(rng, 64), M.random_base(rng, 64), M.random_secure(rng, 64)]
    mles = [G.Mle.base(c.astype(np.uint32)) if c.ndim == 1 else G.Mle.secure([x.astype(np.uint32) for x in c]) for c in cols]
    point = [M.random_felt(rng) for _ in range(6)]
    calls = []
    orig = L.call
    try:
        L.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        got = G.eval_mles_at_point(mles, [q(p) for p in point])
    finally:
        L.call = orig
    assert [g.tup() for g in got] == [M.eval_mle_at(c, point) for c in cols]
    assert sorted(calls) == ["tstwo_mle_eval_at_point_base", "tstwo_mle_eval_at_point_secure"]
    assert G.eval_mles_at_point([], []) == []


def test_wrong_point_length_raises():
    mle = G.Mle.base(np.arange(8, dtype=np.uint32))
    for k in (0, 2, 4):
        with pytest.raises(ValueError, match="coordinates"):
            mle.eval_at_point([QM31.one()] * k)
    with pytest.raises(ValueError, match="coordinates"):
        G.eval_mles_at_point([mle, G.Mle.base(np.arange(4, dtype=np.uint32))], [QM31.one()] * 3)

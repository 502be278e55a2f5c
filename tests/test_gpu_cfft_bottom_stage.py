"""-m gpu tests of the bottom pass's tile staging (csrc/cfft_fast.cuh: k_cfft_b).

A workgroup of the bottom pass owns runs of columns that share a tile position: it stages the twiddles once per run, keeps the
next column's tile in flight while the current one is transformed in the one LDS tile buffer.  (The same body with the
non-temporal policy on its tile accesses, k_cfft_b_stream, runs forward transforms of 1 GiB and more: all 2^30 words of one are
compared in test_gpu_config5_trace.py.)  The shapes are the smallest at which that data path can go wrong:
  * log 13 (one tile, bottom pass only; the inverse carries the 2^-n scale): runs of 1, 2, 3 and 33 columns -- no next tile, a
    reused tile buffer, a workgroup that owns many columns.  A wrong wait shows as the previous column's words;
  * log 15, 16 (13 bottom layers + one strided pass: tile index > 0, the heap / twiddle offsets depend on it; the inverse bottom
    pass is unscaled) with 3, 5, 7 columns: the equal shares of (tile, column) items cut runs in the middle of a tile;
  * log 17 x 64 columns: 1024 items, so workgroups are co-resident on a CU and one writing into a neighbour's buffer would show.
Every word is compared with the CPU oracle, and every column lies between guard bands (tests/arena.py): nothing outside the
columns may change.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rand_column
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402
from arena import Arena, Layout, check_image, rin, rinout, rout  # noqa: E402

OL = orc.lib()
SHAPES = [(13, 1), (13, 2), (13, 3), (13, 33), (15, 3), (15, 5), (15, 7), (16, 3), (16, 5), (16, 7), (17, 64)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()
    for cached in (twiddles, case):
        cached.cache_clear()


def half_odds(k):
    return OL.orc_half_odds_initial(k)


@functools.lru_cache(maxsize=None)
def twiddles(log):
    return orc.precompute_twiddles(half_odds(log), log)


def evaluate_ref(cols, log):
    tw = twiddles(log - 1)[0]
    if log >= 16:
        return orc.mt_cfft_evaluate([c.copy() for c in cols], log, half_odds(log - 1), tw, log - 1, 16)
    return [orc.cfft_evaluate(c, log, half_odds(log - 1), tw, log - 1) for c in cols]


def interpolate_ref(cols, log):
    return [orc.cfft_interpolate(c, log, half_odds(log - 1), twiddles(log - 1)[1], log - 1) for c in cols]


@functools.lru_cache(maxsize=None)
def case(log, n_cols, seed=0):
    """Columns of different random words, their evaluations and their interpolations, all from the oracle (read-only)."""
    cols = [rand_column(7000 + 1000 * seed + 100 * log + c, 1 << log) for c in range(n_cols)]
    evs, its = evaluate_ref(cols, log), interpolate_ref(cols, log)
    for a in cols + list(evs) + list(its):
        a.setflags(write=False)
    return cols, evs, its


def names(prefix, k):
    return [f"{prefix}{i}" for i in range(k)]


def regions(cols, log, inverse):
    tw, itw = twiddles(log - 1)
    return [rinout(k, c) for k, c in zip(names("col", len(cols)), cols)] + [rin("tw", itw if inverse else tw)]


def transform(A, entry, log, n_cols):
    L.call(f"tstwo_cfft_{entry}", A.ptrs(names("col", n_cols)), n_cols, log, half_odds(log - 1), A.ptr("tw"), log - 1)


def assert_columns(got, exp, what=""):
    for i, e in enumerate(exp):
        g = got[f"col{i}"]
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what} column {i}: {bad.size} wrong words, first at {int(bad[0])}"


@pytest.mark.parametrize("log,n_cols", SHAPES)
def test_evaluate(log, n_cols):
    cols, evs, _ = case(log, n_cols)
    with Arena(regions(cols, log, False)) as A:
        transform(A, "evaluate", log, n_cols)
        assert_columns(A.check(), evs)


@pytest.mark.parametrize("log,n_cols", SHAPES)
def test_interpolate(log, n_cols):
    """log 13: the bottom pass is the last one and scales by 2^-n; above, it is the first and does not."""
    cols, _, its = case(log, n_cols)
    with Arena(regions(cols, log, True)) as A:
        transform(A, "interpolate", log, n_cols)
        assert_columns(A.check(), its)


@pytest.mark.parametrize("log,n_cols", [(13, 3), (15, 5)])
def test_interpolate_to(log, n_cols):
    """The out-of-place bottom pass (sources read, never written)."""
    cols, _, its = case(log, n_cols)
    s_, d_ = names("src", n_cols), names("col", n_cols)
    regs = [rin(k, c) for k, c in zip(s_, cols)] + [rout(k, 1 << log) for k in d_] + [rin("tw", twiddles(log - 1)[1])]
    with Arena(regs) as A:
        L.call("tstwo_cfft_interpolate_to", A.ptrs(s_), A.ptrs(d_), n_cols, log, half_odds(log - 1), A.ptr("tw"), log - 1)
        assert_columns(A.check(), its)


@pytest.mark.parametrize("log,n_cols", [(13, 3), (15, 5)])
def test_same_call_twice_and_round_trip(log, n_cols):
    """evaluate, evaluate on the same buffers with nothing between them, then interpolate, interpolate: the second evaluation
    is the oracle's evaluation of the first, and the two interpolations give the input back."""
    cols, evs, _ = case(log, n_cols)
    twice = evaluate_ref(evs, log)
    tw, itw = twiddles(log - 1)
    regs = [rinout(k, c) for k, c in zip(names("col", n_cols), cols)] + [rin("tw", tw), rin("itw", itw)]
    with Arena(regs) as A:
        for _ in range(2):
            L.call("tstwo_cfft_evaluate", A.ptrs(names("col", n_cols)), n_cols, log, half_odds(log - 1), A.ptr("tw"), log - 1)
        assert_columns(A.check(), twice, "evaluate twice:")
        for _ in range(2):
            L.call("tstwo_cfft_interpolate", A.ptrs(names("col", n_cols)), n_cols, log, half_odds(log - 1), A.ptr("itw"), log - 1)
        assert_columns(A.check(), cols, "round trip:")


def test_graph_replay():
    """One evaluate captured into a graph (the launch geometry is pinned by it) and replayed twice on new input words copied into
    the same buffers: each replay gives the oracle's words for its input, guards intact."""
    log, n_cols = 15, 5
    data = [case(log, n_cols, seed) for seed in range(3)]
    layouts = [Layout(regions(d[0], log, False)) for d in data]
    h = C.c_void_p()
    staged = []
    with Arena(regions(data[0][0], log, False)) as A:
        try:
            transform(A, "evaluate", log, n_cols)          # eager once: the allocator and the pointer tables are warm
            assert_columns(A.check(), data[0][1], "eager:")
            L.call("tstwo_graph_begin_capture")
            try:
                transform(A, "evaluate", log, n_cols)
            finally:
                L.call("tstwo_graph_end_capture", C.byref(h))
            for seed in (1, 2):
                b = L.DeviceBuffer(A.layout.total)
                b.upload(layouts[seed].image())
                staged.append(b)
            L.sync()
            for step, seed in enumerate((1, 2)):
                L.call("tstwo_copy", C.c_void_p(A.buf.ptr), C.c_void_p(staged[step].ptr), A.layout.total)
                L.call("tstwo_graph_launch", h)
                got = check_image(layouts[seed], layouts[seed].image(), A.buf.download(np.uint8))
                assert_columns(got, data[seed][1], f"replay {step}:")
        finally:
            L.sync()
            if h.value:
                L.call("tstwo_graph_destroy", h)
            for b in staged:
                b.free()

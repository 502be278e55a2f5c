"""-m gpu tests of the Circle FFT's launch plan (csrc/cfft_plan.h) as the library runs it.

tests/cfft_plan.py is the tests' statement of the plan (compared with the header, without a GPU, in test_cpu_cfft_plan.py).  Here:
  * tstwo_cfft_plan_passes reports that plan's pass count, on this device's compute units, for every size and column count;
  * every (kind, K, LOGT) shape that the shipped library can launch, except the non-temporal ones (they need 1 GiB of columns:
    test_gpu_cfft_bottom_stage.py, test_gpu_config5_trace.py), is launched once, on the smallest column set the model finds for
    it, through all four entries: evaluate against the CPU oracle, interpolate back to the input, interpolate_to against the
    in-place result with its source untouched, evaluate_extended from one and two bits below against extend + evaluate.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import cfft_plan as P
from conftest import rand_column
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402

OL = orc.lib()
COLS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 256, 512, 1024)
MAX_BYTES = 128 << 20
SHAPES = sorted(s for s, knob_only in P.TABLE.items() if not knob_only and not s[0].endswith("_stream"))
vp = C.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()
    for cached in (n_cus, checked):
        cached.cache_clear()


@functools.lru_cache(maxsize=None)
def n_cus():
    """this device's compute units: tstwo_device_name ends in "(<arch>, <count> CUs)" """
    return int(re.search(r"(\d+) CUs\)$", L.device_name()).group(1))


def test_plan_passes_reports_the_models_count():
    """n = 1..30 x the column counts of the CPU sweep; a pair is left out only when the call itself refuses it"""
    compared = 0
    for n in range(1, 31):
        for n_cols in COLS:
            got = C.c_uint32(0)
            try:
                L.call("tstwo_cfft_plan_passes", n, n_cols, C.byref(got))
            except L.TstwoError:
                continue
            assert got.value == len(P.plan("evaluate", n, n_cols, n_cus()).passes), (n, n_cols)
            compared += 1
    assert compared == 30 * len(COLS)           # (nothing in this range is refused today)


def _ptrs(bufs):
    return L.ptr_array([b.ptr for b in bufs])


def _upload(cols):
    out = []
    for c in cols:
        b = L.DeviceBuffer(c.nbytes)
        b.upload(c)
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def checked(n, n_cols):
    """All four entries on n_cols columns of 2^n words; True once they have passed (shapes that share a case share the run)."""
    half = OL.orc_half_odds_initial(n - 1)
    tw, itw = L.DeviceBuffer(4 << (n - 1)), L.DeviceBuffer(4 << (n - 1))
    L.call("tstwo_twiddles_build", half, n - 1, vp(tw.ptr), vp(itw.ptr))
    cols = [rand_column(9100 + 64 * n + c, 1 << n) for c in range(n_cols)]
    bufs = []
    try:
        d = _upload(cols)
        bufs += d
        L.call("tstwo_cfft_evaluate", _ptrs(d), n_cols, n, half, vp(tw.ptr), n - 1)
        evals = [b.download() for b in d]
        otw = orc.precompute_twiddles(half, n - 1, inverse=False)[0]
        assert (evals[0] == orc.mt_cfft_evaluate([cols[0].copy()], n, half, otw, n - 1, 16)[0]).all(), "evaluate, column 0 against the oracle"
        L.call("tstwo_cfft_interpolate", _ptrs(d), n_cols, n, half, vp(itw.ptr), n - 1)
        for i, (b, c) in enumerate(zip(d, cols)):
            assert (b.download() == c).all(), f"interpolate, column {i}"
        src, dst = _upload(evals), [L.DeviceBuffer(4 << n) for _ in cols]
        bufs += src + dst
        L.call("tstwo_cfft_interpolate_to", _ptrs(src), _ptrs(dst), n_cols, n, half, vp(itw.ptr), n - 1)
        for i, (s, o, e, c) in enumerate(zip(src, dst, evals, cols)):
            assert (o.download() == c).all(), f"interpolate_to, column {i}"
            assert (s.download() == e).all(), f"interpolate_to wrote its source, column {i}"
        for log_poly in (n - 1, n - 2):
            polys = [c[:1 << log_poly] for c in cols]
            small = _upload(polys)
            bufs += small
            for s, o in zip(small, d):
                L.call("tstwo_poly_extend", vp(s.ptr), log_poly, vp(o.ptr), n)
            L.call("tstwo_cfft_evaluate", _ptrs(d), n_cols, n, half, vp(tw.ptr), n - 1)
            L.call("tstwo_cfft_evaluate_extended", _ptrs(small), log_poly, _ptrs(dst), n_cols, n, half, vp(tw.ptr), n - 1)
            for i, (o, r, s, p) in enumerate(zip(dst, d, small, polys)):
                assert (o.download() == r.download()).all(), f"evaluate_extended from 2^{log_poly}, column {i}"
                assert (s.download() == p).all(), f"evaluate_extended wrote its source, column {i}"
    finally:
        L.sync()
        for b in bufs + [tw, itw]:
            b.free()
    return True


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_every_shipped_shape_runs(shape):
    case = P.smallest_case(shape, n_cus(), COLS, MAX_BYTES)
    assert case is not None, "no column set of 128 MiB or less reaches this shape"
    assert checked(*case)

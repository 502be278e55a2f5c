"""-m gpu guard-band tests: no entry point writes outside its outputs.

Every device argument of one C-ABI call lives in one guarded arena (tests/arena.py): 16 KiB of the word 0xA5A5A5A5 before and
after every region.  After the call the whole arena comes back in one download and three things are asserted for every case:
the output payloads equal the CPU oracle / integer model bit for bit, every guard word still holds the sentinel, and every
input region is what was uploaded.  Expected values never come from another call of the library.

Placements (where the header lets a pointer be unaligned): all pointers 16-byte aligned, all offset by 4 bytes, only the
outputs offset, only one input offset -- the last two force the scalar kernels at a vectorisable n.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import P, rand_column
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402
from arena import Arena, Region, rin, rinout, rout  # noqa: E402

OL = orc.lib()
ALPHA = (19283, 1, 2, 3)
PLACEMENTS = ("aligned", "all+4", "out+4", "in+4")
N_CUS = 256                       # the grid-cap shapes below are written for a 256-CU part (fewer CUs: lower caps, still crossed)


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()
    for cached in (otwiddles, cfft_case, circle_inv_y):         # the shared references (up to 150 MB each) end with this module
        cached.cache_clear()


def half_odds(k):
    return OL.orc_half_odds_initial(k)


def offs(place, ins, outs):
    """Byte offset from a 16-byte boundary of every named region under a placement."""
    o = {n: 0 for n in list(ins) + list(outs)}
    if place == "all+4":
        o = {n: 4 for n in o}
    elif place == "out+4":
        o.update({n: 4 for n in outs})
    elif place == "in+4":
        o[list(ins)[0]] = 4
    else:
        assert place == "aligned"
    return o


def names(prefix, k=4):
    return [f"{prefix}{i}" for i in range(k)]


def soa(seed, n, k=4, nonzero=False):
    return [rand_column(seed + i, n, nonzero) for i in range(k)]


def eq(got, exp):
    return got.shape == np.asarray(exp).shape and bool((got == exp).all())


@functools.lru_cache(maxsize=None)
def otwiddles(log):
    """(tw, itw) of the tree of half_odds(log), from the oracle."""
    return orc.precompute_twiddles(half_odds(log), log)


# ------------------------------------------------------------------ M31 columns
M31_NS = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1021, 1024, 1027]


def _m31_op(op, n, place, seed=1):
    a, b = rand_column(seed, n), rand_column(seed + 1, n)
    ins = ["a"] if op == "neg" else ["a", "b"]
    o = offs(place, ins, ["out"])
    regs = [rin("a", a, o["a"])] + ([] if op == "neg" else [rin("b", b, o["b"])]) + [rout("out", n, o["out"])]
    with Arena(regs) as A:
        if op == "neg":
            L.call("tstwo_m31_neg", A.ptr("a"), A.ptr("out"), n)
        else:
            L.call(f"tstwo_m31_{op}", A.ptr("a"), A.ptr("b"), A.ptr("out"), n)
        got = A.check()
    assert eq(got["out"], orc.col_op(op, a, b))


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", M31_NS)
@pytest.mark.parametrize("op", ["add", "sub", "mul", "neg"])
def test_m31_elementwise(op, n, place):
    _m31_op(op, n, place)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027])
@pytest.mark.parametrize("entry", ["tstwo_m31_batch_inverse", "tstwo_m31_batch_inverse_async"])
def test_m31_batch_inverse_k4(entry, n, place):
    a = rand_column(5, n, nonzero=True)
    o = offs(place, ["in"], ["out"])
    with Arena([rin("in", a, o["in"]), rout("out", n, o["out"])]) as A:
        L.call(entry, A.ptr("in"), A.ptr("out"), n)
        if entry.endswith("_async"):
            L.call("tstwo_check_zero_flag")
        got = A.check()
    assert eq(got["out"], orc.m31_batch_inverse(a))


def test_m31_batch_inverse_k16_ragged():
    """k_m31_batch_inverse<16> serves n >= 2^24 only: n = 2^24 + 5 leaves T = ceil(n / 16) = 2^20 + 1 lanes, of which all but
    the first five run past n in their last element (the i < n guard of loads and stores)."""
    n = (1 << 24) + 5
    a = rand_column(6, n, nonzero=True)
    with Arena([rin("in", a), rout("out", n)]) as A:
        L.call("tstwo_m31_batch_inverse", A.ptr("in"), A.ptr("out"), n)
        got = A.check()
    assert eq(got["out"], orc.m31_batch_inverse(a))


def cm31_inverse_oracle(a):
    n = a[0].size
    aos = np.ascontiguousarray(np.stack(a, axis=1), dtype=np.uint32)
    out = np.zeros_like(aos)
    rc = OL.orc_cm31_batch_inverse(aos.ctypes.data_as(C.POINTER(orc.CM31)), out.ctypes.data_as(C.POINTER(orc.CM31)), n)
    assert rc == 0
    return [np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1])]


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049])
@pytest.mark.parametrize("entry", ["tstwo_cm31_batch_inverse", "tstwo_cm31_batch_inverse_async"])
def test_cm31_batch_inverse(entry, n, place):
    a = soa(30, n, 2, nonzero=True)
    i_, o_ = names("in", 2), names("out", 2)
    o = offs(place, i_, o_)
    with Arena([rin(k, c, o[k]) for k, c in zip(i_, a)] + [rout(k, n, o[k]) for k in o_]) as A:
        L.call(entry, L.P2(*[A.addr(k) for k in i_]), L.P2(*[A.addr(k) for k in o_]), n)
        if entry.endswith("_async"):
            L.call("tstwo_check_zero_flag")
        got = A.check()
    exp = cm31_inverse_oracle(a)
    for k in range(2):
        assert eq(got[o_[k]], exp[k]), k


# n: aligned, these reach k_qm31_batch_inverse_norm (n % 8 == 0), _v4<1> (n % 4 == 0) and the strided <8>; misaligned, the
# vectorisable n = 8 and 2048 must take the strided kernel
QM31_INV_CASES = [(n, "aligned") for n in (1, 3, 4, 7, 8, 9, 12, 16, 2044, 2048, 2052)] + \
                 [(n, p) for n in (8, 2048) for p in PLACEMENTS[1:]]


@pytest.mark.parametrize("n,place", QM31_INV_CASES)
@pytest.mark.parametrize("entry", ["tstwo_qm31_batch_inverse", "tstwo_qm31_batch_inverse_async"])
def test_qm31_batch_inverse(entry, n, place):
    a = soa(10, n, nonzero=True)
    i_, o_ = names("in"), names("out")
    o = offs(place, i_, o_)
    with Arena([rin(k, c, o[k]) for k, c in zip(i_, a)] + [rout(k, n, o[k]) for k in o_]) as A:
        L.call(entry, A.p4(i_), A.p4(o_), n)
        if entry.endswith("_async"):
            L.call("tstwo_check_zero_flag")
        got = A.check()
    exp = orc.qm31_batch_inverse(a)
    for k in range(4):
        assert eq(got[o_[k]], exp[k]), k


# ------------------------------------------------------------------ QM31 SoA elementwise, accumulate, decompose
SOA_NS = [1, 3, 4, 5, 8, 255, 256, 257, 1024, 1027]


def _qm31_mul(n, place):
    a, b = soa(10, n), soa(20, n)
    a_, b_, o_ = names("a"), names("b"), names("out")
    o = offs(place, a_ + b_, o_)
    with Arena([rin(k, c, o[k]) for k, c in zip(a_ + b_, a + b)] + [rout(k, n, o[k]) for k in o_]) as A:
        L.call("tstwo_qm31_mul", A.p4(a_), A.p4(b_), A.p4(o_), n)
        got = A.check()
    exp = orc.qm31_col_mul(a, b)
    for k in range(4):
        assert eq(got[o_[k]], exp[k]), k


def _secure_accumulate(n, place):
    col, other = soa(40, n), soa(50, n)
    c_, t_ = names("col"), names("other")
    o = offs(place, t_, c_)
    with Arena([rinout(k, c, o[k]) for k, c in zip(c_, col)] + [rin(k, c, o[k]) for k, c in zip(t_, other)]) as A:
        L.call("tstwo_secure_accumulate", A.p4(c_), A.p4(t_), n)
        got = A.check()
    exp = orc.accumulate(col, other)
    for k in range(4):
        assert eq(got[c_[k]], exp[k]), k


def _decompose(n, place):
    cols = soa(500, n)
    i_, o_ = names("in"), names("out")
    o = offs(place, i_, o_)
    lam = (C.c_uint32 * 4)()
    with Arena([rin(k, c, o[k]) for k, c in zip(i_, cols)] + [rout(k, n, o[k]) for k in o_]) as A:
        L.call("tstwo_fri_decompose", A.p4(i_), n, A.p4(o_), lam)
        got = A.check()
    exp, elam = orc.decompose(cols)
    assert tuple(lam) == elam
    for k in range(4):
        assert eq(got[o_[k]], exp[k]), k


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", SOA_NS)
def test_qm31_mul(n, place):
    _qm31_mul(n, place)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", SOA_NS)
def test_secure_accumulate(n, place):
    _secure_accumulate(n, place)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", SOA_NS)
def test_fri_decompose(n, place):
    _decompose(n, place)


# ------------------------------------------------------------------ extend, bit reverse, twiddles
EXTEND_CASES = [(s, d) for s in range(5) for d in range(s, s + 4)] + [(10, 13)]


def _extend(log_src, log_dst, place):
    src = rand_column(9 + log_src, 1 << log_src)
    o = offs(place, ["src"], ["dst"])
    with Arena([rin("src", src, o["src"]), rout("dst", 1 << log_dst, o["dst"])]) as A:
        L.call("tstwo_poly_extend", A.ptr("src"), log_src, A.ptr("dst"), log_dst)
        got = A.check()
    exp = np.zeros(1 << log_dst, dtype=np.uint32)          # PolyOps.extend: the coefficients, zero-padded
    exp[:1 << log_src] = src
    assert eq(got["dst"], exp)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("log_src,log_dst", EXTEND_CASES)
def test_poly_extend(log_src, log_dst, place):
    _extend(log_src, log_dst, place)


@pytest.mark.parametrize("place", ["aligned", "one+4"])
@pytest.mark.parametrize("n_cols", [1, 3])
@pytest.mark.parametrize("log", list(range(1, 14)))
def test_bit_reverse(log, n_cols, place):
    """Aligned columns take k_bit_reverse_tiled from log 12; one column offset by 4 bytes sends the launch to k_bit_reverse."""
    cols = soa(40 + log, 1 << log, n_cols)
    c_ = names("col", n_cols)
    with Arena([rinout(k, c, 4 if (place == "one+4" and i == n_cols - 1) else 0) for i, (k, c) in enumerate(zip(c_, cols))]) as A:
        L.call("tstwo_bit_reverse", A.ptrs(c_), n_cols, 1 << log)
        got = A.check()
    for k, c in zip(c_, cols):
        assert eq(got[k], orc.bit_reverse(c)), k


@pytest.mark.parametrize("place", ["aligned", "all+4"])
@pytest.mark.parametrize("with_itw", [False, True])
@pytest.mark.parametrize("log", list(range(0, 14)))
def test_twiddles_build(log, with_itw, place):
    off = 4 if place == "all+4" else 0
    regs = [rout("tw", 1 << log, off)] + ([rout("itw", 1 << log, off)] if with_itw else [])
    with Arena(regs) as A:
        L.call("tstwo_twiddles_build", half_odds(log), log, A.ptr("tw"), A.ptr("itw") if with_itw else C.c_void_p(0))
        got = A.check()
    etw, eitw = otwiddles(log)
    assert eq(got["tw"], etw)
    if with_itw:
        assert eq(got["itw"], eitw)


# ------------------------------------------------------------------ CFFT: every column its own region
@functools.lru_cache(maxsize=None)
def cfft_case(log, n_cols, log_poly=None):
    """Seeded coefficient columns (2^log_poly of them nonzero) and their evaluations on CanonicCoset(log), from the oracle."""
    tw_log = max(log - 1, 1)
    half = half_odds(log - 1)
    otw = otwiddles(tw_log)[0]
    coeffs = []
    for c in range(n_cols):
        col = np.zeros(1 << log, dtype=np.uint32)
        m = 1 << (log if log_poly is None else log_poly)
        col[:m] = rand_column(100 * log + c, m)
        coeffs.append(col)
    if log >= 16:
        evs = orc.mt_cfft_evaluate([c.copy() for c in coeffs], log, half, otw, tw_log, 16)
    else:
        evs = [orc.cfft_evaluate(c, log, half, otw, tw_log) for c in coeffs]
    for a in coeffs + list(evs):
        a.setflags(write=False)
    return coeffs, evs


CFFT_SHAPES = [(log, n_cols) for log in (1, 2, 3, 4, 5, 6, 12, 13, 14, 15) for n_cols in (1, 3, 17)] + \
              [(16, 3), (20, 1), (21, 9)]       # one per larger plan family: log 16; 12 + 8 split; the 2^15 tile


@pytest.mark.parametrize("log,n_cols", CFFT_SHAPES)
@pytest.mark.parametrize("entry", ["evaluate", "interpolate", "interpolate_to"])
def test_cfft(entry, log, n_cols):
    coeffs, evs = cfft_case(log, n_cols)
    tw_log = max(log - 1, 1)
    half = half_odds(log - 1)
    tw, itw = otwiddles(tw_log)
    c_, d_ = names("col", n_cols), names("dst", n_cols)
    if entry == "evaluate":
        src, exp, regs = coeffs, evs, [rinout(k, c) for k, c in zip(c_, coeffs)] + [rin("tw", tw)]
    elif entry == "interpolate":
        src, exp, regs = evs, coeffs, [rinout(k, c) for k, c in zip(c_, evs)] + [rin("tw", itw)]
    else:                                 # the sources are inputs: check() asserts they are unchanged
        src, exp, regs = evs, coeffs, [rin(k, c) for k, c in zip(c_, evs)] + [rout(k, 1 << log) for k in d_] + [rin("tw", itw)]
    with Arena(regs) as A:
        if entry == "interpolate_to":
            L.call("tstwo_cfft_interpolate_to", A.ptrs(c_), A.ptrs(d_), n_cols, log, half, A.ptr("tw"), tw_log)
        else:
            L.call(f"tstwo_cfft_{entry}", A.ptrs(c_), n_cols, log, half, A.ptr("tw"), tw_log)
        got = A.check()
    for k, e in zip(d_ if entry == "interpolate_to" else c_, exp):
        assert eq(got[k], e), k


@pytest.mark.parametrize("log,n_cols", CFFT_SHAPES)
@pytest.mark.parametrize("ext", [1, 2])
def test_cfft_evaluate_extended(ext, log, n_cols):
    log_poly = max(log - ext, 0)
    coeffs, evs = cfft_case(log, n_cols, log_poly)
    tw_log = max(log - 1, 1)
    tw = otwiddles(tw_log)[0]
    p_, o_ = names("poly", n_cols), names("out", n_cols)
    regs = [rin(k, c[:1 << log_poly]) for k, c in zip(p_, coeffs)] + [rout(k, 1 << log) for k in o_] + [rin("tw", tw)]
    with Arena(regs) as A:
        L.call("tstwo_cfft_evaluate_extended", A.ptrs(p_), log_poly, A.ptrs(o_), n_cols, log, half_odds(log - 1), A.ptr("tw"), tw_log)
        got = A.check()
    for k, e in zip(o_, evs):
        assert eq(got[k], e), k


# ------------------------------------------------------------------ FRI folds
def _line_setup(k):
    """Tree of half_odds(k + 2); the line domain is its root doubled twice (as test_gpu_capi.test_fold_line)."""
    tw_log = max(k, 1) + 2
    coset_initial = (half_odds(tw_log) << (tw_log - k)) & 0x7FFFFFFF
    return tw_log, coset_initial, otwiddles(tw_log)[1]


@pytest.mark.parametrize("place", ["aligned", "all+4", "out+4"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 9, 14])
@pytest.mark.parametrize("entry", ["plain", "dev", "tw"])
def test_fri_fold_line(entry, k, place):
    n = 1 << k
    cols = soa(200 + 4 * k, n)
    tw_log, coset_initial, itw = _line_setup(k)
    i_, o_ = names("in"), names("out")
    o = offs(place, i_ + ["itw"], o_)
    if entry == "tw":                      # the n / 2 inverse twiddles themselves: the tree level of the line's coset
        itw = itw[(1 << tw_log) - n:(1 << tw_log) - n // 2]
    regs = [rin(x, c, o[x]) for x, c in zip(i_, cols)] + [rin("itw", itw, o["itw"])] + [rout(x, n // 2, o[x]) for x in o_]
    if entry == "dev":
        regs.append(rin("alpha", np.array(ALPHA, dtype=np.uint32)))          # 16-byte aligned, as the header demands
    with Arena(regs) as A:
        if entry == "plain":
            L.call("tstwo_fri_fold_line", A.p4(i_), k, A.ptr("itw"), tw_log, L.u32x(ALPHA), A.p4(o_))
        elif entry == "dev":
            L.call("tstwo_fri_fold_line_dev", A.p4(i_), k, A.ptr("itw"), tw_log, A.ptr("alpha"), A.p4(o_))
        else:
            L.call("tstwo_fri_fold_line_tw", A.p4(i_), k, A.ptr("itw"), L.u32x(ALPHA), A.p4(o_))
        got = A.check()
    exp = orc.fold_line(cols, k, coset_initial, ALPHA)
    for j in range(4):
        assert eq(got[o_[j]], exp[j]), j


@functools.lru_cache(maxsize=None)
def circle_inv_y(n, half_initial):
    """y^-1 of domain.at(bitrev(2i, n)), the explicit twiddles of tstwo_fri_fold_circle_into_line_tw."""
    inv = []
    for i in range(1 << (n - 1)):
        p = OL.orc_circle_domain_at(half_initial, n - 1, OL.orc_bit_reverse_index(2 * i, n))
        inv.append(pow(p.y, P - 2, P))
    return np.array(inv, dtype=np.uint32)


CIRCLE_CASES = [(e, n) for e in ("plain", "dev", "tw") for n in (3, 4, 5, 10)] + [("tw", 1), ("tw", 2)]


@pytest.mark.parametrize("place", ["aligned", "src+4", "dst+4", "all+4"])
@pytest.mark.parametrize("entry,n", CIRCLE_CASES)
def test_fri_fold_circle_into_line(entry, n, place):
    """Aligned sources take k_fold_circle2 (two rows per lane); a source or destination off its alignment the one-row kernel."""
    N = 1 << n
    src, dst = soa(300 + 4 * n, N), soa(400 + 4 * n, N // 2)
    s_, d_ = names("src"), names("dst")
    so = 4 if place in ("src+4", "all+4") else 0
    do = 4 if place in ("dst+4", "all+4") else 0
    if entry == "tw":
        half_initial = half_odds(n - 1)
        tw_log, twid = 0, circle_inv_y(n, half_initial)
    else:
        tw_log = n + 1
        half_initial = (half_odds(n + 1) << 2) & 0x7FFFFFFF     # root(half_odds(n + 1)).repeated_double(2)
        twid = otwiddles(tw_log)[1]
    regs = [rinout(x, c, do) for x, c in zip(d_, dst)] + [rin(x, c, so) for x, c in zip(s_, src)] + [rin("itw", twid, so)]
    if entry == "dev":
        regs.append(rin("alpha", np.array(ALPHA, dtype=np.uint32)))
    with Arena(regs) as A:
        if entry == "plain":
            L.call("tstwo_fri_fold_circle_into_line", A.p4(d_), N // 2, A.p4(s_), n, A.ptr("itw"), tw_log, L.u32x(ALPHA))
        elif entry == "dev":
            L.call("tstwo_fri_fold_circle_into_line_dev", A.p4(d_), N // 2, A.p4(s_), n, A.ptr("itw"), tw_log, A.ptr("alpha"))
        else:
            L.call("tstwo_fri_fold_circle_into_line_tw", A.p4(d_), N // 2, A.p4(s_), n, A.ptr("itw"), L.u32x(ALPHA))
        got = A.check()
    exp = orc.fold_circle_into_line(dst, src, n, half_initial, ALPHA)
    for j in range(4):
        assert eq(got[d_[j]], exp[j]), j


def shards(n_out):
    return [(0, 4), (4, 4), (n_out // 2 - 4, 8), (n_out - 4, 4)]


@pytest.mark.parametrize("shard", range(4))
@pytest.mark.parametrize("k", [6, 12])
def test_fri_fold_line_rows(k, shard):
    """A row shard of a line fold: `out` is a region the size of the whole output layer, pre-filled; the shard's rows become
    the oracle's, every other row keeps what was uploaded."""
    n = 1 << k
    row_offset, n_rows = shards(n // 2)[shard]
    cols, old = soa(200 + 4 * k, n), soa(250 + 4 * k, n // 2)
    tw_log, coset_initial, itw = _line_setup(k)
    i_, o_ = names("in"), names("out")
    regs = [rin(x, c) for x, c in zip(i_, cols)] + [rin("itw", itw)] + [rinout(x, c) for x, c in zip(o_, old)]
    with Arena(regs) as A:
        L.call("tstwo_fri_fold_line_rows", L.p4([A.addr(x, 8 * row_offset) for x in i_]), k, row_offset, n_rows, A.ptr("itw"), tw_log,
               L.u32x(ALPHA), L.p4([A.addr(x, 4 * row_offset) for x in o_]))
        got = A.check()
    full = orc.fold_line(cols, k, coset_initial, ALPHA)
    for j in range(4):
        exp = old[j].copy()
        exp[row_offset:row_offset + n_rows] = full[j][row_offset:row_offset + n_rows]
        assert eq(got[o_[j]], exp), j


@pytest.mark.parametrize("shard", range(4))
@pytest.mark.parametrize("n", [6, 12])
def test_fri_fold_circle_into_line_rows(n, shard):
    """A row shard of a circle fold: the shard's rows of `dst` are updated as the oracle updates them, the others keep their
    old values."""
    N = 1 << n
    row_offset, n_rows = shards(N // 2)[shard]
    src, dst = soa(300 + 4 * n, N), soa(400 + 4 * n, N // 2)
    tw_log = n + 1
    half_initial = (half_odds(n + 1) << 2) & 0x7FFFFFFF
    s_, d_ = names("src"), names("dst")
    regs = [rinout(x, c) for x, c in zip(d_, dst)] + [rin(x, c) for x, c in zip(s_, src)] + [rin("itw", otwiddles(tw_log)[1])]
    with Arena(regs) as A:
        L.call("tstwo_fri_fold_circle_into_line_rows", L.p4([A.addr(x, 4 * row_offset) for x in d_]),
               L.p4([A.addr(x, 8 * row_offset) for x in s_]), n, row_offset, n_rows, A.ptr("itw"), tw_log, L.u32x(ALPHA))
        got = A.check()
    full = orc.fold_circle_into_line(dst, src, n, half_initial, ALPHA)
    for j in range(4):
        exp = dst[j].copy()
        exp[row_offset:row_offset + n_rows] = full[j][row_offset:row_offset + n_rows]
        assert eq(got[d_[j]], exp), j


# ------------------------------------------------------------------ Blake2s Merkle
def layers_bytes(max_log):
    nbytes = L.lib().tstwo_merkle_layers_bytes(max_log)
    assert nbytes == 32 * ((2 << max_log) - 1)
    return nbytes


MERKLE_SHAPES = [(c, lg) for c in (0, 1, 15, 16, 17, 32, 33, 48, 64, 65) for lg in (0, 1, 5, 9, 10)]


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("n_cols,log", MERKLE_SHAPES)
def test_merkle_commit_layer(n_cols, log, with_prev):
    cols = soa(600 + log, 1 << log, n_cols)
    c_ = names("col", n_cols)
    prev = np.random.default_rng(700 + log).integers(0, 256, size=(2 << log, 32), dtype=np.uint8) if with_prev else None
    regs = [rin(k, c) for k, c in zip(c_, cols)] + ([rin("prev", prev)] if with_prev else []) + [Region("out", "out", nbytes=32 << log)]
    with Arena(regs) as A:
        L.call("tstwo_merkle_commit_layer", log, A.ptr("prev") if with_prev else C.c_void_p(0), A.ptrs(c_), n_cols, A.ptr("out"))
        got = A.check(np.uint8)
    assert eq(got["out"].reshape(-1, 32), orc.commit_on_layer(log, prev, cols))


def _merkle_commit(cols, logs):
    """One tree: the layers region has exactly tstwo_merkle_layers_bytes(max log) bytes."""
    c_ = names("col", len(cols))
    max_log = max(logs) if logs else 0
    root = (C.c_uint8 * 32)()
    with Arena([rin(k, c) for k, c in zip(c_, cols)] + [Region("layers", "out", nbytes=layers_bytes(max_log))]) as A:
        L.call("tstwo_merkle_commit", A.ptrs(c_), L.u32x(logs), len(cols), A.ptr("layers"), root)
        got = A.check(np.uint8)
    olayers, oroot = orc.merkle_commit(cols, logs)
    assert bytes(root) == oroot
    assert eq(got["layers"].reshape(-1, 32), np.concatenate(olayers))


@pytest.mark.parametrize("n_cols,log", MERKLE_SHAPES + [(32, 16), (48, 16), (32, 17), (48, 17)])
def test_merkle_commit(n_cols, log):
    """Up to log 10 the small-tree kernels; 32 and 48 columns at log 16 and 17 the static leaf, subtree and quad kernels."""
    _merkle_commit(soa(600 + log, 1 << log, n_cols), [log] * n_cols)


def test_merkle_commit_mixed_sizes():
    logs = [12, 12, 10, 10, 10, 4]
    _merkle_commit([rand_column(650 + i, 1 << lg) for i, lg in enumerate(logs)], logs)


@pytest.mark.parametrize("shape", ["equal", "unequal"])
def test_merkle_commit_many(shape):
    """3 equal trees of 16 columns of 2^17 (the shared launches) and 3 unequal ones (tree by tree): each layers buffer is a region
    of its own."""
    trees = [[(17, 16)] * 3, [(10, 3), (12, 17), (5, 1)]][shape == "unequal"]
    cols = [soa(5000 + 100 * t, 1 << lg, nc) for t, (lg, nc) in enumerate(trees)]
    regs = []
    for t, (lg, nc) in enumerate(trees):
        regs += [rin(f"t{t}c{i}", c) for i, c in enumerate(cols[t])]
    regs += [Region(f"layers{t}", "out", nbytes=layers_bytes(lg)) for t, (lg, _) in enumerate(trees)]
    reqs = (L.CommitRequest * 3)()
    roots = (C.c_uint8 * 96)()
    keep = []
    with Arena(regs) as A:
        for t, (lg, nc) in enumerate(trees):
            cp, lgs = A.ptrs([f"t{t}c{i}" for i in range(nc)]), L.u32x([lg] * nc)
            keep += [cp, lgs]
            reqs[t] = L.CommitRequest(cp, lgs, nc, A.addr(f"layers{t}"))
        L.call("tstwo_merkle_commit_many", reqs, 3, roots)
        got = A.check(np.uint8)
    for t, (lg, nc) in enumerate(trees):
        olayers, oroot = orc.merkle_commit(cols[t], [lg] * nc)
        assert bytes(roots[32 * t:32 * t + 32]) == oroot, t
        assert eq(got[f"layers{t}"].reshape(-1, 32), np.concatenate(olayers)), t


# ------------------------------------------------------------------ quotients
def _points(k, golden):
    px, py = golden["eval_at_point"][0]["point"]
    pts = [(tuple(px), tuple(py))]
    for _ in range(k - 1):                 # further points on the QM31 circle: repeated doubling
        x, y = pts[-1]
        x2 = OL.orc_qm31_mul(orc.q(x), orc.q(x)).tup()
        xy = OL.orc_qm31_mul(orc.q(x), orc.q(y)).tup()
        pts.append((tuple((2 * a - (1 if i == 0 else 0)) % P for i, a in enumerate(x2)), tuple((2 * a) % P for a in xy)))
    return pts


def _quotient_consts(random_coeff, batches):
    """The per-batch constants of tstwo_quotients_accumulate, from the oracle's line-coefficient helper."""
    off, cidx, abc, bcoef, prx, pry, pix, piy = [0], [], [], [], [], [], [], []
    for px, py, cv in batches:
        alpha = (1, 0, 0, 0)
        for ci, v in cv:
            alpha = OL.orc_qm31_mul(orc.q(alpha), orc.q(random_coeff)).tup()
            out = (orc.QM31 * 3)()
            OL.orc_line_coeffs(orc.SPoint(orc.q(px), orc.q(py)), orc.q(v), orc.q(alpha), out)
            for t in out:
                abc += list(t.tup())
            cidx.append(ci)
        off.append(len(cidx))
        bcoef += list(alpha)
        prx += px[:2]; pry += py[:2]; pix += px[2:]; piy += py[2:]
    return off, cidx, abc, bcoef, prx, pry, pix, piy


QUOT_CASES = [(nb, nc) for nb in (1, 2, 3, 4, 5) for nc in (1, 5)] + [("two-lists", 5)]


@pytest.mark.parametrize("batches_kind,n_cols", QUOT_CASES)
@pytest.mark.parametrize("log", [1, 2, 3, 4, 6, 9])
@pytest.mark.parametrize("entry", ["tstwo_quotients_accumulate", "tstwo_quotients_accumulate_async",
                                   "tstwo_quotients_accumulate_samples", "tstwo_quotients_accumulate_samples_async"])
def test_quotients(entry, log, batches_kind, n_cols, golden):
    """1 to 5 sample batches over one column list (k_quotients8, _multi<2>, _rp<3>, _rp<4>, the ACCUM continuation) and two batches
    over different lists (the per-batch kernel)."""
    cols = soa(900 + log * 8, 1 << log, n_cols)
    val = lambda j: tuple(int(x) for x in rand_column(950 + j, 4))
    if batches_kind == "two-lists":
        pts = _points(2, golden)
        lists = [[0, 1, 2], [3, 4]]
    else:
        pts = _points(batches_kind, golden)
        lists = [list(range(n_cols))] * batches_kind
    batches, j = [], 0
    for (bx, by), cl in zip(pts, lists):
        cv = []
        for c in cl:
            cv.append((c, val(j)))
            j += 1
        batches.append((bx, by, cv))
    rc = (5, 6, 7, 8)
    half = half_odds(log - 1)
    c_, o_ = names("col", n_cols), names("out")
    with Arena([rin(k, c) for k, c in zip(c_, cols)] + [rout(k, 1 << log) for k in o_]) as A:
        if "samples" in entry:
            off, cidx, points, values = [0], [], [], []
            for bx, by, cv in batches:
                points += [*bx, *by]
                for ci, v in cv:
                    cidx.append(ci)
                    values += list(v)
                off.append(len(cidx))
            L.call(entry, half, log, A.ptrs(c_), n_cols, len(batches), L.u32x(off), L.u32x(cidx), L.u32x(points), L.u32x(values),
                   L.u32x(rc), A.p4(o_))
        else:
            off, cidx, abc, bcoef, prx, pry, pix, piy = _quotient_consts(rc, batches)
            L.call(entry, half, log, A.ptrs(c_), n_cols, len(batches), L.u32x(off), L.u32x(cidx), L.u32x(abc), L.u32x(bcoef),
                   L.u32x(prx), L.u32x(pry), L.u32x(pix), L.u32x(piy), A.p4(o_))
        if entry.endswith("_async"):
            L.call("tstwo_check_zero_flag")
        got = A.check()
    exp = orc.accumulate_quotients(half, log, cols, rc, batches)
    for k in range(4):
        assert eq(got[o_[k]], exp[k]), k


# ------------------------------------------------------------------ copy, zero, upload at an offset
BYTE_COUNTS = [4, 12, 16, 20, 4092, 4096, 4100]


COPY_ENTRIES = ["tstwo_copy", "tstwo_zero", "tstwo_upload", "tstwo_upload_async", "tstwo_allgather", "tstwo_allgather_async"]


def _copy_like(entry, nbytes, place):
    """dst starts with other bytes than it must end with; the gathers run without a communicator (a world of one: a device copy)."""
    data = np.random.default_rng(nbytes).integers(0, 256, size=nbytes, dtype=np.uint8)
    o = offs(place, ["src"], ["dst"])
    has_src = entry in ("tstwo_copy", "tstwo_allgather", "tstwo_allgather_async", "tstwo_allgather_roots")
    regs = [Region("dst", "inout", data=data[::-1].copy(), offset=o["dst"])] + ([rin("src", data, o["src"])] if has_src else [])
    with Arena(regs) as A:
        exp = data
        if entry == "tstwo_copy":
            L.call(entry, A.ptr("dst"), A.ptr("src"), nbytes)
        elif entry == "tstwo_zero":
            L.call(entry, A.ptr("dst"), nbytes)
            exp = np.zeros(nbytes, dtype=np.uint8)
        elif entry == "tstwo_upload":
            L.call(entry, A.ptr("dst"), data.ctypes.data_as(C.c_void_p), nbytes)
        elif entry == "tstwo_upload_async":
            L.call(entry, A.ptr("dst"), data.ctypes.data_as(C.c_void_p), nbytes)
            L.call("tstwo_upload_wait")
        elif entry == "tstwo_allgather":
            L.call(entry, A.ptr("src"), A.ptr("dst"), nbytes)
        elif entry == "tstwo_allgather_async":
            L.call(entry, A.ptr("src"), A.ptr("dst"), nbytes)
            L.call("tstwo_comm_wait")
        else:
            assert entry == "tstwo_allgather_roots" and nbytes == 32
            L.call(entry, A.ptr("src"), A.ptr("dst"))
        got = A.check(np.uint8)
    assert eq(got["dst"], exp)


@pytest.mark.parametrize("place", ["aligned", "all+4", "out+4", "in+4"])
@pytest.mark.parametrize("nbytes", BYTE_COUNTS)
@pytest.mark.parametrize("entry", COPY_ENTRIES)
def test_copy_zero_upload_gather(entry, nbytes, place):
    _copy_like(entry, nbytes, place)


@pytest.mark.parametrize("place", ["aligned", "all+4"])
def test_allgather_roots(place):
    _copy_like("tstwo_allgather_roots", 32, place)


# ------------------------------------------------------------------ grid caps: a second trip through the grid-stride loop
# One case per capped launcher at the smallest ragged n that sends lanes through their grid-stride loop a second time on a
# 256-CU part: cap * 256 * W + 256 * W * 3 + 3 (cap blocks of 256 lanes of W elements, three more blocks, three odd elements).
def test_grid_cap_m31_mul():
    """launch_binop: cap = n_cus * 64 blocks, W = 4: 2^24 + 3072 + 3; k_m31_binop_vec4 wraps, the scalar tail takes the last 3."""
    n = N_CUS * 64 * 256 * 4 + 256 * 4 * 3 + 3
    assert n == (1 << 24) + 3075
    _m31_op("mul", n, "aligned", seed=7)


def test_grid_cap_qm31_mul():
    """k_qm31_mul: capped_blocks = n_cus * 64, W = 1: 2^22 + 768 + 3."""
    _qm31_mul(N_CUS * 64 * 256 + 256 * 3 + 3, "aligned")


@pytest.mark.parametrize("kernel", ["vec", "scalar"])
def test_grid_cap_secure_accumulate(kernel):
    """k_secure_accumulate<true> (n % 4 == 0, W = 4: 2^24 + 3072, the ragged 3 would select the scalar kernel) and
    k_secure_accumulate<false> (W = 1: 2^22 + 771, ragged), both capped at n_cus * 64 blocks."""
    n = N_CUS * 64 * 256 * 4 + 256 * 4 * 3 if kernel == "vec" else N_CUS * 64 * 256 + 256 * 3 + 3
    _secure_accumulate(n, "aligned")


@pytest.mark.parametrize("kernel", ["vec", "scalar"])
def test_grid_cap_fri_decompose(kernel):
    """k_decompose_apply<true> (n % 8 == 0, W = 4: 2^24 + 3072) and k_decompose_apply<false> (W = 1: 2^22 + 771, ragged), capped
    at n_cus * fold_cap = n_cus * 64 blocks."""
    n = N_CUS * 64 * 256 * 4 + 256 * 4 * 3 if kernel == "vec" else N_CUS * 64 * 256 + 256 * 3 + 3
    _decompose(n, "aligned")


def test_grid_cap_poly_extend():
    """k_extend<true>: cap n_cus * 64 blocks of 256 lanes of 4 words = 2^24 words; sizes are powers of two, so log_dst = 25 is
    the first at which lanes take a second trip (source 2^24: the second trip is all zero fill)."""
    _extend(24, 25, "aligned")


def test_grid_cap_fri_fold_line():
    """k_fold_line: one output row per lane, cap n_cus * fold_cap * 256 = 2^22 rows, so log_n = 24 (2^23 output rows) is the first
    layer whose lanes take a second trip.  The oracle's own fold (a domain point and a Fermat inverse per row) takes 15 s at this
    size, so the payload is checked against the oracle's column arithmetic instead, with a base-field alpha a: per coordinate
    out = (f0 + f1) + a * x^-1 * (f0 - f1) (fri.ts:120-152), x^-1 being the oracle's inverse twiddles; the same composition is
    first checked against the oracle's fold at log 10."""
    a = 19283

    def composed(cols, inv_x):
        ax = orc.col_op("mul", inv_x, np.full(inv_x.size, a, dtype=np.uint32))
        return [orc.col_op("add", orc.col_op("add", c[0::2], c[1::2]), orc.col_op("mul", ax, orc.col_op("sub", c[0::2], c[1::2]))) for c in cols]

    small = soa(77, 1 << 10)
    for g, e in zip(composed(small, otwiddles(10)[1][:1 << 9]), orc.fold_line(small, 10, half_odds(10), (a, 0, 0, 0))):
        assert eq(g, e)
    k = 24
    tw = orc.precompute_twiddles(half_odds(k), k, inverse=False)[0]
    itw = orc.m31_batch_inverse(tw)          # every x of the tree is nonzero: the elementwise inverses, as precomputeTwiddles gives
    big = rand_column(78, 4 << k)
    cols = [big[j << k:(j + 1) << k] for j in range(4)]
    i_, o_ = names("in"), names("out")
    with Arena([rin(x, c) for x, c in zip(i_, cols)] + [rin("itw", itw)] + [rout(x, 1 << (k - 1)) for x in o_]) as A:
        L.call("tstwo_fri_fold_line", A.p4(i_), k, A.ptr("itw"), k, L.u32x((a, 0, 0, 0)), A.p4(o_))
        got = A.check()
    exp = composed(cols, itw[:1 << (k - 1)])
    for j in range(4):
        assert eq(got[o_[j]], exp[j]), j


def test_grid_cap_air_wide_fib_trace():
    """k_wide_fib_trace<4>: grid_for caps at n_cus * 16 blocks of 256 lanes of 4 rows = 2^22 rows; sizes are powers of two, so
    log_n = 23 is the first trace whose lanes take a second trip.  Three columns: a, b and one computed."""
    _wide_fib(23, 3, "aligned")


# ------------------------------------------------------------------ line interpolation (the last FRI layer)
@pytest.mark.parametrize("k", list(range(0, 13)))
def test_line_interpolate(k):
    """Against LineEvaluation.interpolate as the reference formulates it (per-element inverses, on the host), as
    test_gpu_backend.test_line_interpolate_on_device_equals_reference_formulation does."""
    import tstwo_amd as T
    from tstwo_amd.fri_prover import line_interpolate_words
    cols = soa(7100 + 10 * k, 1 << k)
    coset = T.Coset.half_odds(13).repeated_double(13 - k)
    ev = T.LineEvaluation(T.LineDomain(coset), T.SecureColumnByCoords.from_numpy(cols))
    want = line_interpolate_words(ev, None)
    i_, o_ = names("in"), names("out")
    with Arena([rin(x, c) for x, c in zip(i_, cols)] + [rin("itw", otwiddles(13)[1])] + [rout(x, 1 << k) for x in o_]) as A:
        L.call("tstwo_line_interpolate", A.p4(i_), k, A.ptr("itw"), 13, A.p4(o_))
        got = A.check()
    for j in range(4):
        assert eq(got[o_[j]], want[j]), j


# ------------------------------------------------------------------ Poseidon252
import poseidon_model as PM  # noqa: E402


def _felts(rng, n):
    return [int.from_bytes(rng.bytes(32), "little") % PM.P for _ in range(n)]


def _felt_words(xs):
    return np.array([w for x in xs for w in PM.to_words(x)], dtype=np.uint32)


@pytest.mark.parametrize("felts_per_msg", [1, 2, 3])
@pytest.mark.parametrize("n_msgs", [1, 2, 63, 64, 65, 257])
def test_poseidon252_hash_many(n_msgs, felts_per_msg):
    rng = np.random.default_rng(100 * n_msgs + felts_per_msg)
    msgs = [_felts(rng, felts_per_msg) for _ in range(n_msgs)]
    with Arena([rin("in", _felt_words([x for m in msgs for x in m])), rout("out", 8 * n_msgs)]) as A:
        L.call("tstwo_poseidon252_hash_many", A.ptr("in"), n_msgs, felts_per_msg, A.ptr("out"))
        got = A.check()
    assert eq(got["out"], _felt_words([PM.hash_many(m) for m in msgs]))


POSEIDON_SHAPES = [(c, lg) for c in (1, 8, 9, 17) for lg in (0, 1, 4, 6)]


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("n_cols,log", POSEIDON_SHAPES)
def test_poseidon252_merkle_commit_layer(n_cols, log, with_prev):
    rng = np.random.default_rng(1000 + 37 * n_cols + log)
    cols = soa(1200 + log, 1 << log, n_cols)
    prev = _felts(rng, 2 << log) if with_prev else None
    c_ = names("col", n_cols)
    regs = [rin(k, c) for k, c in zip(c_, cols)] + ([rin("prev", _felt_words(prev))] if with_prev else []) + [rout("out", 8 << log)]
    with Arena(regs) as A:
        L.call("tstwo_poseidon252_merkle_commit_layer", log, A.ptr("prev") if with_prev else C.c_void_p(0), A.ptrs(c_), n_cols, A.ptr("out"))
        got = A.check()
    want = [PM.hash_node((prev[2 * i], prev[2 * i + 1]) if with_prev else None, [int(c[i]) for c in cols]) for i in range(1 << log)]
    assert eq(got["out"], _felt_words(want))


@pytest.mark.parametrize("n_cols,log", POSEIDON_SHAPES)
def test_poseidon252_merkle_commit(n_cols, log):
    cols = soa(1300 + log, 1 << log, n_cols)
    c_ = names("col", n_cols)
    root = (C.c_uint8 * 32)()
    with Arena([rin(k, c) for k, c in zip(c_, cols)] + [Region("layers", "out", nbytes=layers_bytes(log))]) as A:
        L.call("tstwo_poseidon252_merkle_commit", A.ptrs(c_), L.u32x([log] * n_cols), n_cols, A.ptr("layers"), root)
        got = A.check()
    expect = PM.commit([c.tolist() for c in cols])                      # expect[k] = layer k, root first
    assert eq(got["layers"], _felt_words([x for lg in range(log + 1) for x in expect[lg]]))
    assert PM.from_words([int(w) for w in np.frombuffer(bytes(root), dtype="<u4")]) == expect[0][0]


# ------------------------------------------------------------------ GKR / MLE
import gkr_model as GM  # noqa: E402

GKR_KINDS = [GM.GP, GM.GENERIC, GM.MULT, GM.SINGLES]


def u32cols(a):
    """The coordinate columns of a model array: (4, n) secure or (n,) base."""
    a = np.asarray(a)
    return [a.astype(np.uint32)] if a.ndim == 1 else [a[k].astype(np.uint32) for k in range(a.shape[0])]


def regs_of(prefix, a, role, off=0):
    cols = u32cols(a)
    ns = names(prefix, len(cols))
    return ns, [Region(n, role, data=c, offset=off) for n, c in zip(ns, cols)]


def outs_of(prefix, n, off=0):
    ns = names(prefix)
    return ns, [rout(x, n, off) for x in ns]


def secure_eq(got, ns, want):
    return all(eq(got[n], np.asarray(want[k]).astype(np.uint32)) for k, n in enumerate(ns))


def gkr_layer(rng, kind, n_vars):
    n = 1 << n_vars
    num = {GM.GENERIC: GM.random_secure(rng, n), GM.MULT: GM.random_base(rng, n)}.get(kind)
    return {"kind": kind, "num": num, "den": GM.random_secure(rng, n)}


def num_p4(A, kind, ns):
    """The `num` table as the header describes it: 4 columns (generic), only num[0] read (multiplicities), not read (singles)."""
    if kind == GM.GENERIC:
        return A.p4(ns)
    if kind == GM.MULT:
        return L.p4([A.addr(ns[0])] * 4)
    return L.p4([0] * 4)


@pytest.mark.parametrize("place", ["aligned", "out+4"])
@pytest.mark.parametrize("n_y", [0, 1, 2, 3, 4, 5, 12])
def test_gkr_gen_eq_evals(n_y, place):
    """k_eq_expand<4> from n_y = 4 (lo >= 2) with aligned outputs, k_eq_expand<1> below and for offset outputs."""
    rng = np.random.default_rng(100 + n_y)
    y = [GM.random_felt(rng) for _ in range(n_y)]
    v = GM.random_felt(rng)
    o_, regs = outs_of("out", 1 << n_y, 4 if place == "out+4" else 0)
    with Arena(regs) as A:
        L.call("tstwo_gkr_gen_eq_evals", L.u32x([w for t in y for w in t]), n_y, L.u32x(v), A.p4(o_))
        got = A.check()
    assert secure_eq(got, o_, GM.gen_eq_evals_loop(y, v) if n_y <= 8 else GM.gen_eq_evals(y, v))


@pytest.mark.parametrize("place", ["aligned", "all+4"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 11])
@pytest.mark.parametrize("kind", GKR_KINDS)
def test_gkr_next_layer(kind, n, place):
    rng = np.random.default_rng(1000 * kind + n)
    lay = gkr_layer(rng, kind, n)
    off = 4 if place == "all+4" else 0
    d_, regs = regs_of("den", lay["den"], "in", off)
    n_ = []
    if lay["num"] is not None:
        n_, r = regs_of("num", lay["num"], "in", off)
        regs += r
    od_, r = outs_of("oden", 1 << (n - 1), off)
    regs += r
    on_ = []
    if kind != GM.GP:
        on_, r = outs_of("onum", 1 << (n - 1), off)
        regs += r
    with Arena(regs) as A:
        if kind == GM.GP:
            L.call("tstwo_gkr_next_layer_grand_product", A.p4(d_), n, A.p4(od_))
        else:
            L.call("tstwo_gkr_next_layer_logup", kind, num_p4(A, kind, n_), A.p4(d_), n, A.p4(on_), A.p4(od_))
        got = A.check()
    want = GM.next_layer(lay)
    assert secure_eq(got, od_, want["den"])
    if kind != GM.GP:
        assert secure_eq(got, on_, want["num"])


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 11])
@pytest.mark.parametrize("is_base", [False, True])
def test_mle_fix_first_variable(is_base, n, place):
    """k_fold<BASE, 4> when half % 4 == 0 and everything is aligned, k_fold<BASE, 1> otherwise."""
    rng = np.random.default_rng(2000 + 100 * is_base + n)
    col = GM.random_base(rng, 1 << n) if is_base else GM.random_secure(rng, 1 << n)
    r = GM.random_felt(rng)
    i_ = names("in", 1 if is_base else 4)
    o = offs(place, i_, names("out"))
    regs = [rin(x, c, o[x]) for x, c in zip(i_, u32cols(col))] + [rout(x, 1 << (n - 1), o[x]) for x in names("out")]
    with Arena(regs) as A:
        if is_base:
            L.call("tstwo_mle_fix_first_variable_base", A.ptr(i_[0]), n, L.u32x(r), A.p4(names("out")))
        else:
            L.call("tstwo_mle_fix_first_variable_secure", A.p4(i_), n, L.u32x(r), A.p4(names("out")))
        got = A.check()
    assert secure_eq(got, names("out"), GM.fix_first_variable(col, r))


@pytest.mark.parametrize("place", ["aligned", "all+4"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 11])
def test_mle_fix_first_variable_secure_in_place(n, place):
    """out == in: the lower half becomes the folded MLE, the upper half is read, never written."""
    rng = np.random.default_rng(3000 + n)
    col = GM.random_secure(rng, 1 << n)
    r = GM.random_felt(rng)
    c_, regs = regs_of("col", col, "inout", 4 if place == "all+4" else 0)
    with Arena(regs) as A:
        L.call("tstwo_mle_fix_first_variable_secure", A.p4(c_), n, L.u32x(r), A.p4(c_))
        got = A.check()
    half = 1 << (n - 1)
    want = np.concatenate([GM.fix_first_variable(col, r), col[:, half:]], axis=1)
    assert secure_eq(got, c_, want)


@pytest.mark.parametrize("n_vars", [1, 2, 3, 11])
@pytest.mark.parametrize("kind", GKR_KINDS)
def test_gkr_sum_poly_async(kind, n_vars):
    """The 8-word (f(0), f(2)) result is a region of its own."""
    rng = np.random.default_rng(4000 + 100 * kind + n_vars)
    lay = gkr_layer(rng, kind, n_vars + 1)
    eq_cols = GM.random_secure(rng, 1 << (n_vars - 1))
    lam = GM.random_felt(rng)
    e_, regs = regs_of("eq", eq_cols, "in")
    d_, r = regs_of("den", lay["den"], "in")
    regs += r
    n_ = []
    if lay["num"] is not None:
        n_, r = regs_of("num", lay["num"], "in")
        regs += r
    regs.append(rout("result", 8))
    with Arena(regs) as A:
        L.call("tstwo_gkr_sum_poly_async", kind, A.p4(e_), num_p4(A, kind, n_), A.p4(d_), n_vars, L.u32x(lam), A.ptr("result"))
        got = A.check()
    f0, f2 = GM.sum_f0_f2(lay, eq_cols, n_vars, lam)
    assert tuple(int(w) for w in got["result"]) == tuple(f0) + tuple(f2)


@pytest.mark.parametrize("n_vars", [1, 2, 3, 11])
@pytest.mark.parametrize("kind", GKR_KINDS)
def test_gkr_round(kind, n_vars):
    """tstwo_gkr_round out of place: the layer (2^(n_vars + 2) values) is an input, the folded columns are regions of half that
    length, the 8-word result a region of its own."""
    rng = np.random.default_rng(5000 + 100 * kind + n_vars)
    lay = gkr_layer(rng, kind, n_vars + 2)
    eq_cols = GM.random_secure(rng, 1 << (n_vars - 1))
    lam, r = GM.random_felt(rng), GM.random_felt(rng)
    half = 1 << (n_vars + 1)
    e_, regs = regs_of("eq", eq_cols, "in")
    d_, rr = regs_of("den", lay["den"], "in")
    regs += rr
    n_ = []
    if lay["num"] is not None:
        n_, rr = regs_of("num", lay["num"], "in")
        regs += rr
    od_, rr = outs_of("oden", half)
    regs += rr
    on_ = []
    if lay["num"] is not None:
        on_, rr = outs_of("onum", half)
        regs += rr
    regs.append(rout("result", 8))
    with Arena(regs) as A:
        L.call("tstwo_gkr_round", kind, A.p4(e_), num_p4(A, kind, n_), A.p4(d_), A.p4(on_) if on_ else L.p4([0] * 4), A.p4(od_), n_vars,
               L.u32x(r), L.u32x(lam), A.ptr("result"))
        got = A.check()
    folded = {"kind": GM.GENERIC if kind == GM.MULT else kind,
              "num": GM.fix_first_variable(lay["num"], r) if lay["num"] is not None else None,
              "den": GM.fix_first_variable(lay["den"], r)}
    f0, f2 = GM.sum_f0_f2(folded, eq_cols, n_vars, lam)
    assert tuple(int(w) for w in got["result"]) == tuple(f0) + tuple(f2)
    assert secure_eq(got, od_, folded["den"])
    if on_:
        assert secure_eq(got, on_, folded["num"])


# ------------------------------------------------------------------ AIR and LogUp
import air_model as AM  # noqa: E402
import air_program_model as XM  # noqa: E402
import logup_model as LM  # noqa: E402

AIR_LOGS = [1, 2, 3, 5, 10]


def rand_felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def _wide_fib(log, n_cols, place):
    rng = np.random.default_rng(log)
    a, b = rng.integers(0, P, size=1 << log, dtype=np.uint32), rng.integers(0, P, size=1 << log, dtype=np.uint32)
    c_ = names("col", n_cols)
    o = offs(place, ["a", "b"], c_)
    with Arena([rin("a", a, o["a"]), rin("b", b, o["b"])] + [rout(x, 1 << log, o[x]) for x in c_]) as A:
        L.call("tstwo_air_wide_fib_trace", A.ptr("a"), A.ptr("b"), log, A.ptrs(c_), n_cols)
        got = A.check()
    want = AM.wide_fib_trace(a.astype(np.uint64), b.astype(np.uint64), n_cols)
    for x, w in zip(c_, want):
        assert eq(got[x], w.astype(np.uint32)), x


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("n_cols", [3, 17])
@pytest.mark.parametrize("log", AIR_LOGS)
def test_air_wide_fib_trace(log, n_cols, place):
    _wide_fib(log, n_cols, place)


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("log", AIR_LOGS)
@pytest.mark.parametrize("kind,n_cols", [(AM.WIDE_FIB, 3), (AM.WIDE_FIB, 4), (AM.MUL_ADD, 3)])
def test_air_constraint_quotients(kind, n_cols, log, place):
    """The smallest constraint sets of test_gpu_air.py (3 and 4 wide-Fibonacci columns, mul-add), log_expand 1; accum is added to."""
    log_expand = 1
    rng = np.random.default_rng(1000 + 37 * log + n_cols + log_expand)
    n = 1 << (log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    coeffs = [rand_felt(rng) for _ in range(AM.n_constraints(kind, n_cols))]
    dinv = AM.denom_inv(log, log + log_expand)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    c_, a_ = names("col", n_cols), names("acc")
    o = offs(place, c_, a_)
    regs = [rin(x, c.astype(np.uint32), o[x]) for x, c in zip(c_, cols)] + [rinout(x, pre[j].astype(np.uint32), o[x]) for j, x in enumerate(a_)]
    with Arena(regs) as A:
        L.call("tstwo_air_constraint_quotients", 1 if kind == AM.MUL_ADD else 0, A.ptrs(c_), n_cols, log, log_expand,
               L.u32x([w for c in coeffs for w in c]), len(coeffs), L.u32x([int(d) for d in dinv]), A.p4(a_))
        got = A.check()
    assert secure_eq(got, a_, AM.quotients_on_domain(kind, cols, log, log_expand, coeffs, dinv, pre))


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("log", AIR_LOGS)
def test_air_eval_program(log, place):
    """The random straight-line programs of test_gpu_constraint_framework.py (6 columns, 5 constraints, 40 operations, row offsets
    up to 3), log_expand 1."""
    log_expand, n_cols, n_constraints = 1, 6, 5
    rng = np.random.default_rng(7 * log + log_expand)
    n = 1 << (log + log_expand)
    cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_cols)]
    words = XM.random_program(rng, n_cols, n_constraints, 40, max_offset=3)
    coeffs = [rand_felt(rng) for _ in range(n_constraints)]
    dinv = AM.denom_inv(log, log + log_expand)
    pre = rng.integers(0, P, size=(4, n), dtype=np.uint64)
    c_, a_ = names("col", n_cols), names("acc")
    o = offs(place, c_, a_)
    regs = [rin(x, c.astype(np.uint32), o[x]) for x, c in zip(c_, cols)] + [rinout(x, pre[j].astype(np.uint32), o[x]) for j, x in enumerate(a_)]
    with Arena(regs) as A:
        L.call("tstwo_air_eval_program", A.ptrs(c_), n_cols, log, log_expand, L.u32x(words), len(words) // 2,
               L.u32x([w for c in coeffs for w in c]), n_constraints, L.u32x([int(d) for d in dinv]), A.p4(a_))
        got = A.check()
    assert secure_eq(got, a_, XM.eval_program_on_domain(words, cols, log, log_expand, coeffs, dinv, pre))


# (log, fractions, terms per denominator, column numerator, prev): the smallest cases of test_gpu_logup.py, one per log
LOGUP_CASES = [(1, 1, 1, False, False), (2, 1, 2, True, True), (3, 2, 1, True, False), (5, 8, 16, True, True), (10, 2, 2, True, True)]


@pytest.mark.parametrize("place", ["aligned", "all+4", "out+4"])
@pytest.mark.parametrize("log,n_fracs,n_terms,col_num,with_prev", LOGUP_CASES)
def test_logup_column(log, n_fracs, n_terms, col_num, with_prev, place):
    rng = np.random.default_rng(1000 + 7 * log + n_fracs)
    n = 1 << log
    in_off, out_off = (4 if place == "all+4" else 0), (4 if place in ("all+4", "out+4") else 0)
    regs, fr, model = [], [], []
    for f in range(n_fracs):
        cols = [rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(n_terms)]
        coeffs = [rand_felt(rng) for _ in range(n_terms)]
        const = rand_felt(rng)
        den = np.zeros((4, n), dtype=np.uint64)
        for j in range(4):
            den[j] = const[j]
            for c, co in zip(cols, coeffs):
                den[j] = (den[j] + co[j] * c) % P
        t_ = [f"f{f}t{t}" for t in range(n_terms)]
        regs += [rin(x, c.astype(np.uint32), in_off) for x, c in zip(t_, cols)]
        if col_num:
            num = rng.integers(0, P, size=n, dtype=np.uint64)
            regs.append(rin(f"f{f}num", num.astype(np.uint32), in_off))
            num_const = 0
        else:
            num_const = int(rng.integers(0, P))
            num = np.full(n, num_const, dtype=np.uint64)
        fr.append((t_, coeffs, const, num_const))
        model.append((num, den))
    prev = rng.integers(0, P, size=(4, n), dtype=np.uint64) if with_prev else None
    p_ = []
    if with_prev:
        p_, r = regs_of("prev", prev, "in", in_off)
        regs += r
    o_, r = outs_of("out", n, out_off)
    regs += r
    descs, keep = (L.LogupFrac * n_fracs)(), []
    with Arena(regs) as A:
        for f, (t_, coeffs, const, num_const) in enumerate(fr):
            tab, cw = A.ptrs(t_), L.u32x([w for co in coeffs for w in co])
            keep += [tab, cw]
            d = descs[f]
            d.cols, d.coeffs, d.n_terms = C.cast(tab, C.POINTER(L.vp)), C.cast(cw, L.u32p), n_terms
            d.constant[:] = list(const)
            d.num, d.num_const = (A.addr(f"f{f}num") if col_num else None), num_const
        L.call("tstwo_logup_column", descs, n_fracs, A.p4(p_) if with_prev else None, log, A.p4(o_))
        L.call("tstwo_check_zero_flag")
        got = A.check()
    assert secure_eq(got, o_, LM.column(model, prev, n))


@pytest.mark.parametrize("place", ["aligned", "all+4"])
@pytest.mark.parametrize("log", AIR_LOGS)
def test_logup_finalize_last(log, place):
    rng = np.random.default_rng(50 + log)
    col = rng.integers(0, P, size=(4, 1 << log), dtype=np.uint64)
    want, claimed = LM.finalize_last(col, log)
    c_, regs = regs_of("col", col, "inout", 4 if place == "all+4" else 0)
    out = (C.c_uint32 * 4)()
    with Arena(regs) as A:
        L.call("tstwo_logup_finalize_last", A.p4(c_), log, out)
        got = A.check()
    assert tuple(out) == tuple(claimed)
    assert secure_eq(got, c_, want)


# ------------------------------------------------------------------ the device channel and the FRI commit loop
def _host_channel():
    from tstwo_amd.channel import Blake2sChannel
    ch = Blake2sChannel()
    ch.mix_u64(12345)
    return ch


def _chan_words(ch):
    st = np.zeros(10, dtype=np.uint32)
    st[:8] = np.frombuffer(ch.digest(), dtype="<u4")
    st[8], st[9] = ch.n_challenges, ch.n_sent
    return st


@pytest.mark.parametrize("what", ["root", "felt", "both"])
def test_channel_mix_root_draw_felt(what):
    """chan (10 words), root (32 bytes, read only) and felt (4 words) are three regions; against the host Blake2sChannel (hashlib)."""
    ref = _host_channel()
    root = bytes((7 * 3 + k) & 0xFF for k in range(32))
    regs = [rinout("chan", _chan_words(ref))]
    if what != "felt":
        regs.append(rin("root", np.frombuffer(root, dtype=np.uint8)))
    if what != "root":
        regs.append(rout("felt", 4))
    with Arena(regs) as A:
        L.call("tstwo_channel_mix_root_draw_felt", A.ptr("chan"), A.ptr("root") if what != "felt" else C.c_void_p(0),
               A.ptr("felt") if what != "root" else C.c_void_p(0))
        got = A.check()
    if what != "felt":
        ref.mix_root(root)
    if what != "root":
        assert tuple(int(w) for w in got["felt"]) == ref.draw_felt().tup()
    assert eq(got["chan"], _chan_words(ref))


# (col_logs, last, the step kinds of tests/fri_plan.py the schedule holds beside the first tree and the first fold): the two
# single columns first, then the smallest inputs that take each branch of the schedule
FRI_COMMIT_CASES = [
    pytest.param([10], 2, {"TAIL"}, id="10"),                                       # every line layer in the one-workgroup tail
    pytest.param([14], 2, {"COMMIT", "FOLD_COMMIT", "TAIL+pre"}, id="14"),          # four layers of separate launches first
    pytest.param([3], 2, set(), id="3-last2"),                                      # no inner layer
    pytest.param([4], 2, {"TAIL"}, id="4-last2"),                                   # tail at once, no pre-fold
    pytest.param([4, 3], 2, {"COMMIT", "FOLD_LINE", "CIRCLE_ACCUM"}, id="4.3-last2"),          # separate commit, line fold, a column joining at the last layer
    pytest.param([6, 4], 2, {"COMMIT", "FOLD_COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "TAIL"}, id="6.4-last2"),       # fused at 2^4 rows, join, tail without pre-fold
    pytest.param([11], 9, {"COMMIT", "FOLD_LINE"}, id="11-last9"),                  # no tail at all
    pytest.param([12], 9, {"COMMIT", "FOLD_COMMIT", "FOLD_LINE"}, id="12-last9"),   # fused, then a plain fold into the last layer
    pytest.param([13, 12], 2, {"COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "FOLD_COMMIT", "TAIL+pre"}, id="13.12-last2"),   # join at the first inner layer, fused, tail with pre-fold
]


def _fri_commit_arena(col_logs, tw_log, cap):
    """(regions, names of the 4 n coordinate columns, the columns, the host channel) of a commit over circle columns of col_logs"""
    ref = _host_channel()
    cols = [soa(8100 + 40 * j + c, 1 << c) for j, c in enumerate(col_logs)]
    c_ = [x for j in range(len(col_logs)) for x in names(f"col{j}_")]
    regs = [rin(x, c) for x, c in zip(c_, [c for col in cols for c in col])]
    regs += [rin("itw", otwiddles(tw_log)[1]), rinout("chan", _chan_words(ref)), rout("alphas", 4 * cap)]
    return regs, c_, cols, ref


@pytest.mark.parametrize("col_logs,last,kinds", FRI_COMMIT_CASES)
def test_fri_commit_layers(col_logs, last, kinds):
    """The whole commit loop on circle evaluations of col_logs (log 10: every line layer in the one-workgroup tail; log 14: four
    layers of separate launches first; the others: the smallest inputs that take each branch of the schedule, which the case first
    checks it takes, by tests/fri_plan.py), down to a last layer of 2^last rows.  The columns, the twiddles, the 10-word channel and
    the alphas (capacity = trees + 3) are regions; the loop is replayed on the CPU -- the oracle's trees and folds, a joining column
    folded into the current layer with the same alpha, the host channel -- and the channel, every alpha, every returned evaluation
    and tree must match; the alpha entries past the count keep the sentinel."""
    from arena import SENTINEL
    import fri_plan
    assert fri_plan.kinds(col_logs, last) == kinds | {"FIRST_TREE", "CIRCLE_WRITE"}
    log = col_logs[0]
    tw_log = log + 1
    half_initial = lambda c: (half_odds(tw_log) << (tw_log - c + 1)) & 0x7FFFFFFF      # of the canonic domain of log c
    n_trees = 1 + (log - 1 - last)
    cap = n_trees + 3
    regs, c_, cols, ref = _fri_commit_arena(col_logs, tw_log, cap)
    outs, n_out, first = (L.FriLayerOut * (n_trees + 1))(), C.c_size_t(0), L.vp()
    with Arena(regs) as A:
        L.call("tstwo_fri_commit_layers", A.ptrs(c_), L.u32x(col_logs), len(col_logs), A.ptr("itw"), tw_log, last, A.ptr("chan"),
               A.ptr("alphas"), cap, C.byref(first), outs, n_trees + 1, C.byref(n_out))
        got = A.check()
        owned = [L.DeviceBuffer.adopt(first.value, layers_bytes(log))]
        dev_layers = []
        for i in range(n_out.value):
            lg = outs[i].log_size
            ev = [L.DeviceBuffer.adopt(outs[i].cols[k], 4 << lg) for k in range(4)]
            tree = L.DeviceBuffer.adopt(outs[i].layers, layers_bytes(lg)) if outs[i].layers else None
            owned += ev + ([tree] if tree else [])
            dev_layers.append((lg, [e.download() for e in ev], tree.download(np.uint8).reshape(-1, 32) if tree else None))
        first_tree = owned[0].download(np.uint8).reshape(-1, 32)
        for b in owned:
            b.free()
    # the same loop on the CPU
    alphas = []
    olayers, oroot = orc.merkle_commit([c for col in cols for c in col], [c for c in col_logs for _ in range(4)])
    assert eq(first_tree, np.concatenate(olayers))
    ref.mix_root(oroot)
    alphas.append(ref.draw_felt().tup())
    cur = orc.fold_circle_into_line(orc.soa_alloc(1 << (log - 1)), cols[0], log, half_initial(log), alphas[-1])
    joining = {c - 1: col for c, col in zip(col_logs[1:], cols[1:])}          # line layer log -> the circle column that joins it
    assert n_out.value == n_trees
    for i, lg in enumerate(range(log - 1, last, -1)):
        dlg, dev_ev, dev_tree = dev_layers[i]
        assert dlg == lg and all(eq(dev_ev[k], cur[k]) for k in range(4)), lg
        olayers, oroot = orc.merkle_commit(cur, [lg] * 4)
        assert eq(dev_tree, np.concatenate(olayers)), lg
        ref.mix_root(oroot)
        alphas.append(ref.draw_felt().tup())
        cur = orc.fold_line(cur, lg, (half_odds(tw_log) << (tw_log - lg)) & 0x7FFFFFFF, alphas[-1])
        if lg - 1 in joining:
            cur = orc.fold_circle_into_line(cur, joining.pop(lg - 1), lg, half_initial(lg), alphas[-1])
    assert not joining
    dlg, dev_ev, dev_tree = dev_layers[-1]
    assert dlg == last and dev_tree is None and all(eq(dev_ev[k], cur[k]) for k in range(4))
    assert len(alphas) == n_trees
    assert eq(got["alphas"][:4 * n_trees], np.array(alphas, dtype=np.uint32).reshape(-1))
    assert (got["alphas"][4 * n_trees:] == SENTINEL).all()
    assert eq(got["chan"], _chan_words(ref))


def test_fri_commit_layers_too_few_twiddles():
    """a twiddle tree one level short of the first fold (tw_log = col_logs[0] - 2): the error comes back before anything is
    allocated or launched -- the channel is bit for bit its input, every alpha entry the sentinel, nothing is returned"""
    from arena import SENTINEL
    col_logs, last = [13, 12], 2
    tw_log = col_logs[0] - 2
    n_trees = 1 + (col_logs[0] - 1 - last)
    regs, c_, _, ref = _fri_commit_arena(col_logs, tw_log, n_trees + 3)
    outs, n_out, first = (L.FriLayerOut * (n_trees + 1))(), C.c_size_t(7), L.vp(1)
    with Arena(regs) as A:
        with pytest.raises(L.TstwoError, match="Not enough twiddles!"):
            L.call("tstwo_fri_commit_layers", A.ptrs(c_), L.u32x(col_logs), len(col_logs), A.ptr("itw"), tw_log, last, A.ptr("chan"),
                   A.ptr("alphas"), n_trees + 3, C.byref(first), outs, n_trees + 1, C.byref(n_out))
        got = A.check()
    assert eq(got["chan"], _chan_words(ref))
    assert (got["alphas"] == SENTINEL).all()
    assert n_out.value == 0 and not first.value

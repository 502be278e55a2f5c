"""tstwo_eval_at_points on the MI355X: columns of mixed sizes, each group at up to 16 out-of-domain points, in one call.  Every
value is compared bit for bit with oracle.eval_at_point and with the unchanged tstwo_eval_at_point as a second witness; the
shapes are those of tests/eval_points_plan.py (tests/test_cpu_eval_points_plan.py shows that they reach every branch of the
plan).  Then the refusals, guard bands, call sequences over the shared scratch block and result pages, the Python wrapper,
prove_values and an AIR proof with a LogUp component."""
import ctypes as C
import functools

import numpy as np
import pytest

import arena as AR
import eval_points_plan as EP
import saturation as S
import sequence as SQ
from conftest import P, rand_column
from gpu_util import dev
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import tstwo_amd as T  # noqa: E402
from tstwo_amd import _lib as L  # noqa: E402
from tstwo_amd import pcs as PCS  # noqa: E402
from tstwo_amd import poly as POLY  # noqa: E402

SENT = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def points(k, first=0):
    """k distinct points on the QM31 circle, as ((x words), (y words))."""
    return list(SQ._sample_points(first + k)[first:])


@functools.lru_cache(maxsize=None)
def column(seed, log):
    c = rand_column(seed, 1 << log)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def device_column(seed, log):
    """Aligned device copies, shared by the tests of this module and never written."""
    return dev(column(seed, log))


@functools.lru_cache(maxsize=None)
def reference(seed, log, pt):
    return orc.eval_at_point(column(seed, log), log, pt[0], pt[1])


def one_point_entry(addr, log, pt):
    out = (C.c_uint32 * 4)()
    L.call("tstwo_eval_at_point", C.c_void_p(addr), log, L.u32x(pt[0]), L.u32x(pt[1]), out)
    return tuple(out)


def eval_at_points(groups, out=None, lib_call=None):
    """groups = [(log, [device addresses], [points])] -> [array (cols, points, 4) per group]: one tstwo_eval_at_points call."""
    addrs = [a for _, cols, _ in groups for a in cols]
    words = [w for _, _, pts in groups for x, y in pts for w in (*x, *y)]
    n_out = sum(len(cols) * len(pts) for _, cols, pts in groups)
    if out is None:
        out = np.full(4 * max(n_out, 1), SENT, dtype=np.uint32)
    (lib_call or L.call)("tstwo_eval_at_points", L.ptr_array(addrs), L.u32x([len(cols) for _, cols, _ in groups]), L.u32x([lg for lg, _, _ in groups]),
                         L.u32x([len(pts) for _, _, pts in groups]), len(groups), L.u32x(words), out.ctypes.data_as(L.u32p))
    res, o = [], 0
    for _, cols, pts in groups:
        n = 4 * len(cols) * len(pts)
        res.append(out[o:o + n].reshape(len(cols), len(pts), 4))
        o += n
    return res


def check_group(got, seeds, log, pts, witness_addrs=None):
    assert got.shape == (len(seeds), len(pts), 4)
    for i, seed in enumerate(seeds):
        for k, pt in enumerate(pts):
            want = reference(seed, log, pt)
            assert tuple(int(w) for w in got[i, k]) == want, (log, i, k)
            if witness_addrs is not None:
                assert one_point_entry(witness_addrs[i], log, pt) == want, (log, i, k)


# ------------------------------------------------------------------ one group, aligned
@pytest.mark.parametrize("log,cols,k", EP.one_group_shapes())
def test_one_group_aligned(log, cols, k):
    seeds = [7000 + 10 * log + i for i in range(cols)]
    addrs = [device_column(s, log).ptr for s in seeds]
    assert all(a % 16 == 0 for a in addrs)
    pts = points(k)
    (got,) = eval_at_points([(log, addrs, pts)])
    check_group(got, seeds, log, pts, witness_addrs=addrs)


def test_g4_branch():
    """log 16 x 64 columns at 2 points: the 4-group tile on a 256-CU plan (tests/eval_points_plan.py)."""
    (log, cols, k, _), = EP.gpu_calls()["g4"]
    assert EP.plan(log, cols, k, True).g == 4
    seeds = [7600 + i for i in range(cols)]
    addrs = [device_column(s, log).ptr for s in seeds]
    pts = points(k, first=3)
    (got,) = eval_at_points([(log, addrs, pts)])
    check_group(got, seeds, log, pts, witness_addrs=addrs)


def test_three_level_branch():
    """One column of 2^27 coefficients at 2 points, against tstwo_eval_at_point only; the words come from a seeded generator."""
    (log, cols, k, _), = EP.gpu_calls()["three-levels"]
    assert EP.plan(log, cols, k, True).levels == 3
    words = np.random.default_rng(27).integers(0, P, size=1 << log, dtype=np.uint32)
    buf = dev(words)
    try:
        pts = points(k, first=5)
        (got,) = eval_at_points([(log, [buf.ptr], pts)])
        for j, pt in enumerate(pts):
            assert tuple(int(w) for w in got[0, j]) == one_point_entry(buf.ptr, log, pt), j
        assert tuple(got[0, 0]) != tuple(got[0, 1])
    finally:
        buf.free()
        L.call("tstwo_trim")


def test_result_region_in_scratch_and_column_slabs():
    """More results than the page-locked page holds (1100 columns x 4 points; the same 5 columns over and over: a column may
    appear twice), and more columns than one launch takes (8200 constant polynomials)."""
    (log, cols, k, _), = EP.gpu_calls()["result-in-scratch"]
    assert not EP.result_pinned(cols * k)
    seeds = [7700 + (i % 5) for i in range(cols)]
    pts = points(k)
    (got,) = eval_at_points([(log, [device_column(s, log).ptr for s in seeds], pts)])
    check_group(got, seeds, log, pts)
    (log, cols, k, _), = EP.gpu_calls()["slabs"]
    assert EP.plan(log, cols, k, True).slabs == 2 and log == 0
    consts = rand_column(7800, cols)
    buf = dev(consts)
    (got,) = eval_at_points([(0, [buf.ptr + 4 * i for i in range(cols)], points(k))])
    assert (got[:, 0, 0] == consts).all() and not got[:, :, 1:].any()
    buf.free()


# ------------------------------------------------------------------ alignment and guard bands
def _arena_call(shapes, pts_of):
    """shapes = [(log, [byte offset per column])]: the columns sit in one guarded arena; returns after checking the guards."""
    regions, groups, seeds = [], [], []
    for g, (log, offsets) in enumerate(shapes):
        ss = [7900 + 100 * g + i for i in range(len(offsets))]
        seeds.append(ss)
        regions += [AR.rin(f"g{g}c{i}", column(s, log), off) for i, (s, off) in enumerate(zip(ss, offsets))]
    with AR.Arena(regions) as A:
        for g, (log, offsets) in enumerate(shapes):
            groups.append((log, [A.addr(f"g{g}c{i}") for i in range(len(offsets))], pts_of(g)))
        got = eval_at_points(groups)
        A.check()                                   # the guard bands and the coefficient columns are what was uploaded
        for g, (log, offsets) in enumerate(shapes):
            check_group(got[g], seeds[g], log, groups[g][2], witness_addrs=groups[g][1])


@pytest.mark.parametrize("log", [5, 13])
def test_columns_at_a_4_byte_offset(log):
    _arena_call([(log, [4, 4])], lambda g: points(2))


def test_one_unaligned_column_among_aligned_ones():
    _arena_call([(13, [0, 4, 0]), (13, [0, 0])], lambda g: points(2, first=g))


@pytest.mark.parametrize("log,k", [(0, 2), (5, 4), (12, 5), (13, 3), (14, 16)])
def test_guard_bands(log, k):
    _arena_call([(log, [0, 0, 0])], lambda g: points(k))


# ------------------------------------------------------------------ several groups in one call
def test_several_groups_in_one_call():
    shapes = EP.gpu_calls()["mixed"]
    assert [(lg, c, k) for lg, c, k, _ in shapes] == [(6, 3, 1), (13, 2, 3), (0, 2, 2), (12, 70, 2)]
    groups, seeds = [], []
    for g, (log, cols, k, _) in enumerate(shapes):
        ss = [8100 + 100 * g + i for i in range(cols)]
        if g == 3:
            ss[5] = ss[0]                                    # the same column twice in one group ...
        seeds.append(ss)
        groups.append((log, [device_column(s, log).ptr for s in ss], points(k, first=g)))
    # ... and one column present in two groups: a second group of log 13 at other points
    seeds.append([seeds[1][1]])
    groups.append((13, [groups[1][1][1]], points(2, first=7)))
    got = eval_at_points(groups)
    for g, (log, _, pts) in enumerate(groups):
        check_group(got[g], seeds[g], log, pts)
    # the output order is (group, column, point): the flat words are the groups' blocks one after the other
    flat = np.concatenate([g.reshape(-1) for g in got])
    want = [w for g, (log, _, pts) in enumerate(groups) for s in seeds[g] for pt in pts for w in reference(s, log, pt)]
    assert flat.tolist() == want


# ------------------------------------------------------------------ saturation
@pytest.mark.parametrize("log", [5, 12, 14])
@pytest.mark.parametrize("cfam", ["S", "E"])
def test_saturated_operands(log, cfam):
    coeffs = S.eval_coeffs(log, cfam)
    pts = [S.eval_point("S", log), S.eval_point("E", log), S.eval_point("circle", log), S.eval_point("S", log)]
    pts = [(tuple(int(w) for w in x), tuple(int(w) for w in y)) for x, y in pts]
    buf = dev(coeffs)
    (got,) = eval_at_points([(log, [buf.ptr], pts)])
    for k, (x, y) in enumerate(pts):
        want = orc.eval_at_point(coeffs, log, x, y)
        assert tuple(int(w) for w in got[0, k]) == want, k
        assert one_point_entry(buf.ptr, log, (x, y)) == want, k
    buf.free()


# ------------------------------------------------------------------ repeated points
def test_repeated_points_and_point_order():
    a, b, c = points(3)
    log, seeds = 13, [8500, 8501]
    addrs = [device_column(s, log).ptr for s in seeds]
    pts = [a, b, a, c, b, a]
    (got,) = eval_at_points([(log, addrs, pts)])
    check_group(got, seeds, log, pts)
    assert (got[:, 0] == got[:, 2]).all() and (got[:, 0] == got[:, 5]).all() and (got[:, 1] == got[:, 4]).all()
    (rev,) = eval_at_points([(log, addrs, pts[::-1])])
    assert (rev == got[:, ::-1]).all()


# ------------------------------------------------------------------ refusals
def _refused(text, *args):
    out = np.full(64, SENT, dtype=np.uint32)
    with pytest.raises(L.TstwoError) as e:
        L.call("tstwo_eval_at_points", *args, out.ctypes.data_as(L.u32p))
    assert str(e.value) == text and e.value.code != 0
    assert (out == SENT).all()


def test_refusals_leave_out_untouched():
    buf = device_column(8600, 5)
    cols, pt = L.ptr_array([buf.ptr, buf.ptr]), points(1)[0]
    one = L.u32x([*pt[0], *pt[1]])
    many = L.u32x([*pt[0], *pt[1]] * 17)
    u = L.u32x
    none32 = nonep = None
    _refused("eval_at_points: null argument", nonep, u([1]), u([5]), u([1]), 1, one)
    _refused("eval_at_points: null argument", cols, none32, u([5]), u([1]), 1, one)
    _refused("eval_at_points: null argument", cols, u([1]), none32, u([1]), 1, one)
    _refused("eval_at_points: null argument", cols, u([1]), u([5]), none32, 1, one)
    _refused("eval_at_points: null argument", cols, u([1]), u([5]), u([1]), 1, none32)
    _refused("eval_at_points: null argument", L.ptr_array([buf.ptr, 0]), u([2]), u([5]), u([1]), 1, one)
    with pytest.raises(L.TstwoError, match="eval_at_points: null argument"):
        L.call("tstwo_eval_at_points", cols, u([1]), u([5]), u([1]), 1, one, none32)
    _refused("eval_at_points: a group without columns", cols, u([1, 0]), u([5, 5]), u([1, 1]), 2, many)
    _refused("eval_at_points: 1 to 16 points per group", cols, u([1]), u([5]), u([0]), 1, one)
    _refused("eval_at_points: 1 to 16 points per group", cols, u([1]), u([5]), u([17]), 1, many)
    _refused("eval_at_points: log size out of range", cols, u([1, 1]), u([5, 32]), u([1, 1]), 2, many)
    for word in range(8):
        w = [*pt[0], *pt[1]]
        w[word] = P
        _refused("eval_at_points: point word out of range", cols, u([1]), u([5]), u([1]), 1, u(w))
    # during graph capture: the handling of tstwo_mle_eval_at_point_base
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        _refused("eval_at_points: host read-back during graph capture (the values cannot be recorded)", cols, u([1]), u([5]), u([1]), 1, one)
    finally:
        g = L.vp()
        L.call("tstwo_graph_end_capture", C.byref(g))
        L.call("tstwo_graph_destroy", g)
    # n_groups == 0 is a no-op, whatever the other arguments are
    out = np.full(4, SENT, dtype=np.uint32)
    L.call("tstwo_eval_at_points", nonep, none32, none32, none32, 0, none32, out.ctypes.data_as(L.u32p))
    assert (out == SENT).all()
    # and the library still answers
    (got,) = eval_at_points([(5, [buf.ptr], [pt])])
    check_group(got, [8600], 5, [pt])


# ------------------------------------------------------------------ sequences over the shared scratch block and result pages
def test_between_other_users_of_the_scratch_and_the_result_page():
    """tstwo_fri_decompose (scratch), the call, tstwo_eval_at_point_batch (scratch, page-locked page), tstwo_download_many (the
    mapped result page), back to back; every result is checked."""
    s = SQ.Seq()
    rng = np.random.default_rng(41)
    n = 1 << 13
    in4 = SQ.rand_cols(s, rng, 4, n)
    out4 = s.bufs(4, n)
    small = SQ.rand_cols(s, rng, 70, 1 << 6)
    state = s.initial_state()
    A = SQ.Arena(s)
    try:
        L.sync()
        lam = (C.c_uint32 * 4)()
        L.call("tstwo_fri_decompose", L.p4([A.addr(x) for x in in4]), n, L.p4([A.addr(x) for x in out4]), lam)
        pa, pb = points(3), points(2, first=4)
        got = eval_at_points([(13, [A.addr(x) for x in in4], pa), (6, [A.addr(x) for x in small], pb)])
        batch = np.zeros(4 * 4, dtype=np.uint32)
        L.call("tstwo_eval_at_point_batch", L.ptr_array([A.addr(x) for x in in4]), 4, 13, L.u32x(pa[1][0]), L.u32x(pa[1][1]), batch.ctypes.data_as(L.u32p))
        pieces = L.download_many([(A.addr(in4[0]), 1000), (A.addr(small[3]), 64)])
        image = A.download()
    finally:
        A.free()
    exp, elam = orc.decompose([state[x] for x in in4])
    assert tuple(lam) == elam
    after = s.split(image)
    for k in range(4):
        assert (after[out4[k]] == exp[k]).all() and (after[in4[k]] == state[in4[k]]).all()
    for i, x in enumerate(in4):
        for k, pt in enumerate(pa):
            assert tuple(int(w) for w in got[0][i, k]) == orc.eval_at_point(state[x], 13, pt[0], pt[1]), (i, k)
        assert tuple(int(w) for w in batch[4 * i:4 * i + 4]) == orc.eval_at_point(state[x], 13, pa[1][0], pa[1][1])
    for i, x in enumerate(small):
        for k, pt in enumerate(pb):
            assert tuple(int(w) for w in got[1][i, k]) == orc.eval_at_point(state[x], 6, pt[0], pt[1]), (i, k)
    assert (pieces[0] == state[in4[0]][:1000]).all() and (pieces[1] == state[small[3]]).all()


def test_two_calls_where_the_second_needs_more_scratch():
    """The second call holds its 65600 results in scratch (more than a MiB, the block's first size) behind the same partials."""
    log, seeds = 13, [8700, 8701]
    addrs = [device_column(s, log).ptr for s in seeds]
    pts = points(2)
    n_const, k_const = EP.SLAB_COLS + 8, 8
    first = [(log, 2, 2, True)]
    second = first + [(0, n_const, k_const, True)]
    assert EP.call_scratch_qm31(first) < EP.call_scratch_qm31(second) and 16 * EP.call_scratch_qm31(second) > 1 << 20
    consts = rand_column(8702, n_const)
    buf = dev(consts)
    a = np.full(4 * 4, SENT, dtype=np.uint32)
    b = np.full(4 * (4 + n_const * k_const), SENT, dtype=np.uint32)
    (g1,) = eval_at_points([(log, addrs, pts)], out=a)
    g2, g3 = eval_at_points([(log, addrs, pts), (0, [buf.ptr + 4 * i for i in range(n_const)], points(k_const))], out=b)
    (g4,) = eval_at_points([(log, addrs, pts)])
    buf.free()
    for g in (g1, g2, g4):
        check_group(g, seeds, log, pts)
    assert (g3[:, :, 0] == consts[:, None]).all() and not g3[:, :, 1:].any()


# ------------------------------------------------------------------ the wrapper
def _cpoint(pt):
    return T.CirclePoint(T.QM31.from_u32_unchecked(*pt[0]), T.QM31.from_u32_unchecked(*pt[1]))


def _counting(monkeypatch):
    names = []
    real = L.call

    def counted(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", counted)
    return names


def test_wrapper_makes_one_call(monkeypatch):
    a, b, c = (_cpoint(p) for p in points(3))
    polys = [T.HipCirclePoly(rand_column(8800 + i, 1 << lg)) for i, lg in enumerate([4, 6, 7, 6, 4, 7])]
    point_sets = [[a], [a, b], [a, b, c], [a, b], [b], [c, b, a]]
    want = [[p.evalAtPoint(pt).tup() for pt in pts] for p, pts in zip(polys, point_sets)]
    names = _counting(monkeypatch)
    got = T.HipCirclePoly.eval_at_points(polys, point_sets)
    assert [n for n in names if "eval_at_point" in n] == ["tstwo_eval_at_points"]
    assert [[v.tup() for v in vs] for vs in got] == want
    assert T.HipCirclePoly.eval_at_points([], []) == [] and T.HipCirclePoly.eval_at_points(polys[:1], [[]]) == [[]]
    # a longer list is split into runs of 16 points
    many = [_cpoint(p) for p in points(POLY.EVAL_MAX_POINTS + 3)]
    (long,) = T.HipCirclePoly.eval_at_points(polys[1:2], [many])
    assert [v.tup() for v in long] == [polys[1].evalAtPoint(pt).tup() for pt in many]


# ------------------------------------------------------------------ prove_values and an AIR proof
def _flat(x):
    """A proof as nested plain data, field for field."""
    import dataclasses
    if dataclasses.is_dataclass(x) and not isinstance(x, type):
        return {f.name: _flat(getattr(x, f.name)) for f in dataclasses.fields(x)}
    if hasattr(x, "tup"):
        return x.tup()
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (bytes, bytearray, str, int, float, bool)) or x is None:
        return x
    if isinstance(x, dict):
        return {k: _flat(v) for k, v in x.items()}
    if hasattr(x, "__iter__"):
        return [_flat(v) for v in x]
    if hasattr(x, "__dict__"):
        return {k: _flat(v) for k, v in vars(x).items()}
    return x


def _per_point(polys, point_sets):
    """eval_at_points as the parent commit sampled: one tstwo_eval_at_point_batch call per (column, point)."""
    return [[T.HipCirclePoly.eval_at_point_batch([p], pt)[0] for pt in pts] for p, pts in zip(polys, point_sets)]


def test_prove_values_samples_in_one_call(monkeypatch):
    from test_gpu_backend import _pcs_setup, _pcs_verifier
    config = T.PcsConfig(pow_bits=6, fri_config=T.FriConfig(1, 1, 6))
    logs = [[7, 6, 7], [6, 7]]

    def prove(patched, limit=None):
        scheme, ch = _pcs_setup(config, logs, seed=13000)
        point = T.CirclePoint.get_random_point(ch)
        sh1 = point.add(T.SECURE_FIELD_CIRCLE_GEN)
        sh2 = sh1.add(T.SECURE_FIELD_CIRCLE_GEN)
        pts = [[[point], [point, sh1], [point, sh1, sh2]], [[point, sh1], [point]]]
        with monkeypatch.context() as m:
            if patched:
                m.setattr(T.HipCirclePoly, "eval_at_points", staticmethod(_per_point))
            if limit is not None:
                m.setattr(PCS, "ONE_CALL_SAMPLING_MAX_COEFFS", limit)
            names = _counting(m)
            proof = scheme.prove_values(pts, ch)
        return proof, pts, ch, [n for n in names if "eval_at_point" in n]
    proof, pts, ch, calls = prove(False)
    assert calls == ["tstwo_eval_at_points"]                     # the sampling phase: one synchronous call
    old, _, old_ch, old_calls = prove(True)
    assert old_calls == ["tstwo_eval_at_point_batch"] * 9
    assert _flat(proof) == _flat(old) and ch.digest() == old_ch.digest()
    # an opening above the size limit keeps the batched call per (size, point): 5 such pairs here
    big, _, big_ch, big_calls = prove(False, limit=(1 << 7) - 1)
    assert big_calls == ["tstwo_eval_at_point_batch"] * 5
    assert _flat(big) == _flat(proof) and big_ch.digest() == ch.digest()
    v, vch = _pcs_verifier(config, logs, proof.commitments)
    vpoint = T.CirclePoint.get_random_point(vch)
    assert vpoint.x.tup() == pts[0][0][0].x.tup()
    v.verify_values(pts, proof, vch)
    assert vch.digest() == ch.digest()


def test_air_proof_with_logup_is_unchanged(monkeypatch):
    """StateMachineEval at log 6: row offsets and a LogUp interaction trace, so columns open at several points."""
    from test_gpu_interaction_trace import _closed_form, _state_machine_proof, _verify_state_machine
    names = _counting(monkeypatch)
    comp, proof, config, le = _state_machine_proof(6)
    assert [n for n in names if "eval_at_point" in n].count("tstwo_eval_at_points") == 1
    assert not [n for n in names if n in ("tstwo_eval_at_point", "tstwo_eval_at_point_batch")]
    with monkeypatch.context() as m:
        m.setattr(T.HipCirclePoly, "eval_at_points", staticmethod(_per_point))
        _, old, _, _ = _state_machine_proof(6)
    assert _flat(proof) == _flat(old)
    _verify_state_machine(comp, proof, config, _closed_form(6, le))

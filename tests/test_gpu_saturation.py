"""-m gpu: the lazy 64-bit accumulators at operands that reach their bounds.  Every case of tests/saturation.py (operand families
S, Z, H, E and their row mixes; tests/test_cpu_saturation.py shows on exact integers that each is accepted by its reference, is not
degenerate and reaches the bound it names) goes through the C ABI, and every output word is compared with the CPU oracle or the
integer models: batch inverses, quotients (raw constants and samples, every kernel of csrc/quotients.hip), the hand-written AIR
constraints, AIR programs, LogUp columns and the coset-order prefix sum, eval_at_point."""
import ctypes as C

import numpy as np
import pytest

import logup_model as LM
import saturation as S
from gpu_util import dev, host, p4, ptrs, vp
from oracle import oracle as orc
from tstwo_amd import _lib as L

pytestmark = pytest.mark.gpu

P = S.P


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def place(a, k):
    """A device buffer holding `a` behind k leading words (k = 1: the data is not 16-byte aligned); (buffer, pointer)."""
    buf = dev(np.concatenate([np.zeros(k, dtype=np.uint32), np.asarray(a, dtype=np.uint32)]))
    return buf, buf.ptr + 4 * k


def read(placed, k, n):
    return host(placed[0], n + k)[k:]


def same(got, want, what):
    want = np.asarray(want).astype(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first wrong word", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), "wrong words", int(bad.size))


def half_initial(log):
    return 1 << (31 - (log + 1))


# ------------------------------------------------------------------ batch inverses
@pytest.mark.parametrize("dim,n,aligned", S.INVERSE_CASES)
def test_batch_inverse_grid(dim, n, aligned):
    x = S.inverse_input(dim, n, aligned)
    k = 0 if aligned else 1
    din = [place(c, k) for c in x]
    dout = [place(np.zeros(n), k) for _ in range(dim)]
    pin, pout = [p for _, p in din], [p for _, p in dout]
    x32 = [c.astype(np.uint32) for c in x]
    if dim == 1:
        L.call("tstwo_m31_batch_inverse", C.c_void_p(pin[0]), C.c_void_p(pout[0]), n)
        want = [orc.m31_batch_inverse(x32[0])]
    elif dim == 2:
        L.call("tstwo_cm31_batch_inverse", L.P2(*pin), L.P2(*pout), n)
        zero = np.zeros(n, dtype=np.uint32)
        want = orc.qm31_batch_inverse([x32[0], x32[1], zero, zero])
        assert not want[2].any() and not want[3].any()
        want = want[:2]
    else:
        L.call("tstwo_qm31_batch_inverse", L.p4(pin), L.p4(pout), n)
        want = orc.qm31_batch_inverse(x32)
    for j in range(dim):
        same(read(dout[j], k, n), want[j], (S.inverse_kernel(dim, n, aligned), "coordinate", j))


# ------------------------------------------------------------------ quotients
@pytest.mark.parametrize("name,log,setting,family", S.quotient_case_ids())
def test_quotients_raw_constants(name, log, setting, family):
    c = S.quotient_case(name, log, setting, family)
    n, k = 1 << log, 0 if c["out_aligned"] else 1
    d = [dev(col) for col in c["cols"]]                     # (the columns must be 16-byte aligned: only the output may not be)
    out = [place(np.zeros(n), k) for _ in range(4)]
    flat = lambda vs: L.u32x([w for v in vs for w in v])
    L.call("tstwo_quotients_accumulate", half_initial(log), log, ptrs(d), len(d), len(c["lists"]), L.u32x(c["off"]), L.u32x(c["cidx"]),
           flat(c["abc"]), flat(c["coeff"]), flat(c["prx"]), flat(c["pry"]), flat(c["pix"]), flat(c["piy"]), L.p4([p for _, p in out]))
    want = S.quotient_expected(c)
    for j in range(4):
        same(read(out[j], k, n), want[j], (c["kernels"], "coordinate", j))


@pytest.mark.parametrize("name,log,setting,family", S.sample_case_ids())
def test_quotients_from_samples(name, log, setting, family):
    c = S.sample_case(name, log, setting, family)
    n, k = 1 << log, 0 if c["out_aligned"] else 1
    d = [dev(col) for col in c["cols"]]
    out = [place(np.zeros(n), k) for _ in range(4)]
    off, cidx, pts, vals = [0], [], [], []
    for px, py, cv in c["batches"]:
        pts += list(px) + list(py)
        for ci, v in cv:
            cidx.append(ci)
            vals += list(v)
        off.append(len(cidx))
    L.call("tstwo_quotients_accumulate_samples", half_initial(log), log, ptrs(d), len(d), len(c["batches"]), L.u32x(off), L.u32x(cidx),
           L.u32x(pts), L.u32x(vals), L.u32x(c["coeff"]), L.p4([p for _, p in out]))
    want = S.sample_expected(c)
    for j in range(4):
        same(read(out[j], k, n), want[j], (c["kernels"], "coordinate", j))


# ------------------------------------------------------------------ AIR
def _air_io(c):
    k = 0 if c["aligned"] else 1
    n = 1 << (c["trace_log"] + c["log_expand"])
    cols = [place(col, k) for col in c["cols"]]
    acc = [place(c["accum"][j], k) for j in range(4)]
    return k, n, cols, acc


@pytest.mark.parametrize("kind,n_constraints,log_expand,aligned,family", S.air_case_ids())
def test_air_constraint_quotients(kind, n_constraints, log_expand, aligned, family):
    c = S.air_case(kind, n_constraints, log_expand, aligned, family)
    k, n, cols, acc = _air_io(c)
    L.call("tstwo_air_constraint_quotients", 1 if kind == "mul_add" else 0, L.ptr_array([p for _, p in cols]), len(cols), c["trace_log"],
           log_expand, L.u32x([w for q in c["coeffs"] for w in q]), n_constraints, L.u32x(c["dinv"]), L.p4([p for _, p in acc]))
    want = S.air_expected(c)
    for j in range(4):
        same(read(acc[j], k, n), want[j], ("W = 4" if aligned else "W = 1", "coordinate", j))


@pytest.mark.parametrize("n_acc,way,log_expand,aligned", S.program_case_ids())
def test_air_program(n_acc, way, log_expand, aligned):
    c = S.program_case(n_acc, way, log_expand, aligned)
    k, n, cols, acc = _air_io(c)
    L.call("tstwo_air_eval_program", L.ptr_array([p for _, p in cols]), len(cols), c["trace_log"], log_expand, L.u32x(c["words"]),
           len(c["words"]) // 2, L.u32x([w for q in c["coeffs"] for w in q]), c["n_acc"], L.u32x(c["dinv"]), L.p4([p for _, p in acc]))
    want = S.program_expected(c)
    for j in range(4):
        same(read(acc[j], k, n), want[j], ("W = 4" if aligned else "W = 1", "coordinate", j))


# ------------------------------------------------------------------ LogUp
@pytest.mark.parametrize("n_terms,n_fracs,aligned,family", S.logup_case_ids())
def test_logup_column(n_terms, n_fracs, aligned, family):
    c = S.logup_case(n_terms, n_fracs, aligned, family)
    n, k = 1 << c["log"], 0 if aligned else 1
    keep, descs = [], (L.LogupFrac * n_fracs)()
    for d, f in zip(descs, c["fracs"]):
        dcols = [place(col, k) for col in f["cols"]]
        tab = L.ptr_array([p for _, p in dcols])
        cw = L.u32x([w for co in f["coeffs"] for w in co])
        keep += [dcols, tab, cw]
        d.cols, d.coeffs, d.n_terms = C.cast(tab, C.POINTER(L.vp)), C.cast(cw, L.u32p), n_terms
        d.constant[:] = list(f["constant"])
        if isinstance(f["num"], int):
            d.num, d.num_const = None, f["num"]
        else:
            num = place(f["num"], k)
            keep.append(num)
            d.num, d.num_const = num[1], 0
    prev = [place(c["prev"][j], k) for j in range(4)]
    out = [place(np.zeros(n), k) for _ in range(4)]
    L.call("tstwo_logup_column", descs, n_fracs, L.p4([p for _, p in prev]), c["log"], L.p4([p for _, p in out]))
    L.call("tstwo_check_zero_flag")
    want = S.logup_expected(c)
    for j in range(4):
        same(read(out[j], k, n), want[j], ("W = 4" if aligned else "W = 1", "coordinate", j))


@pytest.mark.parametrize("family", S.FINALIZE_FAMILIES)
@pytest.mark.parametrize("log", S.FINALIZE_LOGS)
def test_logup_finalize_last(log, family):
    col = S.finalize_case(log, family)
    n = 1 << log
    want, claimed = LM.finalize_last(col, log)
    d = [dev(col[j].astype(np.uint32)) for j in range(4)]
    out = (C.c_uint32 * 4)()
    L.call("tstwo_logup_finalize_last", p4(d), log, out)
    assert tuple(out) == claimed
    for j in range(4):
        same(host(d[j], n), want[j], ("coordinate", j))


# ------------------------------------------------------------------ eval_at_point
@pytest.mark.parametrize("log,cfam,pkind,aligned", S.eval_case_ids())
def test_eval_at_point(log, cfam, pkind, aligned):
    coeffs = S.eval_coeffs(log, cfam)
    px, py = S.eval_point(pkind, log)
    k = 0 if aligned else 1
    d = place(coeffs, k)
    out = (C.c_uint32 * 4)()
    L.call("tstwo_eval_at_point", C.c_void_p(d[1]), log, L.u32x(px), L.u32x(py), out)
    want = tuple(orc.eval_at_point(coeffs, log, px, py))
    assert tuple(out) == want
    # the batch entry point: the same column three times beside a uniform one
    other = np.random.default_rng(log).integers(0, P, size=1 << log, dtype=np.uint32)
    e = place(other, k)
    outb = (C.c_uint32 * 16)()
    L.call("tstwo_eval_at_point_batch", L.ptr_array([d[1], e[1], d[1], d[1]]), 4, log, L.u32x(px), L.u32x(py), outb)
    wo = tuple(orc.eval_at_point(other, log, px, py))
    assert tuple(outb) == want + wo + want + want


# ------------------------------------------------------------------ the randomised sweep's default draws
def test_fuzz_default_draws_are_unchanged():
    """fuzz_parity.run() with the default values="uniform" draws what it drew before the edge values existed: the messages of the
    first 200 cases of seed 20261004 (shapes, column counts, FRI / PCS configurations: every one a function of the random stream)
    hash to the digest recorded from the sweep as it was before that parameter was added."""
    import hashlib

    import fuzz_parity
    msgs = []
    assert fuzz_parity.run(seconds=600, seed=20261004, max_cases=200, verbose=False, messages=msgs) == 200
    text = "".join(m + "\n" for m in msgs)
    assert hashlib.sha256(text.encode()).hexdigest() == "df28b8bdf3cda6c686bf0e06f8c69930ab06ab5a9ea8d50d301864135432b7f8"

"""The saturation cases of tests/saturation.py are what they claim (no GPU): for every case tests/test_gpu_saturation.py runs, on
exact Python integers and the reference models,
  * the reference side accepts it (no "0 has no inverse"),
  * it is not degenerate: with 8 rows or more every output coordinate takes at least two values (the whole-constant-column
    families, which run once per site, are exempt: a constant input has a constant output),
  * it reaches the bound: the unreduced 64-bit sum of the kernel, restated here in integers, takes on at least one row the documented
    maximum the C ABI can reach (4 (P-1)^2 + the folded remainder; bit 63 set at the reduce<true> sites; within 2^35 below 2^63 at the
    reduce<false> sites) and never passes 2^64.
The restatements follow the kernels' own grouping (csrc/air.hip, logup.hip, quotients.hip, field_ops.hip, fri.hip, poly_eval.hip)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import air_model as M
import air_program_model as X
import logup_model as LM
import saturation as S
from gkr_model import qadd, qmul, qsub
from oracle import oracle as orc

P, SAT = S.P, S.SAT
U63, U64 = 1 << 63, 1 << 64
UNIT = SAT * SAT                                     # the largest product of two canonical words


def fold_air(x):
    """fold64 of csrc/air.hip and csrc/logup.hip: t1 + t2 + 2 t3"""
    assert x < U64
    return (x & P) + ((x >> 31) & 0xffffffff) + 2 * (x >> 63)


def fold_quot(x):
    """the fold of the LAZY quotient kernels: 2 hi + lo"""
    assert x < U64
    return 2 * (x >> 32) + (x & 0xffffffff)


def two_values(out, n_rows):
    """every output coordinate takes at least two values"""
    return n_rows < 8 or all(len(np.unique(np.asarray(c))) >= 2 for c in out)


# ---------------------------------------------------------------- the families
def test_families_are_what_they_claim():
    rng = np.random.default_rng(3)
    n = 4096
    assert (S.fam_s(rng, n) == SAT).all()
    assert set(S.fam_e(rng, n).tolist()) == set(S.EDGE) and max(S.EDGE) < P
    assert set(S.fam_z(rng, n).tolist()) == {0, SAT}
    a, b = S.h_pair(rng, n)
    assert set((a + b).tolist()) == {P, 2 * P - 2} and a.max() < P and b.max() < P
    assert {(P - 1) // 2, (P + 1) // 2, SAT} <= set(a.tolist())
    mask = S.half_mask(rng, n)
    assert mask.sum() == n // 2
    for fam in S.FAMILIES:
        c = S.column(fam, rng, n, mask)
        assert c.dtype == np.uint64 and c.max() < P
    c = S.column("mixS", rng, n, mask)
    assert (c[mask] == SAT).all() and len(np.unique(c[~mask])) > n // 4
    for w in (4, 8):                                     # lanes of 4 and of 8 rows hold both kinds of row
        assert any(0 < m < w for m in mask.reshape(-1, w).sum(axis=1))
    assert 4 * UNIT + (1 << 34) < U64 <= 5 * UNIT        # four products and a folded remainder fit; five products do not


# ---------------------------------------------------------------- batch inverses
def _norm_sums(a, b, c, d):
    """the unreduced sums of k_qm31_batch_inverse_norm for one element, and the values that follow from them"""
    dmc2, d2, b2, nb, nc, nd2 = 2 * ((d - c) % P), 2 * d, 2 * b, P - b, P - c, 2 * (P - d)
    re0, re1 = a * a + b * nb + c * dmc2, d * d2
    im0, im1 = a * b2 + c * nd2, c * nd2 + c * nc + d * d
    dr, di = (re0 + re1) % P, (im0 + im1) % P
    nn = dr * dr + di * di
    ninv = pow(nn % P, P - 2, P)
    ir, ii = dr * ninv % P, (P - di) * ninv % P
    nir, nii = P - ir, P - ii
    outs = (a * ir + b * nii, a * ii + b * ir, c * nir + d * ii, c * nii + d * nir)
    return dict(re0=re0, re1=re1, im0=im0, im1=im1, nn=nn, outs=outs, operands=(nb, nc, nd2, P - di, nir, nii),
                value=tuple(o % P for o in outs))


@pytest.mark.parametrize("dim,n,aligned", S.INVERSE_CASES)
def test_inverse_cases(dim, n, aligned):
    x = S.inverse_input(dim, n, aligned)
    assert x.shape == (dim, n) and x.max() < P and x.any(axis=0).all()
    kernel = S.inverse_kernel(dim, n, aligned)
    slots = S.inverse_slot(kernel, np.arange(n), n)
    vals = S.inverse_values(dim)
    assert len(S.grid_values(dim)) == 6 ** dim - 1
    for s in range(S.INVERSE_SLOTS[kernel]):               # every grid value in every lane slot
        have = {tuple(v) for v in x[:, slots == s].T.tolist()}
        assert {tuple(v) for v in vals.tolist()} <= have, (kernel, s)
    x32 = [c.astype(np.uint32) for c in x]
    if dim == 1:
        out = [orc.m31_batch_inverse(x32[0])]              # raises OracleError("0 has no inverse") on a rejected input
    elif dim == 2:
        out = orc.qm31_batch_inverse([x32[0], x32[1], np.zeros(n, np.uint32), np.zeros(n, np.uint32)])[:2]
    else:
        out = orc.qm31_batch_inverse(x32)
    assert two_values(out, n)
    if kernel != "qm31_norm":
        return
    sums = [_norm_sums(*(int(v) for v in x[:, i])) for i in range(n)]
    for i in (0, n // 2, n - 1):                           # the restatement computes the inverse
        assert sums[i]["value"] == tuple(int(o[i]) for o in out)
    mx = lambda k: max(s[k] for s in sums)
    assert mx("im0") == 2 * UNIT + 2 * P * SAT < U64       # a = b = c = P - 1, d = 0: 2 (P - d) = 2P
    assert U63 <= mx("re0") < U64
    # im1 = 2 c (P - d) + c (P - c) + d^2 is largest at c = P - 1, d = 0 (convex in d; at d = P - 1 it stays below 1.3 P^2): just
    # below 2^63, so reduce<true> is the safe side there and the grid reaches the true maximum
    assert U63 - (1 << 35) < mx("im1") == SAT * (2 * P + 1) < U63
    assert U63 - (1 << 35) < mx("re1") < U63               # reduce<false>
    assert U63 - (1 << 35) < mx("nn") < U63                # reduce<false>: the norm-saturating element
    # oa .. od (reduce<false>): two products, the second operand P - ir / P - ii possibly P itself.  The inverse's words are not the
    # caller's to choose, so two full units (2^63 - 2^34) cannot be forced: the element found by S.output_saturating_qm31 (a seeded
    # search over 4000 inverses, expected best 2 - O(4000^-1/2) units) carries oa above 1.9 units, and nothing passes 2^63
    assert 19 * UNIT // 10 < max(max(s["outs"]) for s in sums) < U63
    ir, ii = S.qm31_norm_inverse_words(*S.output_saturating_qm31())
    assert SAT * ir + SAT * (P - ii) in {s["outs"][0] for s in sums}
    ops = {o for s in sums for o in s["operands"]}
    assert P in ops and 2 * P in ops                       # P - 0 and 2 (P - 0) as multiplicands


# ---------------------------------------------------------------- quotients
def _numerator_sums(c, row):
    """the 64-bit numerator sums of one coordinate of `row`, group by group, as the kernels of c["kernels"] form them"""
    out = []
    lazy = not c["kernels"][0].startswith("q8") or c["kernels"][0].endswith("true>")
    for b in range(len(c["lists"])):
        acc = 0
        for j in range(c["off"][b], c["off"][b + 1], 4):
            group = sum(c["abc"][3 * e + 2][0] * int(c["cols"][c["cidx"][e]][row]) for e in range(j, min(j + 4, c["off"][b + 1])))
            acc = (fold_quot(acc) if lazy else acc % P) + group
            out.append(acc)
    return out


def _cmul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def _batch_sums(c, b, row):
    """Batch b at `row`, as the 8-row kernels form it: the denominator (da, db), its norm sum nn = da^2 + db^2 (reduce<false>), the
    inverse words (ir, ii), the four term sums U V + W Z (reduce<false>) and every P - x multiplicand met on the way."""
    x, y = M.domain_point(c["log"], M.bit_reverse_index(row, c["log"]))
    prx, pry, pix, piy = (c[k][b] for k in ("prx", "pry", "pix", "piy"))
    c0 = tuple((u - v) % P for u, v in zip(_cmul(prx, piy), _cmul(pry, pix)))
    npy = (P - piy[0], P - piy[1])                                         # multiplicands of x
    da, db = ((c0[k] + x * npy[k] + y * pix[k]) % P for k in range(2))
    nn = da * da + db * db
    ninv = pow(nn % P, P - 2, P)
    ndb = P - db
    ir, ii = da * ninv % P, ndb * ninv % P
    num, A, B = (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)
    for e in range(c["off"][b], c["off"][b + 1]):
        a_, b_, c_ = c["abc"][3 * e:3 * e + 3]
        f = int(c["cols"][c["cidx"][e]][row])
        num, A, B = qadd(num, tuple(w * f % P for w in c_)), qadd(A, a_), qadd(B, b_)
    nq = qsub(num, qadd(tuple(w * y % P for w in A), B))
    nii = P - ii
    terms = (nq[0] * ir + nq[1] * nii, nq[0] * ii + nq[1] * ir, nq[2] * ir + nq[3] * nii, nq[2] * ii + nq[3] * ir)
    return dict(da=da, db=db, nn=nn, ii=ii, terms=terms, operands=(npy[0], npy[1], ndb, nii))


@pytest.mark.parametrize("name,log,setting,family", S.quotient_case_ids())
def test_quotient_cases(name, log, setting, family):
    c = S.quotient_case(name, log, setting, family)
    n = 1 << log
    assert all(col.max() < P for col in c["cols"]) and all(v[2] == S.SAT4 for v in zip(*[iter(c["abc"])] * 3))
    out = S.quotient_expected(c)                            # accepted: a zero denominator raises OracleError
    assert family in S.CONSTANT_FAMILIES or two_values(out, n)
    if setting == "zero_b":
        # den.im = c0.b - x piy.b + y pix.b = 0 on every row: P - db = P, so ii = P * ninv = 0 and P - ii = P; P - piy.a = P in batch 0
        assert all(v[1] == 0 for k in ("prx", "pry", "pix", "piy") for v in c[k]) and c["piy"][0][0] == 0
    # denominators, norm sums and term sums of a few rows, every batch; a single batch's terms are the quotient itself
    rows4 = [0, 1, n // 2, n - 1]
    ops = set()
    for r in rows4:
        for b in range(len(c["lists"])):
            t = _batch_sums(c, b, r)
            assert t["nn"] < U63 and max(t["terms"]) < U63                 # the reduce<false> sites
            ops |= set(t["operands"])
            if setting == "zero_b":
                assert t["db"] == 0 and t["ii"] == 0
            if len(c["lists"]) == 1:
                assert tuple(v % P for v in t["terms"]) == tuple(int(out[k][r]) for k in range(4))
    if setting == "zero_b":
        assert ops == {P} | {P - v[0] for v in c["piy"]}                   # P - piy.b, P - db, P - ii are P; P - piy.a is P in batch 0
    if c["kernels"] == ["row"]:
        return                                             # the reference's formulation: no lazy sum
    rows = S.family_rows(family, c["mask"], n)
    sums = [s for r in rows[:4] for s in _numerator_sums(c, int(r))]
    assert max(sums) < U64
    e_max = max(len(b) for b in c["lists"])
    if family in ("S", "mixS"):
        if e_max >= 8:
            assert 0 < max(sums) - 4 * UNIT < 1 << 34          # four saturated products on top of a folded remainder
        elif e_max >= 4:
            assert max(sums) == 4 * UNIT
        if e_max >= 3:
            assert max(sums) >= U63                        # reduce<true>


def test_quotient_kernel_coverage():
    seen = {k for name, log, lists, al in S.QUOTIENT_SHAPES for k in S.quotient_kernels(log, lists, al)}
    want = {"row", "multi<2,false>", "multi<2,true>", "multi<3,false>", "multi<3,true>", "rp<3,false>", "rp<3,true>", "rp<4,false>",
            "rp<4,true>"} | {f"q8<{s},{z}>" for s in ("true", "false") for z in ("true", "false")}
    assert seen == want
    assert {len(b) for _, _, lists, _ in S.QUOTIENT_SHAPES for b in lists} >= {1, 3, 4, 5, 8, 9, 33}


def _plan_inputs():
    """(log, lists, out_aligned): every quotient shape of the suite, and logs 1..12 x aligned / unaligned x k = 1..12 batches over one
    list of 1, 4, 5 entries, three disjoint lists, and two lists of 10 union columns with 13 and 14 entries (1.3 and 1.4 per column)"""
    out = [(log, lists, al) for _, log, lists, al in S.QUOTIENT_SHAPES]
    shapes = [[list(range(e))] * k for k in range(1, 13) for e in (1, 4, 5)]
    shapes += [[[0], [1, 2, 3], [4, 5, 6, 7, 8]], [list(range(10)), [0, 1, 2]], [list(range(10)), [0, 1, 2, 3]]]
    return out + [(log, lists, al) for log in range(1, 13) for al in (True, False) for lists in shapes]


def test_quotient_plan_matches_the_library(tmp_path):
    """S.quotient_kernels is the tests' own statement of the launch plan; csrc/quotients_plan.h is the library's.  A stand-alone
    program that includes only that header prints the library's plan for every input of _plan_inputs: the two agree, the sweeps over
    a shared list are consecutive and cover every batch, and none of them holds a single batch."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "quotients_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "..", "tstwo_amd", "csrc"),
                           os.path.join(here, "quotients_plan_main.cpp"), "-o", exe])
    inputs = _plan_inputs()
    text = "".join(f"{log} {int(al)} {len({c for b in lists for c in b})} {' '.join(str(len(b)) for b in lists)}\n" for log, lists, al in inputs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(inputs)
    shared = 0
    for (log, lists, al), line in zip(inputs, got):
        launches = line.split()
        assert [l.split("@")[0] for l in launches] == S.quotient_kernels(log, lists, al), (log, lists, al, line)
        if "@" in line:
            shared += 1
            done = 0
            for l in launches:
                nb = int(l[l.index("<") + 1])
                assert nb >= 2 and int(l.split("@")[1]) == done, (log, lists, al, line)
                done += nb
            assert done == len(lists), (log, lists, al, line)
    assert shared > 100
    names = {l.split("@")[0] for line in got for l in line.split()}
    assert names == {"row", "multi<2,false>", "multi<2,true>", "multi<3,false>", "multi<3,true>", "rp<3,false>", "rp<3,true>", "rp<4,false>",
                     "rp<4,true>"} | {f"q8<{s},{z}>" for s in ("true", "false") for z in ("true", "false")}


def test_saturated_sample_constants_are_rejected_at_log_2():
    """why the sample constants are drawn per case: prx = pry = pix = piy = (P - 1, P - 1) has a zero denominator at log 2"""
    cols = [np.full(4, SAT, dtype=np.uint32)]
    sat2 = [(SAT, SAT)]
    with pytest.raises(orc.OracleError, match="0 has no inverse"):
        orc.accumulate_quotients_consts(M.half_initial(2), 2, cols, [0, 1], [0], [S.SAT4] * 3, [S.SAT4], sat2, sat2, sat2, sat2)


def test_saturated_line_coefficients_are_degenerate():
    """why a_j, b_j and the sample constants vary: with a = b = c = (P - 1,) * 4, saturated columns and saturated sample constants
    the numerator is s (1 + i)(1 + u) and the denominator (x - y)(1 + i), so coordinates 1 and 3 of the quotient vanish"""
    log = 5
    cols = [np.full(1 << log, SAT, dtype=np.uint32)]
    sat2 = [(SAT, SAT)]
    out = orc.accumulate_quotients_consts(M.half_initial(log), log, cols, [0, 1], [0], [S.SAT4] * 3, [S.SAT4], sat2, sat2, sat2, sat2)
    assert not out[1].any() and not out[3].any() and out[0].any() and out[2].any()


def _sample_abc(c):
    """(a, b, c) of every entry as the library derives them: a = conj(v) - v, c = conj(py) - py, b = v c - a py, times alpha^(j + 1)"""
    conj = lambda q: (q[0], q[1], (P - q[2]) % P, (P - q[3]) % P)
    abc = []
    for (px, py, cv), ecs in zip(c["batches"], S.sample_constants(c["batches"], c["coeff"])):
        cc = qsub(conj(py), py)
        alpha = (1, 0, 0, 0)
        for (_, v), ec in zip(cv, ecs):
            alpha = qmul(alpha, c["coeff"])
            a_ = qsub(conj(v), v)
            b_ = qsub(qmul(v, cc), qmul(a_, py))
            abc += [qmul(alpha, a_), qmul(alpha, b_), ec]
    return abc


@pytest.mark.parametrize("name,log,setting,family", S.sample_case_ids())
def test_sample_cases(name, log, setting, family):
    """c_j is derived by the library (alpha^(j + 1) (conj(py) - py)), not the caller's to saturate: the points of the saturated
    families are drawn so that a saturated row's numerator sum reaches S.sample_reach (bit 63 once a batch has three entries), and
    the largest sum the case gives is asserted here; for the other families it only has to stay below 2^64."""
    c = S.sample_case(name, log, setting, family)
    n = 1 << log
    out = S.sample_expected(c)                             # accepted: a zero denominator raises OracleError
    assert family in S.CONSTANT_FAMILIES or two_values(out, n)
    if setting == "zero_b":
        assert all(px[1] == px[3] == py[1] == py[3] == 0 and py[2] != 0 for px, py, _ in c["batches"])
    # the derived constants are the library's: the raw-constant oracle with them gives the same quotient
    off = np.cumsum([0] + [len(cv) for _, _, cv in c["batches"]]).tolist()
    bco = []
    for _, _, cv in c["batches"]:
        alpha = (1, 0, 0, 0)
        for _ in cv:
            alpha = qmul(alpha, c["coeff"])
        bco.append(alpha)
    raw = orc.accumulate_quotients_consts(M.half_initial(log), log, c["cols"], off, [ci for _, _, cv in c["batches"] for ci, _ in cv],
                                          _sample_abc(c), bco, [px[:2] for px, _, _ in c["batches"]], [py[:2] for _, py, _ in c["batches"]],
                                          [px[2:] for px, _, _ in c["batches"]], [py[2:] for _, py, _ in c["batches"]])
    assert all(np.array_equal(raw[k], out[k]) for k in range(4))
    if c["kernels"] == ["row"]:
        return                                             # the reference's formulation: no lazy sum
    rows = S.family_rows(family, c["mask"], n)
    sums = [v for r in rows[:4] for v in S.sample_numerator_sums(c, int(r))]
    assert max(sums) < U64
    if family in ("S", "mixS"):
        assert max(sums) >= S.sample_reach(c["lists"])


def test_sample_kernel_coverage():
    """the sample cases reach every quotient kernel, every batch size, log < 3 and an unaligned output"""
    cases = [S.sample_case(*i) for i in S.sample_case_ids()]
    seen = {k for c in cases for k in c["kernels"]}
    want = {"row", "multi<2,false>", "multi<2,true>", "multi<3,false>", "multi<3,true>", "rp<3,false>", "rp<3,true>", "rp<4,false>",
            "rp<4,true>"} | {f"q8<{s},{z}>" for s in ("true", "false") for z in ("true", "false")}
    assert seen == want
    assert {len(cv) for c in cases for _, _, cv in c["batches"]} >= {1, 3, 4, 5, 8, 9, 33}
    assert {c["log"] for c in cases} >= {1, 2} and any(not c["out_aligned"] for c in cases)
    assert {c["family"] for c in cases} >= {"S", "E", "mixS", "mixE"}


# ---------------------------------------------------------------- AIR
def _lazy_sums(values, coeff_word, every=4, fold_partial_group=True):
    """acc += coeff * value; folded after every `every`-th value (air.hip eval_rows also folds behind a last, partial group)"""
    acc, out = 0, []
    for k, v in enumerate(values):
        acc += coeff_word * int(v)
        out.append(acc)
        if k % every == every - 1:
            acc = fold_air(acc)
    return out, (fold_air(acc) if fold_partial_group and len(values) % every else acc)


def _is_lazy_max(worst, count):
    """the documented maximum: four saturated products on top of a folded remainder (0 < r < 2^33) once a second full group exists,
    else the products of the first group alone"""
    if count >= 8:
        return 0 < worst - 4 * UNIT < 1 << 33
    return worst == min(count, 4) * UNIT


@pytest.mark.parametrize("kind,n_constraints,log_expand,aligned,family", S.air_case_ids())
def test_air_cases(kind, n_constraints, log_expand, aligned, family):
    c = S.air_case(kind, n_constraints, log_expand, aligned, family)
    n = 1 << (c["trace_log"] + log_expand)
    mkind, out = M.MUL_ADD if kind == "mul_add" else M.WIDE_FIB, S.air_expected(c)
    assert family in S.CONSTANT_FAMILIES or two_values(out, n)
    cons = M.constraints_cols(mkind, c["cols"])
    assert len(cons) == n_constraints and len(c["dinv"]) == 1 << log_expand and max(c["dinv"]) < P and c["dinv"][0] == SAT
    row = int(np.flatnonzero(c["mask"])[0])
    assert all(int(col[row]) == SAT for col in cons)           # every constraint value P - 1 on the family's rows
    assert not all((col == SAT).all() for col in cons) or family == "S"
    assert all(int(c["accum"][j][row]) == SAT for j in range(4))
    sums, last = _lazy_sums([col[row] for col in cons], SAT)
    assert _is_lazy_max(max(sums), n_constraints) and max(sums) < U64 and last < 1 << 33
    if n_constraints >= 3:
        assert max(sums) >= U63
    assert int(out[0][row]) == (SAT + last % P * c["dinv"][row >> c["trace_log"]]) % P


@pytest.mark.parametrize("n_acc,way,log_expand,aligned", S.program_case_ids())
def test_program_cases(n_acc, way, log_expand, aligned):
    c = S.program_case(n_acc, way, log_expand, aligned)
    n = 1 << (c["trace_log"] + log_expand)
    out = S.program_expected(c)
    assert two_values(out, n)
    cons = X.run_program(c["words"], c["cols"], c["trace_log"], log_expand)
    assert len(cons) == c["n_acc"] <= 256 and len(c["words"]) // 2 <= 1536
    if way == "opcodes":
        a, b = c["cols"][1], c["cols"][2]
        assert ((a + b) == P).any() and ((a + b) == 2 * P - 2).any()        # ADD at exactly P and at 2P - 2
        seen = {int(v) for col in cons for v in col}
        assert {0, 1, P - 2, SAT} <= seen
        rows = range(n)
    else:
        rows = [r for r in range(n) if all(int(col[r]) == SAT for col in cons)]
        assert rows and (way not in ("load0", "load+1", "load-1") or len(rows) < n)
    worst = 0
    for r in list(rows)[:4]:
        sums, _ = _lazy_sums([col[r] for col in cons], SAT, fold_partial_group=False)
        worst = max(worst, max(sums))
    assert worst < U64
    if way != "opcodes":
        assert _is_lazy_max(worst, c["n_acc"])


# ---------------------------------------------------------------- LogUp
@pytest.mark.parametrize("n_terms,n_fracs,aligned,family", S.logup_case_ids())
def test_logup_cases(n_terms, n_fracs, aligned, family):
    c = S.logup_case(n_terms, n_fracs, aligned, family)
    n = 1 << c["log"]
    fr = S.logup_fractions(c)
    assert all(den[:, r].any() for _, den in fr for r in range(n))          # no zero denominator: the kernel raises no flag
    out = S.logup_expected(c)                                            # qinv raises on a zero
    assert family in S.CONSTANT_FAMILIES or two_values(out, n)
    row = int(np.flatnonzero(c["mask"])[0])
    assert all(int(c["prev"][j][row]) == SAT for j in range(4))
    if family in ("S", "mixS"):
        for f in c["fracs"]:
            assert all(int(col[row]) == SAT for col in f["cols"]) and all(co == S.SAT4 for co in f["coeffs"])
            sums, _ = _lazy_sums([col[row] for col in f["cols"]], SAT, fold_partial_group=False)
            assert _is_lazy_max(max(sums), n_terms) and max(sums) < U64
    else:
        for f in c["fracs"]:
            sums, _ = _lazy_sums([col[row] for col in f["cols"]], SAT, fold_partial_group=False)
            assert max(sums) < U64


@pytest.mark.parametrize("family", S.FINALIZE_FAMILIES)
@pytest.mark.parametrize("log", S.FINALIZE_LOGS)
def test_finalize_cases(log, family):
    col = S.finalize_case(log, family)
    n = 1 << log
    want, claimed = LM.finalize_last(col, log)
    assert n * SAT < U64                                                    # the raw-word sums of k_logup_small / _tile / _block_scan
    if family == "S":
        assert claimed == ((-n) % P,) * 4 and not want.any()                # s = -1: every shifted word is 0
    elif family == "zero":
        assert claimed == (0, 0, 0, 0) and not want.any()
    else:
        assert two_values(want, n) or log < 3
    assert all(int(want[j][LM.position(n - 1, log)]) == 0 for j in range(4))


# ---------------------------------------------------------------- eval_at_point
def _eval_tables(px, py, log):
    """W[4 r + j] of k_eval_coeffs: the products of fac over bits {0, 1} (j) and {10, 11} (r); fac = [y, x, pi(x), ...], zero beyond log"""
    fac, x = [(0, 0, 0, 0)] * max(12, log), px
    if log:
        fac[0] = py
    for i in range(1, log):
        fac[i] = x
        sx = qmul(x, x)
        x = tuple((2 * a - (1 if k == 0 else 0)) % P for k, a in enumerate(sx))
    w = []
    for e in range(16):
        v = (1, 0, 0, 0)
        for i, bit in enumerate((0, 1, 10, 11)):
            if (e >> i) & 1:
                v = qmul(v, fac[bit])
        w.append(v)
    return w


def _eval_worst(log, cfam, pkind):
    """The largest 64-bit sum any lane of k_eval_coeffs forms: a block of 4096 coefficients (beyond the polynomial: zeros) is 4 runs
    r of 256 lanes t of 4 words j, word (r, t, j) at 1024 r + 4 t + j; per coordinate the lane sums carry + sum_j v[j] W[4 r + j]
    run after run, the carry being the reduced sum of the run before.  Exact: every product is below 2^62 and the sum is rebuilt
    from 32-bit halves, so a sum that passed 2^64 would show."""
    coeffs = S.eval_coeffs(log, cfam).astype(np.uint64)
    w = _eval_tables(*S.eval_point(pkind, log), log)
    v = np.zeros(-(-len(coeffs) // 4096) * 4096, dtype=np.uint64)
    v[:len(coeffs)] = coeffs
    v = v.reshape(-1, 4, 256, 4)
    worst = 0
    for k in range(4):
        carry = np.zeros(v.shape[0:1] + (256,), dtype=np.uint64)
        for r in range(4):
            prods = [v[:, r, :, j] * np.uint64(w[4 * r + j][k]) for j in range(4)] + [carry]
            hi = sum(p >> np.uint64(32) for p in prods)
            lo = sum(p & np.uint64(0xffffffff) for p in prods)
            top = hi + (lo >> np.uint64(32))
            assert int(top.max()) < 1 << 32                                 # the sum stays below 2^64
            total = (top << np.uint64(32)) | (lo & np.uint64(0xffffffff))
            worst, carry = max(worst, int(total.max())), total % np.uint64(P)
    return worst


@pytest.mark.parametrize("log,cfam,pkind,aligned", S.eval_case_ids())
def test_eval_cases(log, cfam, pkind, aligned):
    """The factor table of k_eval_coeffs comes from the point, not from the caller, so 4 (P-1)^2 + carry cannot be forced.  What each
    case reaches is asserted from its inputs: with 2^11 coefficients or more (the table has its 16 entries, every lane four nonzero
    words per run) the largest sum of any lane has bit 63 set, i.e. more than two units; below that the table holds 1, y, x, x y
    only and the runs behind the first add nothing, so saturated coefficients give exactly (P - 1) (1 + y + x + x y) in the largest
    coordinate (log 1: two coefficients, (P - 1) (1 + y), below 2^63 whatever the point) and edge coefficients at least their
    largest single product.  log 0 is the constant polynomial: no kernel runs.  Nothing passes 2^64 (checked inside _eval_worst)."""
    coeffs = S.eval_coeffs(log, cfam)
    px, py = S.eval_point(pkind, log)
    if pkind == "circle":
        x2, y2 = qmul(px, px), qmul(py, py)
        assert tuple((a + b) % P for a, b in zip(x2, y2)) == (1, 0, 0, 0)
    got = orc.eval_at_point(coeffs, log, px, py)
    assert len(got) == 4 and max(got) < P
    if log == 0:
        return
    worst = _eval_worst(log, cfam, pkind)
    w = _eval_tables(px, py, log)
    if log >= 11:
        assert U63 <= worst < U64
    elif cfam == "S":
        assert worst == SAT * max(sum(w[j][k] for j in range(4)) for k in range(4))
    else:
        assert worst >= max(int(c) * w[i % 4][k] for i, c in enumerate(coeffs) for k in range(4))


def test_eval_cases_reach():
    """over all cases the largest sum is above three quarters of 2^64"""
    worst = max(_eval_worst(log, cfam, pkind) for log, cfam, pkind, _ in S.eval_case_ids() if log)
    assert 3 * U63 // 2 <= worst < U64

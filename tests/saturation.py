"""Operand families that push the lazy 64-bit accumulators of the kernels to their stated bounds, and the cases built from them.

Plain numpy: nothing here touches a GPU or imports the package under test.  tests/test_cpu_saturation.py proves on exact integers
that every case is accepted by its reference model, is not degenerate and reaches the bound it names; tests/test_gpu_saturation.py
runs the same cases through the C ABI and compares every output word.

Families (words are canonical M31 values, P = 2^31 - 1):
  S  every word P - 1
  Z  zeros where a kernel forms P - x or 2 (P - x) (the multiplicand becomes the non-canonical P / 2P), P - 1 elsewhere
  H  pairs (h_pair) that sum to exactly P or 2P - 2 (x, P - x; (P - 1) / 2, (P + 1) / 2; P - 1, P - 1): the switch point of
     min(s, s - P); only meaningful as a pair, so it is used where two columns meet in an add (the AIR programs)
  E  i.i.d. from EDGE
  mixF  family F on a seeded half of the rows (the SAME rows in every column of a case, so that whole rows are saturated), uniform
        words on the other rows: the rows of a 4-row or 8-row lane differ, and a row mix-up cannot hide behind constant columns
All inputs come from fixed seeds.

quotient_kernels(), inverse_kernel() and inverse_slot() restate in Python which launch the host side of the quotients
(csrc/quotients_plan.h) and of csrc/field_ops.hip picks for a shape, and which of a lane's elements an index is.  quotient_kernels()
is compared with the compiled header by tests/test_cpu_saturation.py; nothing ties the other two to the C++: whoever changes that
dispatch must update them here, or the coverage assertions of tests/test_cpu_saturation.py stay green while the GPU cases stop
reaching a kernel."""
from __future__ import annotations

import itertools

import numpy as np

P = 2147483647
SAT = P - 1
SAT4 = (SAT, SAT, SAT, SAT)
EDGE = (0, 1, 2, 1 << 15, (1 << 16) - 1, 1 << 16, 1 << 30, (1 << 30) + 1, P - 2, P - 1)
GRID = (0, 1, 2, 1 << 30, P - 2, P - 1)
FAMILIES = ("S", "Z", "E", "mixS", "mixZ", "mixE")
CONSTANT_FAMILIES = ("S",)               # whole constant columns: run once per site, exempt from the two-values requirement


# ---------------------------------------------------------------- families
def uniform(rng, n, nonzero=False):
    return rng.integers(1 if nonzero else 0, P, size=n, dtype=np.uint64)


def fam_s(rng, n):
    return np.full(n, SAT, dtype=np.uint64)


def fam_z(rng, n):
    """zeros and P - 1, at random"""
    return np.where(rng.integers(0, 2, size=n) == 0, 0, SAT).astype(np.uint64)


def fam_e(rng, n):
    return np.asarray(EDGE, dtype=np.uint64)[rng.integers(0, len(EDGE), size=n)]


def h_pair(rng, n):
    """(a, b) with a + b in {P, 2P - 2} on every row, and a - b = 0 on the P - 1 rows"""
    x = uniform(rng, n, nonzero=True)
    kind = rng.integers(0, 4, size=n)
    a = np.select([kind == 0, kind == 1, kind == 2], [x, np.full(n, (P - 1) // 2), np.full(n, (P + 1) // 2)], SAT).astype(np.uint64)
    b = np.where(kind == 3, SAT, P - a).astype(np.uint64)
    return a, b


_FAM = {"S": fam_s, "Z": fam_z, "E": fam_e, "U": uniform}


def half_mask(rng, n):
    """exactly half of the rows (at least one), seeded"""
    m = np.zeros(n, dtype=bool)
    m[rng.permutation(n)[:max(n // 2, 1)]] = True
    return m


def column(family, rng, n, mask=None):
    """One column of `family`; the mixes use `mask` (rows of the family) so that every column of a case saturates the same rows."""
    if family.startswith("mix"):
        assert mask is not None
        return np.where(mask, _FAM[family[3:]](rng, n), uniform(rng, n)).astype(np.uint64)
    return _FAM[family](rng, n).astype(np.uint64)


def family_rows(family, mask, n):
    """rows on which every column of the case carries the family (all rows for the whole-column families)"""
    return np.flatnonzero(mask) if family.startswith("mix") else np.arange(n)


def felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def felt_from(family, rng):
    return tuple(int(v) for v in column(family, rng, 4))


# ---------------------------------------------------------------- batch inverses
def grid_values(dim):
    """GRID^dim minus zero: (6^dim - 1, dim)"""
    return np.array([v for v in itertools.product(GRID, repeat=dim) if any(v)], dtype=np.uint64)


INVERSE_SLOTS = {"qm31_norm": 8, "qm31_v4": 4, "qm31_strided": 8, "cm31_strided": 8, "m31_strided": 4}


def inverse_kernel(dim, n, aligned):
    """the launch tstwo_{m31,cm31,qm31}_batch_inverse takes (csrc/field_ops.hip)"""
    if dim == 1:
        assert n < 1 << 24
        return "m31_strided"
    if dim == 2:
        return "cm31_strided"
    if aligned and n % 8 == 0 and n >= 8:
        return "qm31_norm"
    if aligned and n % 4 == 0 and n >= 4:
        return "qm31_v4"
    return "qm31_strided"


def inverse_slot(kernel, i, n):
    """which of a lane's elements element i is"""
    i = np.asarray(i)
    if kernel == "qm31_norm":              # lane t: elements 4 (t + g T) + k, T = n / 8 -> slot 4 g + k
        return 4 * (i // (4 * (n // 8))) + i % 4
    if kernel == "qm31_v4":
        return i % 4
    k = INVERSE_SLOTS[kernel]              # lane t: elements t + j T, T = ceil(n / K) -> slot j
    return i // ((n + k - 1) // k)


# (coordinates, length, aligned); unaligned = every pointer one word into its buffer
INVERSE_CASES = [(4, 10432, True), (4, 10436, True), (4, 10435, True), (4, 10432, False),
                 (2, 320, True), (2, 323, True), (2, 320, False),
                 (1, 64, True), (1, 67, True), (1, 64, False)]


def cm31_sqrt(z):
    """a square root of z = (a, b) in CM31 = F_P[i] (P = 3 mod 4), or None"""
    a, b = z
    sq = lambda v: pow(v, (P + 1) // 4, P)
    for s in {sq((a * a + b * b) % P), (P - sq((a * a + b * b) % P)) % P}:
        t = (a + s) * pow(2, P - 2, P) % P
        x = sq(t)
        if x and x * x % P == t:
            y = b * pow(2 * x, P - 2, P) % P
            if ((x * x - y * y) % P, 2 * x * y % P) == (a, b):
                return x, y
    return None


def norm_saturating_qm31():
    """x = (c0, 0) with D = c0^2 = (dr, di), both within 4 of P: its norm sum dr^2 + di^2 is within 2^35 of 2^63 (the largest a
    reduce<false> site of k_qm31_batch_inverse_norm can see)"""
    for dr in range(SAT, SAT - 4, -1):
        for di in range(SAT, SAT - 4, -1):
            r = cm31_sqrt((dr, di))
            if r:
                return (r[0], r[1], 0, 0)
    raise AssertionError("no square near (P - 1, P - 1)")


def qm31_norm_inverse_words(a, b, c, d):
    """(ir, ii) of k_qm31_batch_inverse_norm: D^-1 for D = c0^2 - (2 + i) c1^2"""
    cm = lambda x, y: ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)
    s0, s1 = cm((a, b), (a, b)), cm((c, d), (c, d))
    dr, di = (s0[0] - (2 * s1[0] - s1[1])) % P, (s0[1] - (s1[0] + 2 * s1[1])) % P
    ninv = pow((dr * dr + di * di) % P, P - 2, P)
    return dr * ninv % P, (P - di) * ninv % P


_OUTPUT_SATURATING = []


def output_saturating_qm31(tries=4000):
    """(P - 1, P - 1, c, d) whose inverse words make oa = a ir + b (P - ii) largest over a seeded search: the output sums of
    k_qm31_batch_inverse_norm depend on the inverse, which the caller cannot choose, so two full units (2^63 - 2^34) are out of reach"""
    if not _OUTPUT_SATURATING:
        rng = np.random.default_rng(4242)
        best, arg = -1, None
        for _ in range(tries):
            c, d = int(rng.integers(0, P)), int(rng.integers(0, P))
            ir, ii = qm31_norm_inverse_words(SAT, SAT, c, d)
            v = SAT * ir + SAT * (P - ii)
            if v > best:
                best, arg = v, (SAT, SAT, c, d)
        _OUTPUT_SATURATING.append(arg)
    return _OUTPUT_SATURATING[0]


def inverse_values(dim):
    vals = grid_values(dim)
    if dim == 4:
        vals = np.concatenate([vals, np.array([norm_saturating_qm31(), output_saturating_qm31()], dtype=np.uint64)])
    return vals


def inverse_input(dim, n, aligned, seed=1):
    """(dim, n) words: every value of the grid (and, for QM31, the norm-saturating element) in every lane slot of the launch,
    uniform nonzero values elsewhere"""
    rng = np.random.default_rng(seed)
    vals = inverse_values(dim)
    out = rng.integers(1, P, size=(dim, n), dtype=np.uint64)
    kernel = inverse_kernel(dim, n, aligned)
    slots = inverse_slot(kernel, np.arange(n), n)
    for s in range(INVERSE_SLOTS[kernel]):
        idx = np.flatnonzero(slots == s)
        assert len(idx) >= len(vals), (kernel, n, s)
        where = idx[rng.permutation(len(idx))[:len(vals)]]
        out[:, where] = np.roll(vals, 37 * s, axis=0).T
    return out


# ---------------------------------------------------------------- quotients
def _shared(k, e):
    return [list(range(e))] * k


QUOTIENT_SHAPES = []                      # (name, log, column list of every batch, output aligned)
for _log in (5, 9):
    for _e in (1, 3, 4, 5, 8, 9, 33):     # k_quotients8<SINGLE = true, LAZY = e > 4>
        QUOTIENT_SHAPES.append((f"single{_e}", _log, [list(range(_e))], True))
    # several batches over different lists: k_quotients8<false, LAZY>
    QUOTIENT_SHAPES.append(("lists_1_3_4", _log, [[0], [1, 2, 3], [4, 5, 6, 7]], True))
    QUOTIENT_SHAPES.append(("lists_5_8_9", _log, [list(range(5)), list(range(5, 13)), list(range(13, 22))], True))
    QUOTIENT_SHAPES.append(("lists_33_4_1", _log, [list(range(33)), [33, 34, 35, 36], [37]], True))
    # k batches over one list: log < 9 k_quotients8_multi<2 | 3, ACC>; log >= 9 k_quotients_rp<3 | 4, ACC> (and multi<2> for a rest of 2)
    for _k, _e in zip(range(2, 9), (5, 9, 8, 4, 33, 3, 1)):
        QUOTIENT_SHAPES.append((f"shared{_k}x{_e}", _log, _shared(_k, _e), True))
# k_quotients_row: log < 3, and an unaligned output
QUOTIENT_SHAPES += [("row_log1", 1, [[0, 1, 2], [3, 4, 5, 6, 7]], True), ("row_log2", 2, [[0, 1, 2], [3, 4, 5, 6, 7]], True),
                    ("row_unaligned", 5, [[0, 1, 2, 3, 4], [1, 2]], False)]
QUOTIENT_SETTINGS = ("random", "zero_b")
# every shape with the two row mixes; the other families on one shape per kernel
QUOTIENT_FAMILIES_ALL = ("mixS", "mixE")
QUOTIENT_FAMILIES_MORE = ("S", "Z", "E", "mixZ")
QUOTIENT_SHAPES_MORE = ("single4", "single9", "lists_1_3_4", "lists_5_8_9", "shared2x5", "shared3x9", "shared7x3", "shared8x1", "row_log2",
                        "row_unaligned")


def quotient_case_ids():
    out = []
    for name, log, _, _ in QUOTIENT_SHAPES:
        fams = QUOTIENT_FAMILIES_ALL + (QUOTIENT_FAMILIES_MORE if name in QUOTIENT_SHAPES_MORE else ())
        out += [(name, log, s, f) for s in QUOTIENT_SETTINGS for f in fams]
    return out


def _shape(name, log):
    return next(s for s in QUOTIENT_SHAPES if s[0] == name and s[1] == log)


def quotient_kernels(log, lists, out_aligned):
    """the launches tstwo_quotients_accumulate takes, as names: the tests' own statement of quotients_plan() in csrc/quotients_plan.h
    (test_cpu_saturation.py::test_quotient_plan_matches_the_library compiles that header and compares the two)"""
    if log < 3 or not out_aligned:
        return ["row"]
    n_entries = sum(len(b) for b in lists)
    per = len({c for b in lists for c in b})
    if len(lists) >= 2 and 10 * n_entries >= 14 * per:
        out, done = [], 0
        while done < len(lists):
            left = len(lists) - done
            if log >= 9 and left >= 3:
                nb = 3 if left in (3, 5, 6) else 4
                out.append(f"rp<{nb},{'true' if done else 'false'}>")
            else:
                nb = 2 if left in (2, 4) else 3
                out.append(f"multi<{nb},{'true' if done else 'false'}>")
            done += nb
        return out
    lazy = any(len(b) > 4 for b in lists)
    return [f"q8<{'true' if len(lists) == 1 else 'false'},{'true' if lazy else 'false'}>"]


def quotient_case(name, log, setting, family):
    """Raw-constant quotients (tstwo_quotients_accumulate): c_j, the batch coefficients and the column words saturated; a_j, b_j and
    the sample constants vary.  setting "zero_b": every prx.b, pry.b, pix.b, piy.b is 0 (the imaginary part of every denominator is 0:
    P - db = P, ii = 0, P - ii = P) and piy = 0 in batch 0 (P - piy.a = P)."""
    _, _, lists, out_aligned = _shape(name, log)
    rng = np.random.default_rng(sum(ord(c) for c in name + setting + family) * 131 + log)
    n = 1 << log
    n_cols = max(c for b in lists for c in b) + 1
    mask = half_mask(rng, n)
    cols = [column(family, rng, n, mask).astype(np.uint32) for _ in range(n_cols)]
    off, cidx, abc = [0], [], []
    for b in lists:
        for c in b:
            cidx.append(c)
            abc += [felt(rng), felt(rng), SAT4]
        off.append(len(cidx))
    nb = len(lists)
    cm = lambda zero_b: (int(rng.integers(1, P)), 0 if zero_b else int(rng.integers(0, P)))
    zb = setting == "zero_b"
    prx, pry, pix, piy = ([cm(zb) for _ in range(nb)] for _ in range(4))
    if zb:
        piy[0] = (0, 0)
    return dict(name=name, log=log, setting=setting, family=family, lists=lists, out_aligned=out_aligned, cols=cols, mask=mask, off=off,
                cidx=cidx, abc=abc, coeff=[SAT4] * nb, prx=prx, pry=pry, pix=pix, piy=piy, kernels=quotient_kernels(log, lists, out_aligned))


SAMPLE_FAMILIES_MORE = ("S", "E")


def sample_case_ids():
    """the matrix of quotient_case_ids through the samples: every shape with the two row mixes, whole columns on one shape per kernel"""
    out = []
    for name, log, _, _ in QUOTIENT_SHAPES:
        fams = QUOTIENT_FAMILIES_ALL + (SAMPLE_FAMILIES_MORE if name in QUOTIENT_SHAPES_MORE else ())
        out += [(name, log, s, f) for s in QUOTIENT_SETTINGS for f in fams]
    return out


def sample_constants(batches, coeff):
    """What tstwo_quotients_accumulate_samples derives (csrc/quotients.hip quotients_from_samples, Rust conjugation): per entry the
    numerator coefficient alpha^(j + 1) c with c = conj(py) - py, j the entry's index in its batch; [[QM31 per entry] per batch]"""
    from gkr_model import qmul, qsub
    out = []
    for _, py, cv in batches:
        c = qsub((py[0], py[1], (P - py[2]) % P, (P - py[3]) % P), py)
        alpha, row = (1, 0, 0, 0), []
        for _ in cv:
            alpha = qmul(alpha, coeff)
            row.append(qmul(alpha, c))
        out.append(row)
    return out


def sample_numerator_sums(c, row):
    """the 64-bit numerator sums of `row`, every coordinate, group by group, as the kernels of c["kernels"] form them from the
    derived coefficients (LAZY: folded as 2 hi + lo between groups of 4; else one group on top of the reduced value)"""
    if c["kernels"] == ["row"]:
        return []
    lazy = not c["kernels"][0].startswith("q8") or c["kernels"][0].endswith("true>")
    out = []
    for (_, _, cv), ec in zip(c["batches"], sample_constants(c["batches"], c["coeff"])):
        for k in range(4):
            acc = 0
            for j in range(0, len(cv), 4):
                group = sum(ec[e][k] * int(c["cols"][cv[e][0]][row]) for e in range(j, min(j + 4, len(cv))))
                acc = (2 * (acc >> 32) + (acc & 0xffffffff) if lazy else acc % P) + group
                out.append(acc)
    return out


def sample_reach(lists):
    """what a saturated row must reach: bit 63 once a batch has three entries, else half of its products' worth"""
    e_max = max(len(b) for b in lists)
    return 1 << 63 if e_max >= 3 else e_max * SAT * SAT // 2


def sample_case(name, log, setting, family):
    """The same through the samples (tstwo_quotients_accumulate_samples): the library derives a, b, c, so c_j cannot be saturated by
    the caller.  Points: random QM31 words, or "zero_b": coordinates 1 and 3 of x and y zero (prx.b = pry.b = pix.b = piy.b = 0;
    piy.a must stay nonzero: a point equal to its conjugate is refused).  Sampled values from E, the random coefficient saturated.
    For the families with saturated rows the points are redrawn (seeded) until the derived coefficients carry the numerator sum of a
    saturated row to sample_reach(); tests/test_cpu_saturation.py asserts the sum the case gives."""
    _, _, lists, out_aligned = _shape(name, log)
    n = 1 << log
    n_cols = max(c for b in lists for c in b) + 1
    for attempt in range(256):
        rng = np.random.default_rng(sum(ord(c) for c in name + setting + family) * 137 + log + 100003 * attempt)
        mask = half_mask(rng, n)
        cols = [column(family, rng, n, mask).astype(np.uint32) for _ in range(n_cols)]
        batches = []
        for b in lists:
            px, py = felt(rng), felt(rng)
            if setting == "zero_b":
                px, py = (px[0], 0, px[2], 0), (py[0], 0, int(rng.integers(1, P)), 0)
            batches.append((px, py, [(c, felt_from("E", rng)) for c in b]))
        case = dict(name=name, log=log, setting=setting, family=family, lists=lists, out_aligned=out_aligned, cols=cols, mask=mask,
                    batches=batches, coeff=SAT4, kernels=quotient_kernels(log, lists, out_aligned))
        if family not in ("S", "mixS") or case["kernels"] == ["row"]:
            return case
        if max(sample_numerator_sums(case, int(family_rows(family, mask, n)[0]))) >= sample_reach(lists):
            return case
    raise AssertionError(("no sample point reaches the bound", name, log, setting, family))


# ---------------------------------------------------------------- AIR, hand-written constraints
AIR_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 126, 127, 128)
AIR_TRACE_LOG = 3


def air_case_ids():
    """(kind, n_constraints, log_expand, aligned, family)"""
    out = [("wide_fib", k, le, al, "mixS") for k in AIR_COUNTS for le in (1, 4) for al in (True, False)]
    out += [("wide_fib", k, 1, True, "S") for k in (4, 5, 8, 128)]
    out += [("mul_add", 1, le, al, f) for le in (1, 4) for al in (True, False) for f in ("mixS", "S")]
    return out


def _sat_denoms(rng, log_expand, family):
    """2^log_expand inverse denominators: all P - 1 for the constant family, else P - 1 first and E / uniform words after it"""
    d = [SAT] * (1 << log_expand)
    if family != "S":
        for i in range(1, len(d)):
            d[i] = int(fam_e(rng, 1)[0]) if i % 2 else int(rng.integers(1, P))
    return d


def air_case(kind, n_constraints, log_expand, aligned, family):
    """Columns whose constraints are all P - 1 on the family's rows (wide Fibonacci with x_{i+2} = x_i^2 + x_{i+1}^2 - 1, mul-add with
    x_2 = x_0 x_1 + x_0 + 1; the entry point does not require a satisfied trace), uniform words on the other rows; coefficient words
    P - 1; the incoming accumulator P - 1 on the family's rows."""
    rng = np.random.default_rng(1000 * n_constraints + 10 * log_expand + aligned + (7 if family == "S" else 0) + (500000 if kind == "mul_add" else 0))
    n = 1 << (AIR_TRACE_LOG + log_expand)
    mask = half_mask(rng, n) if family != "S" else np.ones(n, dtype=bool)
    x0, x1 = column("mixE", rng, n, mask), column("mixS", rng, n, mask)
    if kind == "mul_add":
        cols = [x0, x1, np.where(mask, (x0 * x1 % P + x0 + 1) % P, uniform(rng, n)).astype(np.uint64)]
    else:
        cols = [x0, x1]
        for _ in range(n_constraints):
            a, b = cols[-2], cols[-1]
            cols.append(np.where(mask, (a * a % P + b * b % P + P - 1) % P, uniform(rng, n)).astype(np.uint64))
    accum = np.stack([np.where(mask, SAT, uniform(rng, n)).astype(np.uint64) for _ in range(4)])
    return dict(kind=kind, cols=cols, mask=mask, trace_log=AIR_TRACE_LOG, log_expand=log_expand, aligned=aligned, family=family,
                coeffs=[SAT4] * n_constraints, dinv=_sat_denoms(rng, log_expand, family), accum=accum)


# ---------------------------------------------------------------- AIR programs
LOAD, CONST, ADD, SUB, MUL, SQR, NEG, ACC = range(8)          # include/tstwo_hip.h TSTWO_AIR_OP_*
PROGRAM_COUNTS = AIR_COUNTS + (255, 256)
PROGRAM_WAYS = ("const", "load0", "load+1", "load-1", "sub", "mul")


def enc(op, dst=0, x=0, w1=0):
    return [op | (dst << 8) | (x << 16), w1 & 0xffffffff]


def program_case_ids():
    """(n_acc, way, log_expand, aligned): every count with every way; log_expand and the alignment rotate"""
    out = [(k, w, 1 + (i + j) % 2, (i + j) % 3 != 0) for i, k in enumerate(PROGRAM_COUNTS) for j, w in enumerate(PROGRAM_WAYS)]
    out += [(0, "opcodes", le, al) for le in (1, 2) for al in (True, False)]
    return out


def program_case(n_acc, way, log_expand, aligned):
    """A program that accumulates one register n_acc times; the register holds P - 1 (everywhere, or for the loads on the rows whose
    source row is in the mask), produced by `way`.  Way
    "opcodes": ADD to exactly P, SUB of equals, NEG 0 and SQR (P - 1), each pushed through every opcode before its ACC."""
    rng = np.random.default_rng(77 * n_acc + 5 * log_expand + aligned + sum(ord(c) for c in way))
    trace_log = 3
    n = 1 << (trace_log + log_expand)
    mask = half_mask(rng, n)
    a, b = h_pair(rng, n)                                     # a + b = P or 2P - 2 on every row
    sat = column("mixS", rng, n, mask)
    cols = [sat, a, b, column("mixE", rng, n, mask)]
    w = []
    if way == "opcodes":
        w += enc(LOAD, 0, 0, 0) + enc(LOAD, 1, 1, 0) + enc(LOAD, 2, 2, 0) + enc(CONST, 3, 0, SAT) + enc(CONST, 4, 0, 0)
        w += enc(ADD, 5, 1, 2)                                # exactly P (-> 0) or 2P - 2 (-> P - 2)
        w += enc(SUB, 6, 1, 1)                                # equals: 0
        w += enc(NEG, 7, 4)                                   # NEG 0
        w += enc(SQR, 8, 3)                                   # SQR (P - 1) = 1
        n_acc = 0
        for v in (5, 6, 7, 8):
            for op, args in ((ADD, (v, v)), (ADD, (v, 3)), (SUB, (v, 3)), (SUB, (4, v)), (MUL, (v, 3)), (MUL, (v, 0)), (SQR, (v,)), (NEG, (v,))):
                w += enc(op, 9, args[0], args[1] if len(args) > 1 else 0) + enc(ACC, 0, 9) + enc(ACC, 0, v)
                n_acc += 2
    else:
        if way == "const":
            w += enc(CONST, 0, 0, SAT)
        elif way.startswith("load"):
            w += enc(LOAD, 0, 0, int(way[4:]))
        elif way == "sub":
            w += enc(CONST, 1, 0, 0) + enc(CONST, 2, 0, 1) + enc(SUB, 0, 1, 2)
        else:
            w += enc(CONST, 1, 0, SAT) + enc(CONST, 2, 0, 1) + enc(MUL, 0, 1, 2)
        for _ in range(n_acc):
            w += enc(ACC, 0, 0)
    accum = np.stack([np.where(mask, SAT, uniform(rng, n)).astype(np.uint64) for _ in range(4)])
    return dict(words=w, cols=cols, mask=mask, trace_log=trace_log, log_expand=log_expand, aligned=aligned, n_acc=n_acc, way=way,
                coeffs=[SAT4] * n_acc, dinv=_sat_denoms(rng, log_expand, "mixS"), accum=accum)


# ---------------------------------------------------------------- LogUp
LOGUP_TERMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16)
LOGUP_FRACS = (1, 2, 8)
LOGUP_LOG = 3


def logup_case_ids():
    """(n_terms, n_fracs, aligned, family)"""
    out = [(t, f, al, "mixS") for t in LOGUP_TERMS for f in LOGUP_FRACS for al in (True, False)]
    out += [(t, 2, True, fam) for t in (4, 5, 8, 16) for fam in ("S", "mixE", "mixZ")]
    return out


def logup_case(n_terms, n_fracs, aligned, family):
    """Coefficient and column words saturated (the family's rows), a random constant per fraction, the numerator a constant (even
    n_terms + fraction index) or a column, prev P - 1 on the family's rows."""
    rng = np.random.default_rng(100 * n_terms + 10 * n_fracs + aligned + sum(ord(c) for c in family))
    n = 1 << LOGUP_LOG
    mask = half_mask(rng, n) if family.startswith("mix") else np.ones(n, dtype=bool)
    fracs = []
    for b in range(n_fracs):
        cols = [column(family, rng, n, mask) for _ in range(n_terms)]
        num = int(fam_e(rng, 1)[0]) if (n_terms + b) % 2 == 0 else column("mixE" if family.startswith("mix") else "E", rng, n, mask)
        fracs.append(dict(cols=cols, coeffs=[SAT4] * n_terms, constant=felt(rng), num=num))
    prev = np.stack([np.where(mask, SAT, uniform(rng, n)).astype(np.uint64) for _ in range(4)])
    return dict(fracs=fracs, prev=prev, mask=mask, log=LOGUP_LOG, aligned=aligned, family=family)


def logup_denominator(frac, n):
    """(4, n): sum_t coeff_t cols_t + constant"""
    den = np.zeros((4, n), dtype=np.uint64)
    for j in range(4):
        den[j] = frac["constant"][j]
        for c, co in zip(frac["cols"], frac["coeffs"]):
            den[j] = (den[j] + co[j] * c % P) % P
    return den


FINALIZE_LOGS = (1, 2, 5, 11, 12, 13, 14, 18)
FINALIZE_FAMILIES = ("S", "zero", "E", "mixS")


def finalize_case(log, family):
    rng = np.random.default_rng(9000 + log)
    n = 1 << log
    if family == "zero":
        return np.zeros((4, n), dtype=np.uint64)
    mask = half_mask(rng, n)
    return np.stack([column(family, rng, n, mask) for _ in range(4)])


# ---------------------------------------------------------------- eval_at_point
EVAL_LOGS = (0, 1, 5, 11, 12, 13, 14, 16, 20)


def eval_case_ids():
    """(log, coefficient family, point kind, aligned)"""
    out = [(lg, cf, pk, True) for lg in EVAL_LOGS for cf in ("S", "E") for pk in ("S", "E", "circle")]
    out += [(lg, "S", "S", False) for lg in (5, 13)]
    return out


def eval_coeffs(log, family):
    rng = np.random.default_rng(31 * log + ord(family[0]))
    return column(family, rng, 1 << log).astype(np.uint32)


def eval_point(kind, log):
    """(x, y) as QM31 words: saturated, edge words, or ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)), a point on the QM31 circle"""
    rng = np.random.default_rng(17 * log + ord(kind[0]))
    if kind == "S":
        return SAT4, SAT4
    if kind == "E":
        return felt_from("E", rng), felt_from("E", rng)
    from gkr_model import qadd, qinv, qmul, qsub          # exact integer QM31 arithmetic (test infrastructure)
    t, one = felt(rng), (1, 0, 0, 0)
    t2 = qmul(t, t)
    inv = qinv(qadd(t2, one))
    return qmul(qsub(one, t2), inv), qmul(qadd(t, t), inv)


# ---------------------------------------------------------------- the reference side (exact integers / the CPU oracle; imported lazily)
def quotient_expected(c):
    import air_model as M
    from oracle import oracle as orc
    return orc.accumulate_quotients_consts(M.half_initial(c["log"]), c["log"], c["cols"], c["off"], c["cidx"], c["abc"], c["coeff"],
                                           c["prx"], c["pry"], c["pix"], c["piy"])


def sample_expected(c):
    import air_model as M
    from oracle import oracle as orc
    return orc.accumulate_quotients(M.half_initial(c["log"]), c["log"], c["cols"], c["coeff"], c["batches"])


def air_expected(c):
    import air_model as M
    kind = M.MUL_ADD if c["kind"] == "mul_add" else M.WIDE_FIB
    return M.quotients_on_domain(kind, c["cols"], c["trace_log"], c["log_expand"], c["coeffs"], c["dinv"], c["accum"])


def program_expected(c):
    import air_program_model as X
    return X.eval_program_on_domain(c["words"], c["cols"], c["trace_log"], c["log_expand"], c["coeffs"], c["dinv"], c["accum"])


def logup_fractions(c):
    """[(numerator column, (4, n) denominator)] as tests/logup_model.py takes them"""
    n = 1 << c["log"]
    return [(np.full(n, f["num"], dtype=np.uint64) if isinstance(f["num"], int) else f["num"], logup_denominator(f, n)) for f in c["fracs"]]


def logup_expected(c):
    import logup_model as LM
    return LM.column(logup_fractions(c), c["prev"], 1 << c["log"])

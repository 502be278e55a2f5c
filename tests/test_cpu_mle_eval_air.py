"""The mle_eval component on the host (no GPU): the construction of DESIGN §4.5 on Python integers (tests/mle_eval_air_model.py)
with the project's own offset map, the eval of tstwo_amd/mle_eval.py against that model (its compiled program through the
interpreter's integer model, PointEvaluator at a random point), the refusals, and the ISA of the two new kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import P

import air_check_model as CM
import air_program_model as X
import gkr_model as G
import logup_model as LM
import mle_eval_air_model as M
from tstwo_amd import constraint_framework as F
from tstwo_amd import mle_eval as ME
from tstwo_amd.fields import QM31

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LOGS = [2, 3, 4, 5, 6, 7]


def q(t):
    return QM31.from_u32_unchecked(*[int(v) for v in t])


def case(n, seed=0, n_terms=3):
    """An honest statement of log size n: (point, cols, coeffs, constant, E, S, claim)."""
    rng = np.random.default_rng(1000 * seed + n)
    point = M.random_point(rng, n)
    cols = [G.random_base(rng, 1 << n) for _ in range(n_terms)]
    coeffs = [G.random_felt(rng) for _ in range(n_terms)]
    constant = G.random_felt(rng)
    e, s, claim = M.interaction_trace(point, cols, coeffs, constant)
    return point, cols, coeffs, constant, e, s, claim


# ------------------------------------------------------------------ the geometry the construction assumes
@pytest.mark.parametrize("n", LOGS)
def test_offset_two_moves_the_circle_domain_index_by_one_inside_each_half(n):
    h = 1 << (n - 1)
    d = np.array([LM.rev(p, n) for p in range(1 << n)])
    for off, sign in ((2, 1), (-2, -1)):
        nb = X.neighbour_map(n, n, off)
        want = np.where(d < h, (d + sign) % h, (d - h - sign) % h + h)
        assert np.array_equal(d[nb], want)
    # the package's own map (which needs a larger evaluation domain) agrees with the geometry there, for every offset used
    for off in (-2, -1, 2):
        nb = X.neighbour_map(n, n + 1, off)
        assert all(F.offset_bit_reversed_circle_domain_index(p, n, n + 1, off) == nb[p] for p in range(2 << n))


@pytest.mark.parametrize("n", LOGS)
def test_the_eq_variable_j_is_bit_j_of_the_circle_domain_index(n):
    point = M.random_point(np.random.default_rng(n), n)
    e = M.eq_table(point)
    for p in range(1 << n):
        d = LM.rev(p, n)
        want = G.ONE
        for j in range(n):
            want = G.qmul(want, point[j] if (d >> j) & 1 else G.qsub(G.ONE, point[j]))
        assert G.at(e, p) == want


# ------------------------------------------------------------------ selectors
@pytest.mark.parametrize("n", LOGS)
def test_exactly_one_selector_of_g_and_k_per_row(n):
    sel = M.selectors(n)
    assert len(sel) == 2 * n + 2 and all(set(np.unique(c)) <= {0, 1} for c in sel)
    assert np.array_equal(np.sum(sel[:2 * n], axis=0), np.ones(1 << n, dtype=np.uint64))
    assert sel[2 * n].sum() == 1 and sel[2 * n + 1].sum() == 1
    assert sum(int(c.sum()) for c in sel[:n]) == 1 << (n - 1)                  # G covers the first half, K the second
    assert np.array_equal(M.selectors_vec(n), np.stack(sel).astype(np.uint32))


# ------------------------------------------------------------------ the honest trace
@pytest.mark.parametrize("n", LOGS)
def test_every_constraint_vanishes_on_the_honest_trace(n):
    point, cols, coeffs, constant, e, s, claim = case(n)
    assert claim == G.eval_mle_at(M.form_values(cols, coeffs, constant, 1 << n), point)
    for c in M.constraints(n, point, claim, cols, coeffs, constant, e, s):
        assert not c.any()
    assert G.at(s, LM.position((1 << n) - 1, n)) == G.ZERO                    # the last coset row of S holds 0


@pytest.mark.parametrize("n", LOGS)
def test_walking_the_step_and_anchor_constraints_rebuilds_the_eq_table(n):
    point = M.random_point(np.random.default_rng(50 + n), n)
    assert np.array_equal(M.walk(n, point), G.gen_eq_evals(point, G.ONE))


def test_host_constants_match_the_model():
    for n in LOGS:
        point = M.random_point(np.random.default_rng(70 + n), n)
        a, b, c0, c1 = ME.mle_eval_constants([q(r) for r in point])
        ma, mb, m0, m1 = M.constants(point)
        assert [x.tup() for x in a] == ma and [x.tup() for x in b] == mb and c0.tup() == m0 and c1.tup() == m1


# ------------------------------------------------------------------ single changes are caught
def _bump(t):
    return tuple((v + 1) % P for v in t)


@pytest.mark.parametrize("n", LOGS)
def test_each_single_change_breaks_a_constraint(n):
    point, cols, coeffs, constant, e, s, claim = case(n, seed=1)
    rng = np.random.default_rng(n)

    def broken(point=point, claim=claim, cols=cols, e=e, s=s):
        return [len(M.failing_rows(c)) for c in M.constraints(n, point, claim, cols, coeffs, constant, e, s)]

    assert broken() == [0, 0, 0]
    p = int(rng.integers(0, 1 << n))
    e2 = e.copy()
    e2[0, p] = (e2[0, p] + 1) % P
    assert sum(broken(e=e2)) > 0 and (broken(e=e2)[0] > 0 or broken(e=e2)[1] > 0)          # one cell of E
    s2 = s.copy()
    s2[2, p] = (s2[2, p] + 1) % P
    assert broken(s=s2)[2] > 0                                                              # one cell of S
    c2 = [c.copy() for c in cols]
    c2[1][p] = (c2[1][p] + 1) % P
    assert broken(cols=c2)[2] > 0                                                           # one cell of a form column
    assert broken(claim=_bump(claim))[2] == 1 << n                                          # v
    for j in range(n):                                                                      # one coordinate of r
        r2 = list(point)
        r2[j] = _bump(r2[j])
        assert sum(broken(point=r2)[:2]) > 0


# ------------------------------------------------------------------ the eval of the package against the model
def _eval(n, point, claim, coeffs, constant):
    form = ME.MleEvalForm([(q(w), ("main", i)) for i, w in enumerate(coeffs)], q(constant))
    return ME.MleEvalEval(n, [q(r) for r in point], q(claim), form)


@pytest.mark.parametrize("n", [2, 3, 5, 7])
def test_the_compiled_program_computes_the_model_constraints(n):
    point, cols, coeffs, constant, e, s, claim = case(n, seed=2)
    ev = _eval(n, point, claim, coeffs, constant)
    comp = F.FrameworkComponent(ev, None, list(range(2 * n + 2)))
    assert comp.n_constraints == 3 and comp.secure_flags == [True] * 3 and comp.info.max_degree() == 2
    assert comp.claimed_sum is None and comp.n_columns == 3 and comp.n_interaction_columns == 8
    assert comp.interaction_offsets == [[-2, 0, 2]] * 4 + [[-1, 0]] * 4
    assert ev.max_constraint_log_degree_bound() == n + 1
    sel = M.selectors(n)
    columns = list(cols) + sel + list(e) + list(s)
    accs = X.run_program(comp.program.words, [np.asarray(c, dtype=np.uint64) for c in columns], n, 0)
    want = M.constraints(n, point, claim, cols, coeffs, constant, e, s, sel)
    assert len(accs) == 12
    for k, c in enumerate(want):
        assert np.array_equal(np.stack(accs[4 * k:4 * k + 4]), c)
    # a changed cell of E and of S: the report names constraint 0 / 2 and the first failing coset row
    groups = CM.grouping([4, 4, 4])
    assert [r[0] for r in CM.report(comp.program.words, columns, n, groups)] == [0, 0, 0]
    rows = CM.coset_rows(n)
    p = 1
    e2 = e.copy()
    e2[3, p] = (e2[3, p] + 5) % P
    rep = CM.report(comp.program.words, list(cols) + sel + list(e2) + list(s), n, groups)
    bad = M.constraints(n, point, claim, cols, coeffs, constant, e2, s, sel)
    for k in range(3):
        fr = M.failing_rows(bad[k])
        assert rep[k] == ((len(fr), int(rows[fr].min())) if len(fr) else (0, CM.NO_ROW))
    assert rep[0][0] > 0 and rep[2][0] == 1


@pytest.mark.parametrize("n", [2, 4, 7])
def test_point_evaluator_agrees_with_the_model_at_a_random_point(n):
    rng = np.random.default_rng(90 + n)
    point = M.random_point(rng, n)
    claim, constant = G.random_felt(rng), G.random_felt(rng)
    coeffs = [G.random_felt(rng) for _ in range(2)]
    ev = _eval(n, point, claim, coeffs, constant)
    sel = [G.random_felt(rng) for _ in range(2 * n + 2)]
    cols = [G.random_felt(rng) for _ in range(2)]
    e3, s2 = [G.random_felt(rng) for _ in range(3)], [G.random_felt(rng) for _ in range(2)]

    def partial(values):
        """4 base-column samples per offset whose from_partial_evals is the wanted QM31: (value, 0, 0, 0)."""
        return [[q(v) for v in values]] + [[QM31.zero() for _ in values] for _ in range(3)]

    inter = partial(e3) + partial(s2)
    got = F.point_constraints(ev, [[q(c)] for c in cols], [q(v) for v in sel], inter)
    want = M.constraints_at(n, point, claim, coeffs, constant, sel, cols, e3[0], e3[1], e3[2], s2[0], s2[1])
    assert [g.tup() for g in got] == want


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [0, 1])
def test_a_point_coordinate_zero_or_one_is_refused(bad):
    rng = np.random.default_rng(5)
    form = ME.MleEvalForm([(QM31.one(), ("main", 0))])
    for n in (2, 5):
        for j in range(n):
            point = [q(r) for r in M.random_point(rng, n)]
            point[j] = q((bad, 0, 0, 0))
            with pytest.raises(ValueError, match=f"coordinate {j}"):
                ME.MleEvalEval(n, point, QM31.zero(), form)
    with pytest.raises(ValueError, match="log_size must be 2 to 28"):
        ME.MleEvalEval(1, [q((5, 0, 0, 0))], QM31.zero(), form)
    with pytest.raises(ValueError, match="3 coordinates"):
        ME.MleEvalEval(4, [q((5, 0, 0, 0))] * 3, QM31.zero(), form)


def test_batched_form_adds_the_claims_with_powers_of_gamma():
    rng = np.random.default_rng(8)
    g, z = q(G.random_felt(rng)), q(G.random_felt(rng))
    f1 = ME.MleEvalForm([(QM31.one(), ("main", 0))], z.neg())
    f2 = ME.MleEvalForm([(QM31.one().neg(), ("main", 1))])
    f3 = ME.MleEvalForm([(QM31.one(), ("pre", 0)), (QM31.one(), ("main", 0))], z.neg())
    v = [q(G.random_felt(rng)) for _ in range(3)]
    form, claim = ME.batched_form(v, [f1, f2, f3], g)
    assert claim.tup() == v[0].add(g.mul(v[1])).add(g.mul(g).mul(v[2])).tup()
    assert form.constant.tup() == z.neg().add(g.mul(g).mul(z.neg())).tup()
    assert dict((ref, w.tup()) for w, ref in form.terms) == {
        ("main", 0): QM31.one().add(g.mul(g)).tup(), ("main", 1): g.neg().tup(), ("pre", 0): g.mul(g).tup()}
    assert form.n_main == 2 and form.n_pre() == 1


# ------------------------------------------------------------------ the kernels' ISA
def test_both_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from tstwo_amd import build as B
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("binutils / ROCm LLVM tools not available")
    os.makedirs(B.OBJ, exist_ok=True)
    obj = B._compile("mle_eval_air.hip", False)          # the in-tree object; compiled here only when it is missing or stale
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    kernels, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif name and line.strip():
            kernels[name].append(line.split("//")[0].strip())
    for stem in ("k_mle_eval_selectors", "k_mle_eval_terms"):
        found = [k for k in kernels if stem in k and not k.endswith(".kd")]
        assert len(found) == 2, (stem, list(kernels))                       # W = 4 and W = 1
        for k in found:
            ins = [i for i in kernels[k] if i]
            assert ins and not [i for i in ins if i.startswith("scratch_")], f"{k} uses scratch memory"
            assert [i for i in ins if i.startswith("global_store")] and not [i for i in ins if i.startswith("flat_")]
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    sizes = re.findall(r"\.name:\s+(\S*k_mle_eval\S*).*?\.private_segment_fixed_size:\s+(\d+)", notes, flags=re.S)
    assert len(sizes) == 4 and all(int(sz) == 0 for _, sz in sizes), sizes

"""AIR host side without a GPU: the integer model's vanishing denominators and power ordering, and the DEEP-ALI identity that ties
the model's composition polynomial (domain accumulation + oracle interpolation) to the verifier's point evaluation in
tstwo_amd/air.py.  This pins the conventions (coefficient order, denominators, bit reversal) the device prover must follow."""
import numpy as np
import pytest

import air_model as M
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd.circle import CanonicCoset, CirclePoint
from tstwo_amd.fields import M31, QM31

P = M.P


def q(t):
    return QM31.from_u32_unchecked(*t)


def qpoint(p):
    return CirclePoint(q(p[0]), q(p[1]))


def rand_felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


@pytest.mark.parametrize("log", [1, 2, 3, 5, 8])
def test_denom_inv_vanishes_on_trace_coset_only(log):
    coset = M.canonic_coset(log)
    init, step = coset[0], 1 << (31 - log)
    for i in range(1 << log):
        assert M.coset_vanishing(coset, M.index_to_point(init + i * step)) == 0
    # the evaluation domain of log + 1 (and + 2) is disjoint from the trace coset: no zero denominator
    for el in (log + 1, log + 2):
        for j in range(1 << el):
            assert M.coset_vanishing(coset, M.domain_point(el, j)) != 0
        dinv = M.denom_inv(log, el)
        assert [d.value for d in A.denominator_inverses(log, el)] == dinv
        # only 2^(el - log) distinct values: the vanishing polynomial is constant on each trace-sized block (bit-reversed order)
        e = el - log
        for j in range(1 << el):
            v = M.coset_vanishing(coset, M.domain_point(el, j))
            assert v * dinv[M.bit_reverse_index(j, el) >> log] % P == 1


def test_host_coset_vanishing_matches_model_at_secure_points():
    rng = np.random.default_rng(1)
    for log in (1, 4, 9, 20):
        for _ in range(3):
            pt = M.random_point(rand_felt(rng))
            want = M.coset_vanishing(M.canonic_coset(log), pt, secure=True)
            assert A.coset_vanishing(CanonicCoset(log).coset, qpoint(pt)).tup() == want
        p = M.domain_point(log + 1, 3)
        assert A.coset_vanishing(CanonicCoset(log).coset, CirclePoint(M31(p[0]), M31(p[1]))).value == \
            M.coset_vanishing(M.canonic_coset(log), p)


def test_point_accumulation_is_horner_with_descending_powers():
    rng = np.random.default_rng(2)
    alpha = rand_felt(rng)
    evals = [rand_felt(rng) for _ in range(11)]
    explicit = (0, 0, 0, 0)
    for i, e in enumerate(evals):
        explicit = M.qadd(explicit, M.qmul(M.qpow(alpha, len(evals) - 1 - i), e))
    assert M.point_horner(alpha, evals) == explicit
    acc = A.PointEvaluationAccumulator(q(alpha))
    for e in evals:
        acc.accumulate(q(e))
    assert acc.finalize().tup() == explicit
    # the split of the powers over several components
    cf = M.component_coeffs(alpha, [3, 5, 1])
    flat = [c for comp in cf for c in comp]
    assert flat == [M.qpow(alpha, 8 - g) for g in range(9)]


def _components_from(specs, rng, broken=None):
    """specs: [(kind, log, n_cols)] -> (model components, tstwo_amd components); broken = (component, column, row)."""
    model, host = [], []
    alloc = A.TraceLocationAllocator()
    for k, (kind, log, n_cols) in enumerate(specs):
        n = 1 << log
        if kind == M.WIDE_FIB:
            cols = M.wide_fib_trace(rng.integers(0, P, size=n), rng.integers(0, P, size=n), n_cols)
            host.append(F.WideFibonacciComponent(log, n_cols, alloc))
        else:
            cols = M.mul_add_trace(rng.integers(0, P, size=n), rng.integers(0, P, size=n))
            host.append(F.MulAddComponent(log, alloc))
        if broken is not None and broken[0] == k:
            cols[broken[1]] = cols[broken[1]].copy()
            cols[broken[1]][broken[2]] = (cols[broken[1]][broken[2]] + 1) % P
        model.append((kind, log, cols))
    return model, host


def _deep_ali(specs, seed, broken=None):
    rng = np.random.default_rng(seed)
    model, host = _components_from(specs, rng, broken)
    alpha = rand_felt(rng)
    log, comp = M.composition_polynomial(model, alpha)
    assert log == max(l for _, l, _ in specs) + 1
    pt = M.random_point(rand_felt(rng))
    lhs = M.from_partial_evals([M.eval_at(comp[j], log, pt) for j in range(4)])
    # the verifier's side in tstwo_amd: mask values = the trace polynomials at the point, preprocessed tree empty
    mask = [[], []]
    for _, l, cols in model:
        mask[1] += [[q(M.eval_at(M.interpolate(c, l), l, pt))] for c in cols]
    comps = A.Components(host)
    rhs = comps.eval_composition_polynomial_at_point(qpoint(pt), mask, q(alpha)).tup()
    assert rhs == M.eval_composition_at_point(model, alpha, pt)
    return lhs, rhs


@pytest.mark.parametrize("log", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("kind,n_cols", [(M.WIDE_FIB, 8), (M.MUL_ADD, 3)])
def test_deep_ali_identity_single_component(log, kind, n_cols):
    lhs, rhs = _deep_ali([(kind, log, n_cols)], seed=100 + log)
    assert lhs == rhs
    lhs, rhs = _deep_ali([(kind, log, n_cols)], seed=100 + log, broken=(0, n_cols - 1, (1 << log) // 3))
    assert lhs != rhs


def test_deep_ali_identity_wide_fib_100_columns():
    lhs, rhs = _deep_ali([(M.WIDE_FIB, 5, 100)], seed=7)
    assert lhs == rhs


@pytest.mark.parametrize("broken", [None, (1, 4, 5), (2, 2, 0)])
def test_deep_ali_identity_multi_component(broken):
    specs = [(M.WIDE_FIB, 7, 12), (M.WIDE_FIB, 5, 6), (M.MUL_ADD, 3, 3), (M.WIDE_FIB, 5, 4)]
    lhs, rhs = _deep_ali(specs, seed=9, broken=broken)
    assert (lhs == rhs) == (broken is None)


def test_components_mask_points_and_log_sizes_concatenate_in_allocation_order():
    alloc = A.TraceLocationAllocator()
    cs = [F.WideFibonacciComponent(6, 5, alloc), F.MulAddComponent(3, alloc), F.WideFibonacciComponent(4, 3, alloc)]
    assert [c.trace_locations[1] for c in cs] == [(0, 5), (5, 8), (8, 11)]
    comps = A.Components(cs)
    assert comps.column_log_sizes() == [[], [6] * 5 + [3] * 3 + [4] * 3]
    assert comps.composition_log_degree_bound() == 7
    pt = qpoint(M.random_point((5, 6, 7, 8)))
    mp = comps.mask_points(pt)
    assert mp[0] == [] and len(mp[1]) == 11 and all(len(c) == 1 and c[0] == pt for c in mp[1])


def test_example05_table_satisfies_the_mul_add_constraint():
    cols = M.example05_trace()
    assert [int(v) for v in cols[2][:2]] == [6, 84]
    assert not M.constraints_cols(M.MUL_ADD, cols)[0].any()

"""-m gpu: the lookups that need keyed and weighted multiplicities, end to end.  An XOR table with the tuple key (a, b) looked up
by a padded component (XorTableEval / XorValuesEval: the multiplicity column comes from tstwo_lookup_multiplicities_keyed, the
interaction traces from derive_interaction_trace, proof and verification from the unchanged prove / verify), and the gated range
check through LogUp-GKR (gkr_range_check_*(..., enablers=))."""
import numpy as np
import pytest

import lookup_keyed_model as KM
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import gkr_lookup as GL
from tstwo_amd import logup as LG
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles
from tstwo_amd.prover import InvalidLogupSum, prove, verify

pytestmark = pytest.mark.gpu

LOG_BITS, LOG_ROWS = 3, 7
PADDING = 0x7FFFFFFE              # what a disabled row holds: a field element far outside the table


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, c if isinstance(c, HipColumn) else HipColumn(np.asarray(c, dtype=np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def _trace(padding):
    """(a, b, c, enabler) of 2^LOG_ROWS rows, about half of them enabled; the others hold `padding` (None: values of the table)."""
    rng = np.random.default_rng(12)
    n = 1 << LOG_ROWS
    a, b = (rng.integers(0, 1 << LOG_BITS, size=n, dtype=np.uint32) for _ in range(2))
    enabler = rng.integers(0, 2, size=n, dtype=np.uint32)
    assert n // 4 < enabler.sum() < 3 * n // 4
    c = a ^ b
    if padding is not None:
        a, b, c = (np.where(enabler, x, padding).astype(np.uint32) for x in (a, b, c))
    return a, b, c, enabler


def _xor_proof(padding, gated):
    """The XOR table and values components by the caller protocol of test_gpu_lookup.py::_range_check_proof, everything on the
    device.  gated: the multiplicities are the enabler-weighted sums; else every row counts once (the old entry's semantics,
    through the keyed entry without a weight column).  Returns (components, proof, config, claimed sums, multiplicity column)."""
    log_table = 2 * LOG_BITS
    config = PcsConfig(5, FriConfig(0, 1, 3))
    a, b, c, enabler = (HipColumn(x) for x in _trace(padding))
    if gated:
        mult = F.xor_multiplicities_device(LOG_BITS, a, b, enabler)
    else:
        mult = LG.lookup_multiplicities_keyed([LG.LookupGroup([(a, LOG_BITS), (b, LOG_BITS)])], order="coset")
    table = [HipColumn(t) for t in F.xor_table_columns(LOG_BITS)]
    tw = precompute_twiddles(CanonicCoset(max(log_table + 1, LOG_ROWS + 2, 10) + 1).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    _commit(scheme, _evals(table, log_table), ch)
    _commit(scheme, _evals([mult], log_table) + _evals([a, b, c, enabler], LOG_ROWS), ch)
    le = LG.LookupElements.draw(ch, 3)
    t_inter, t_sum = LG.derive_interaction_trace(F.XorTableEval(LOG_BITS, le), [mult], table)
    v_inter, v_sum = LG.derive_interaction_trace(F.XorValuesEval(LOG_ROWS, le), [a, b, c, enabler])
    ch.mix_felts([t_sum, v_sum])
    _commit(scheme, t_inter + v_inter, ch)
    alloc = A.TraceLocationAllocator()
    comps = [F.FrameworkComponent(F.XorTableEval(LOG_BITS, le), alloc, [0, 1, 2], claimed_sum=t_sum),
             F.FrameworkComponent(F.XorValuesEval(LOG_ROWS, le), alloc, claimed_sum=v_sum)]
    return comps, prove(comps, ch, scheme), config, (t_sum, v_sum), mult


def _verify(comps, proof, config, sums):
    ch = Blake2sChannel()
    v = CommitmentSchemeVerifier(config)
    sizes = A.Components(comps, 3).column_log_sizes()
    v.commit(proof.commitments[0], [2 * LOG_BITS] * 3, ch)
    v.commit(proof.commitments[1], sizes[1], ch)
    LG.LookupElements.draw(ch, 3)
    ch.mix_felts(list(sums))
    v.commit(proof.commitments[2], sizes[2], ch)
    verify(comps, ch, v, proof)


def test_xor_table_columns():
    a, b, c = F.xor_table_columns(LOG_BITS)
    pos = F._coset_positions(2 * LOG_BITS)
    k = np.arange(1 << (2 * LOG_BITS))
    assert np.array_equal(a[pos] + (b[pos] << LOG_BITS), k) and np.array_equal(c, a ^ b) and a.max() == b.max() == (1 << LOG_BITS) - 1


def test_xor_proof_with_gated_multiplicities():
    comps, proof, config, (t_sum, v_sum), mult = _xor_proof(PADDING, gated=True)
    assert t_sum.add(v_sum) == QM31.zero()
    a, b, c, enabler = _trace(PADDING)
    assert (a[enabler == 0] == PADDING).all() and (c[enabler == 0] == PADDING).all()
    want, rejected = KM.multiplicities(2 * LOG_BITS, [([(a, LOG_BITS), (b, LOG_BITS)], enabler)], "coset")
    assert rejected == 0 and np.array_equal(mult.to_numpy(), want) and int(want.sum()) == int(enabler.sum())
    _verify(comps, proof, config, (t_sum, v_sum))


def test_ungated_counts_fail_the_logup_sum():
    """The disabled rows hold values of the table, and the counts are taken without the weight column: the table then answers
    rows the values component never asks for, and the two claimed sums no longer cancel."""
    comps, proof, config, sums, mult = _xor_proof(None, gated=False)
    assert int(mult.to_numpy().sum()) == 1 << LOG_ROWS
    assert sums[0].add(sums[1]) != QM31.zero()
    with pytest.raises(InvalidLogupSum):
        _verify(comps, proof, config, sums)
    # and with the padding out of range the ungated count refuses the trace altogether
    a, b, _, _ = _trace(PADDING)
    with pytest.raises(ValueError, match="a checked value lies outside the range"):
        LG.lookup_multiplicities_keyed([LG.LookupGroup([(a, LOG_BITS), (b, LOG_BITS)])])


def test_gated_gkr_range_check():
    log_range, n = 6, 1 << 7
    rng = np.random.default_rng(13)
    values = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for _ in range(2)]
    enablers = [(np.arange(n) % 2 == k).astype(np.uint32) for k in range(2)]            # half the rows of each column
    values = [np.where(e, v, PADDING).astype(np.uint32) for v, e in zip(values, enablers)]
    cols, ens = [HipColumn(v) for v in values], [HipColumn(e) for e in enablers]
    proof = GL.gkr_range_check_prove(Blake2sChannel(), log_range, cols, enablers=ens)
    GL.gkr_range_check_verify(Blake2sChannel(), log_range, proof, cols, enablers=ens)
    for c, v in zip(cols + ens, values + enablers):                  # the caller's columns are left as they were
        assert np.array_equal(c.to_numpy(), v)
    want, rejected = KM.multiplicities(log_range, [([(v, log_range)], e) for v, e in zip(values, enablers)], "natural")
    got = LG.lookup_multiplicities_keyed([LG.LookupGroup([(c, log_range)], weight=e) for c, e in zip(cols, ens)], order="natural")
    assert rejected == 0 and np.array_equal(got.to_numpy(), want) and int(want.sum()) == n
    # without enablers the same columns are outside the range
    with pytest.raises(ValueError, match="a checked value lies outside the range"):
        GL.gkr_range_check_prove(Blake2sChannel(), log_range, cols)

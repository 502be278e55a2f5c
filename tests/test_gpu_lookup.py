"""-m gpu: tstwo_lookup_multiplicities and tstwo_coset_iota (tstwo_amd/csrc/lookup.hip) bit for bit against the host functions
they replace (constraint_framework.range_check_multiplicities / range_check_table_column, np.bincount) on the shapes of
tests/lookup_plan.py — which kernel paths each shape reaches is accounted for without a GPU in test_cpu_lookup_plan.py — then
contention, the grid-stride wrap of each branch, rejection, repeatability, guard bands, the argument checks, and a range-check
proof whose multiplicity and table columns never leave the device."""
import ctypes as C

import numpy as np
import pytest

import arena as AR
import lookup_plan as LP
from tstwo_amd import _lib as L
from tstwo_amd import air as A
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.circle import CanonicCoset
from tstwo_amd.fields import QM31
from tstwo_amd.fri_prover import FriConfig
from tstwo_amd.pcs import CommitmentSchemeProver, PcsConfig
from tstwo_amd.pcs_verifier import CommitmentSchemeVerifier
from tstwo_amd.poly import HipCircleEvaluation, precompute_twiddles
from tstwo_amd.prover import prove, verify

pytestmark = pytest.mark.gpu

P = L.P
BAD_ARG = 7                      # include/tstwo_hip.h TSTWO_ERR_BAD_ARG
SENTINEL = 0xA5A5A5A5
BRANCH_LOGS = {"LDS": LP.LAST_LDS_LOG, "GLOBAL": LP.FIRST_GLOBAL_LOG}


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def sizes(lens):
    return (C.c_size_t * max(len(lens), 1))(*lens)


def place_columns(arrays, offsets):
    """Each array in a device buffer of its own, `offset` words past the buffer's (16-byte aligned) start; (buffers, addresses)."""
    bufs = [HipColumn(np.concatenate([np.zeros(off, dtype=np.uint32), np.asarray(a, dtype=np.uint32)])) for a, off in zip(arrays, offsets)]
    assert all(b.ptr % 16 == 0 for b in bufs)
    return bufs, [b.ptr + 4 * off for b, off in zip(bufs, offsets)]


def count(log_range, addrs, lens, order, out=None, with_rejected=True):
    """One call of the entry into `out` (a fresh sentinel-filled column by default): (counts, n_rejected or None)."""
    if out is None:
        out = HipColumn(np.full(1 << log_range, 0x25A5A5A5, dtype=np.uint32))
    rej = HipColumn(np.array([12345], dtype=np.uint32)) if with_rejected else None
    L.call("tstwo_lookup_multiplicities", L.ptr_array(addrs), sizes(lens), len(addrs), log_range, LP.ORDERS[order], out.ptr,
           rej.ptr if rej else None)
    return out.to_numpy(), (int(rej.to_numpy()[0]) if rej else None)


def check_both_orders(log_range, arrays, offsets, want_rejected=0):
    bufs, addrs = place_columns(arrays, offsets)
    lens = [len(a) for a in arrays]
    for order in ("coset", "natural"):
        want, rejected = LP.multiplicities(log_range, arrays, order)
        assert rejected == want_rejected
        got, n_rej = count(log_range, addrs, lens, order)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{order}: {bad.size} wrong words, the first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"
        assert n_rej == want_rejected
    return want


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", [n for n in LP.gpu_shapes() if not n.startswith("wrap")])
def test_parity_with_the_host_functions(name):
    log_range, cols = LP.gpu_shapes()[name]
    rng = np.random.default_rng(9000 + 31 * log_range + len(cols))
    arrays = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for n, _ in cols]
    natural = check_both_orders(log_range, arrays, [off for _, off in cols])
    # the model the helper compares with is itself the host functions' (test_cpu_lookup_plan.py up to 2^10); here at this size
    assert np.array_equal(natural, np.bincount(np.concatenate(arrays), minlength=1 << log_range))
    bufs, addrs = place_columns(arrays, [off for _, off in cols])
    got, _ = count(log_range, addrs, [n for n, _ in cols], "coset")
    assert np.array_equal(got, F.range_check_multiplicities(log_range, *arrays))


# ------------------------------------------------------------------ contention
@pytest.mark.parametrize("branch", ["LDS", "GLOBAL"])
@pytest.mark.parametrize("which", ["first", "last"])
def test_every_value_in_one_bin(branch, which):
    log_range = BRANCH_LOGS[branch]
    k = 0 if which == "first" else (1 << log_range) - 1
    natural = check_both_orders(log_range, [np.full(1 << 16, k, dtype=np.uint32)], [0])
    assert natural[k] == 1 << 16 and natural.sum() == 1 << 16


@pytest.mark.parametrize("branch", ["LDS", "GLOBAL"])
def test_every_bin_exactly_once(branch):
    log_range = BRANCH_LOGS[branch]
    natural = check_both_orders(log_range, [np.random.default_rng(5).permutation(1 << log_range).astype(np.uint32)], [0])
    assert (natural == 1).all()


# ------------------------------------------------------------------ grid stride
@pytest.mark.parametrize("branch", ["LDS", "GLOBAL"])
def test_grid_stride_past_the_wrap_point(branch):
    """One column of wrap + 1029 words: the grid is at its cap and its first 258 lanes take a second unit, the last of them a
    partial one (test_cpu_lookup_plan.py: "wrap")."""
    log_range, cols = LP.WRAP_CASES[branch]
    assert "wrap" in LP.reaches(log_range, [0], [cols[0][0]])
    rng = np.random.default_rng(77 + log_range)
    check_both_orders(log_range, [rng.integers(0, 1 << log_range, size=cols[0][0], dtype=np.uint32)], [0])


# ------------------------------------------------------------------ rejection
class SyncCounter:
    """Counts the library calls that wait for the device (every read-back is one of them)."""
    SYNC_CALLS = {"tstwo_download", "tstwo_download_many", "tstwo_sync", "tstwo_check_zero_flag", "tstwo_gather_words", "tstwo_upload_wait"}

    def __init__(self, monkeypatch):
        self.n, self.names = 0, []
        orig_call = L.call

        def call(name, *a):
            self.names.append(name)
            if name in self.SYNC_CALLS:
                self.n += 1
            return orig_call(name, *a)
        monkeypatch.setattr(L, "call", call)


@pytest.mark.parametrize("branch", ["LDS", "GLOBAL"])
@pytest.mark.parametrize("n_bad", [0, 1, 1000])
def test_words_outside_the_range_are_left_out_and_counted(branch, n_bad, monkeypatch):
    log_range = BRANCH_LOGS[branch]
    rng = np.random.default_rng(600 + n_bad + log_range)
    arrays = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for n in (4099, 257, 2048)]
    inside, _ = LP.multiplicities(log_range, arrays, "natural")
    outside = np.concatenate([[1 << log_range, P - 1], rng.integers(1 << log_range, P, size=1000)]).astype(np.uint32)[:n_bad]
    if n_bad == 1:
        outside[0] = P - 1
    if n_bad == 1000:
        assert 1 << log_range in outside and P - 1 in outside
    # the words outside go in between the others (inserted, so the words inside keep their counts), into all three columns
    parts = np.array_split(outside, 3)
    arrays = [np.insert(a, np.sort(rng.integers(0, a.size, size=p.size)), p) for a, p in zip(arrays, parts)]
    natural = check_both_orders(log_range, arrays, [0, 1, 0], want_rejected=n_bad)
    assert np.array_equal(natural, inside)
    # the Python entry: check=True reads the one word back and raises, check=False reads nothing back and skips them
    cols = [HipColumn(a) for a in arrays]
    if n_bad:
        with pytest.raises(ValueError, match="a checked value lies outside the range"):
            LG.lookup_multiplicities(log_range, *cols, order="natural")
        with pytest.raises(ValueError, match="a checked value lies outside the range"):
            F.range_check_multiplicities_device(log_range, *cols)
    else:
        assert np.array_equal(LG.lookup_multiplicities(log_range, *cols, order="natural").to_numpy(), inside)
    L.sync()
    counter = SyncCounter(monkeypatch)
    out = LG.lookup_multiplicities(log_range, *cols, order="natural", check=False)
    assert counter.n == 0 and "tstwo_lookup_multiplicities" in counter.names
    monkeypatch.undo()
    assert np.array_equal(out.to_numpy(), inside)


# ------------------------------------------------------------------ repeatability and scratch
def test_same_call_twice_and_sizes_in_turn():
    """The entry zeroes `out` itself (a second call into the same column gives the same words), and neither the LDS histogram
    nor the uploaded column table carries anything from one call to the next, whatever the order of the sizes."""
    rng = np.random.default_rng(31)
    for logs in ((16, 3, 16), (3, 14, 2, 15, 14)):
        for log_range in logs:
            arrays = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for n in (5000, 3)]
            bufs, addrs = place_columns(arrays, [0, 0])
            want, _ = LP.multiplicities(log_range, arrays, "coset")
            out = HipColumn.uninitialized(1 << log_range)
            first, _ = count(log_range, addrs, [5000, 3], "coset", out=out)
            second, _ = count(log_range, addrs, [5000, 3], "coset", out=out)
            assert np.array_equal(first, want) and np.array_equal(second, want), log_range


# ------------------------------------------------------------------ coset_iota
@pytest.mark.parametrize("log_size", list(range(1, 13)) + [16])
def test_coset_iota_is_the_range_check_table_column(log_size):
    want = F.range_check_table_column(log_size)
    assert np.array_equal(LG.coset_iota(log_size).to_numpy(), want)
    assert np.array_equal(F.range_check_table_column_device(log_size).to_numpy(), want)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("branch", ["LDS", "GLOBAL"])
@pytest.mark.parametrize("order", ["coset", "natural"])
@pytest.mark.parametrize("with_rejected", [True, False])
def test_nothing_outside_the_outputs_is_written(branch, order, with_rejected):
    log_range = BRANCH_LOGS[branch]
    rng = np.random.default_rng(88 + log_range)
    lens, offsets = (4099, 257, 0, 1), (0, 4, 8, 12)
    arrays = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for n in lens]
    arrays[0][7], arrays[1][256] = 1 << log_range, P - 1                  # two words outside the range
    regions = [AR.rin(f"col{c}", a, offset=off) for c, (a, off) in enumerate(zip(arrays, offsets))]
    regions += [AR.rout("out", 1 << log_range), AR.rout("n_rejected", 1, offset=4)]
    with AR.Arena(regions) as ar:
        L.call("tstwo_lookup_multiplicities", ar.ptrs([f"col{c}" for c in range(4)]), sizes(lens), 4, log_range, LP.ORDERS[order],
               ar.ptr("out"), ar.ptr("n_rejected") if with_rejected else None)
        res = ar.check()
    want, rejected = LP.multiplicities(log_range, arrays, order)
    assert rejected == 2 and np.array_equal(res["out"], want)
    assert res["n_rejected"][0] == (2 if with_rejected else SENTINEL)


@pytest.mark.parametrize("log_size", [1, 5, 13])
def test_coset_iota_writes_its_column_only(log_size):
    with AR.Arena([AR.rout("out", 1 << log_size, offset=4)]) as ar:
        L.call("tstwo_coset_iota", ar.ptr("out"), log_size)
        res = ar.check()
    assert np.array_equal(res["out"], F.range_check_table_column(log_size))


# ------------------------------------------------------------------ arguments
def test_every_limit_is_refused_before_anything_is_launched():
    col = HipColumn(np.arange(64, dtype=np.uint32))
    out = HipColumn(np.full(256, 0x25A5A5A5, dtype=np.uint32))
    rej = HipColumn(np.array([99], dtype=np.uint32))
    one, n64 = L.ptr_array([col.ptr]), sizes([64])
    many = L.ptr_array([col.ptr] * 65)
    cases = {
        "log_range 0": (one, n64, 1, 0, 1, out.ptr, rej.ptr), "log_range 29": (one, n64, 1, 29, 1, out.ptr, rej.ptr),
        "no column": (one, n64, 0, 8, 1, out.ptr, rej.ptr), "65 columns": (many, sizes([1] * 65), 65, 8, 1, out.ptr, rej.ptr),
        "too many values": (one, sizes([2 ** 31 - 1]), 1, 8, 1, out.ptr, rej.ptr),
        "too many values in all": (L.ptr_array([col.ptr] * 2), sizes([2 ** 31 - 2, 1]), 2, 8, 1, out.ptr, rej.ptr),
        "order 2": (one, n64, 1, 8, 2, out.ptr, rej.ptr),
        "null column table": (None, n64, 1, 8, 1, out.ptr, rej.ptr), "null lengths": (one, None, 1, 8, 1, out.ptr, rej.ptr),
        "null column": (L.ptr_array([col.ptr, 0]), sizes([64, 64]), 2, 8, 1, out.ptr, rej.ptr),
        "null out": (one, n64, 1, 8, 1, None, rej.ptr),
        "out is a column": (L.ptr_array([col.ptr, out.ptr]), sizes([64, 64]), 2, 8, 1, out.ptr, rej.ptr),
        "out overlaps a column": (L.ptr_array([out.ptr + 512]), sizes([64]), 1, 8, 1, out.ptr, rej.ptr),
        "n_rejected inside out": (one, n64, 1, 8, 1, out.ptr, out.ptr + 16),
    }
    for name, args in cases.items():
        with pytest.raises(L.TstwoError, match="^lookup: ") as e:
            L.call("tstwo_lookup_multiplicities", *args)
        assert e.value.code == BAD_ARG, name
    for name, args in {"null out": (None, 8), "log_size 0": (out.ptr, 0), "log_size 29": (out.ptr, 29)}.items():
        with pytest.raises(L.TstwoError, match="^lookup: ") as e:
            L.call("tstwo_coset_iota", *args)
        assert e.value.code == BAD_ARG, name
    assert (out.to_numpy() == 0x25A5A5A5).all() and rej.to_numpy()[0] == 99
    with pytest.raises(ValueError, match="order"):
        LG.lookup_multiplicities(8, col, order="rows")
    # and the entry works on the same arguments once they are within the limits
    got, n_rej = count(8, [col.ptr], [64], "natural", out=out)
    assert n_rej == 0 and np.array_equal(got, np.bincount(np.arange(64), minlength=256))


def _capture(fn):
    L.sync()
    L.call("tstwo_graph_begin_capture")
    try:
        with pytest.raises(L.TstwoError, match="^lookup: .*graph capture"):
            fn()
    finally:
        h = C.c_void_p()
        try:
            L.call("tstwo_graph_end_capture", C.byref(h))
        except L.TstwoError:
            pass
        if h.value:
            L.call("tstwo_graph_destroy", h)


def test_entries_are_refused_during_graph_capture():
    col = HipColumn(np.arange(64, dtype=np.uint32))
    out = HipColumn.zeros(256)
    ptrs, lens = L.ptr_array([col.ptr]), sizes([64])
    _capture(lambda: L.call("tstwo_lookup_multiplicities", ptrs, lens, 1, 8, 0, out.ptr, None))
    _capture(lambda: L.call("tstwo_coset_iota", out.ptr, 8))
    L.call("tstwo_lookup_multiplicities", ptrs, lens, 1, 8, 0, out.ptr, None)
    assert np.array_equal(out.to_numpy(), np.bincount(np.arange(64), minlength=256))


# ------------------------------------------------------------------ end to end
def _evals(cols, log):
    d = CanonicCoset(log).circleDomain()
    return [HipCircleEvaluation(d, c if isinstance(c, HipColumn) else HipColumn(np.asarray(c, dtype=np.uint32))) for c in cols]


def _commit(scheme, evs, channel):
    tb = scheme.tree_builder()
    tb.extend_evals(evs)
    tb.commit(channel)


def _range_check_proof(log_range, log_values, device):
    """The range-check pair of test_gpu_logup.py::_range_check by the caller protocol.  device: the value columns are device
    columns, the multiplicities are counted and the table column is built there, and both interaction traces come from
    derive_interaction_trace; else everything comes from the host functions.  Returns (components, proof, config, claimed sums)."""
    rng = np.random.default_rng(3)
    config = PcsConfig(5, FriConfig(0, 1, 3))
    v0 = rng.integers(0, 1 << log_range, size=1 << log_values).astype(np.uint32)
    v1 = rng.integers(0, 1 << log_range, size=1 << log_values).astype(np.uint32)
    if device:
        v0, v1 = HipColumn(v0), HipColumn(v1)
        mult = F.range_check_multiplicities_device(log_range, v0, v1)
        table = F.range_check_table_column_device(log_range)
    else:
        mult = F.range_check_multiplicities(log_range, v0, v1)
        table = F.range_check_table_column(log_range)
    tw = precompute_twiddles(CanonicCoset(max(log_range + 1, log_values + 2, 10) + 1).circleDomain().halfCoset)
    ch = Blake2sChannel()
    scheme = CommitmentSchemeProver(config, tw)
    _commit(scheme, _evals([table], log_range), ch)
    _commit(scheme, _evals([mult], log_range) + _evals([v0, v1], log_values), ch)
    le = LG.LookupElements.draw(ch, 1)
    if device:
        t_inter, t_sum = LG.derive_interaction_trace(F.RangeCheckTableEval(log_range, le), [mult], [table])
        v_inter, v_sum = LG.derive_interaction_trace(F.RangeCheckValuesEval(log_values, le), [v0, v1])
    else:
        t_inter, t_sum = F.range_check_table_interaction_trace(log_range, mult, le)
        v_inter, v_sum = F.range_check_values_interaction_trace(log_values, v0, v1, le)
    ch.mix_felts([t_sum, v_sum])
    _commit(scheme, t_inter + v_inter, ch)
    alloc = A.TraceLocationAllocator()
    comps = [F.FrameworkComponent(F.RangeCheckTableEval(log_range, le), alloc, [0], claimed_sum=t_sum),
             F.FrameworkComponent(F.RangeCheckValuesEval(log_values, le), alloc, claimed_sum=v_sum)]
    return comps, prove(comps, ch, scheme), config, (t_sum, v_sum)


def test_range_check_proof_with_device_multiplicities():
    log_range, log_values = 6, 7
    comps, proof, config, (t_sum, v_sum) = _range_check_proof(log_range, log_values, device=True)
    assert t_sum.add(v_sum) == QM31.zero()
    ch = Blake2sChannel()
    v = CommitmentSchemeVerifier(config)
    sizes_ = A.Components(comps, 1).column_log_sizes()
    v.commit(proof.commitments[0], [log_range], ch)
    v.commit(proof.commitments[1], sizes_[1], ch)
    LG.LookupElements.draw(ch, 1)
    ch.mix_felts([t_sum, v_sum])
    v.commit(proof.commitments[2], sizes_[2], ch)
    verify(comps, ch, v, proof)
    _, host_proof, _, host_sums = _range_check_proof(log_range, log_values, device=False)
    assert [bytes(c) for c in proof.commitments] == [bytes(c) for c in host_proof.commitments]
    assert (t_sum, v_sum) == host_sums


def test_main_tree_with_device_multiplicities_first_global_log():
    """The same at the first table size of the global branch: the multiplicity column and the root of the main tree."""
    log_range, log_values = LP.FIRST_GLOBAL_LOG, 10
    rng = np.random.default_rng(4)
    v0, v1 = (rng.integers(0, 1 << log_range, size=1 << log_values).astype(np.uint32) for _ in range(2))
    d0, d1 = HipColumn(v0), HipColumn(v1)
    mult = F.range_check_multiplicities_device(log_range, d0, d1)
    host_mult = F.range_check_multiplicities(log_range, v0, v1)
    assert np.array_equal(mult.to_numpy(), host_mult)
    tw = precompute_twiddles(CanonicCoset(log_range + 2).circleDomain().halfCoset)
    roots = []
    for m, a, b in ((mult, d0, d1), (host_mult, v0, v1)):
        ch = Blake2sChannel()
        scheme = CommitmentSchemeProver(1, tw)
        _commit(scheme, _evals([m], log_range) + _evals([a, b], log_values), ch)
        roots.append(bytes(scheme.roots()[0]))
    assert roots[0] == roots[1]

"""-m gpu: tstwo_lookup_multiplicities_keyed (tstwo_amd/csrc/lookup.hip) word for word against tests/lookup_keyed_model.py, in both
orders and with the rejected count, on the shapes of tests/lookup_keyed_plan.py — which kernel paths each shape reaches is
accounted for without a GPU in test_cpu_lookup_keyed_plan.py — then limbs, weights, the combining of equal keys within a wave,
repeatability, parity with tstwo_lookup_multiplicities, guard bands and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import arena as AR
import lookup_keyed_model as KM
import lookup_keyed_plan as KP
from tstwo_amd import _lib as L
from tstwo_amd import logup as LG
from tstwo_amd.backend import HipColumn

pytestmark = pytest.mark.gpu

P = L.P
BAD_ARG = 7                      # include/tstwo_hip.h TSTWO_ERR_BAD_ARG
SENTINEL = 0xA5A5A5A5
FILL = 0x25A5A5A5
# (branch, accumulator width) -> log_range of a table just inside it
BRANCHES = {("LDS", "acc32"): 14, ("GLOBAL", "acc32"): 15, ("LDS", "acc64"): 13, ("GLOBAL", "acc64"): 14}
BRANCH_IDS = [f"{b}-{a}" for b, a in BRANCHES]


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


class Placed:
    """The columns of a call in ONE device buffer (one upload): column i starts offsets[i] words past a 16-byte boundary.  A raw
    buffer, not a HipColumn: limbs and weights may be any 32-bit word here."""

    def __init__(self, arrays, offsets):
        starts, cur = [], 0
        for a, off in zip(arrays, offsets):
            cur = (cur + 3) // 4 * 4 + off
            starts.append(cur)
            cur += len(a)
        image = np.zeros(max(cur, 1), dtype=np.uint32)
        for a, s in zip(arrays, starts):
            image[s:s + len(a)] = a
        self.buf = L.DeviceBuffer(4 * image.size)
        assert self.buf.ptr % 16 == 0
        self.buf.upload(image)
        self.addrs = [self.buf.ptr + 4 * s for s in starts]


def descriptors(groups, offsets=None):
    """groups: [(limbs = [(array, bits)], weight array or None)]; offsets: per group (limb offsets, weight offset) in words.
    Returns (the ctypes table, what keeps the columns alive)."""
    arrays, offs = [], []
    for g, (limbs, weight) in enumerate(groups):
        lo, wo = offsets[g] if offsets else ((0,) * len(limbs), 0)
        for (a, _), o in zip(limbs, lo):
            arrays.append(np.asarray(a, dtype=np.uint32))
            offs.append(o)
        if weight is not None:
            arrays.append(np.asarray(weight, dtype=np.uint32))
            offs.append(wo)
    placed = Placed(arrays, offs)
    table, addrs = (L.LookupGroup * max(len(groups), 1))(), iter(placed.addrs)
    for d, (limbs, weight) in zip(table, groups):
        for j, (a, bits) in enumerate(limbs):
            d.limbs[j], d.bits[j] = next(addrs), bits
        d.n_limbs, d.len = len(limbs), len(limbs[0][0])
        d.weight = next(addrs) if weight is not None else None
    return table, placed


def run(log_range, table, n_groups, order, out=None, with_rejected=True):
    """One call of the entry into `out` (a fresh sentinel-filled column by default): (words, n_rejected or None)."""
    if out is None:
        out = HipColumn(np.full(1 << log_range, FILL, dtype=np.uint32))
    rej = HipColumn(np.array([12345], dtype=np.uint32)) if with_rejected else None
    L.call("tstwo_lookup_multiplicities_keyed", table, n_groups, log_range, KM.ORDERS[order], out.ptr, rej.ptr if rej else None)
    return out.to_numpy()[:1 << log_range], (int(rej.to_numpy()[0]) if rej else None)


def check_both_orders(log_range, groups, offsets=None, want_rejected=None):
    table, keep = descriptors(groups, offsets)
    natural = None
    for order in ("coset", "natural"):
        want, rejected = KM.multiplicities(log_range, groups, order)
        if want_rejected is not None:
            assert rejected == want_rejected
        got, n_rej = run(log_range, table, len(groups), order)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{order}: {bad.size} wrong words, the first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"
        assert n_rej == rejected
        natural = want
    return natural


def draw(shapes, rng, weights="01"):
    """Values for a call of KP.GroupShapes: limbs inside their widths, weights 0/1 (or `weights`)."""
    groups, offsets = [], []
    for s in shapes:
        limbs = [(rng.integers(0, 1 << b, size=s.rows, dtype=np.uint32), b) for b in s.bits]
        weight = None
        if s.weight is not None:
            weight = rng.integers(0, 2, size=s.rows, dtype=np.uint32) if weights == "01" else weights(s.rows)
        groups.append((limbs, weight))
        offsets.append((s.offsets, s.weight or 0))
    return groups, offsets


# ------------------------------------------------------------------ parity with the model on the plan's shapes
@pytest.mark.parametrize("log_range,weighted", KP.TABLES, ids=[f"{lg}{'w' if w else ''}" for lg, w in KP.TABLES])
def test_lengths_alignments_and_group_counts(log_range, weighted):
    rng = np.random.default_rng(7000 + 2 * log_range + weighted)
    for name, shapes in KP.parity_calls(log_range, weighted).items():
        groups, offsets = draw(shapes, rng)
        check_both_orders(log_range, groups, offsets, want_rejected=0)


@pytest.mark.parametrize("log_range,weighted", KP.TABLES[2:4] + KP.TABLES[6:8], ids=BRANCH_IDS)
def test_grid_stride_past_the_wrap_point(log_range, weighted):
    """64 groups, one of the plan's wrap point + 1029 rows: its first lanes take a second unit, the last of them a partial one."""
    shapes = KP.wrap_call(log_range, weighted)
    assert "wrap" in KP.reaches(log_range, KP.shape_groups(shapes))[1]
    groups, offsets = draw(shapes, np.random.default_rng(70 + log_range + weighted))
    check_both_orders(log_range, groups, offsets, want_rejected=0)


# ------------------------------------------------------------------ limbs
@pytest.mark.parametrize("bits", [(5,), (3, 2), (9, 5), (2, 5, 3), (1, 6, 2, 4), (4, 1, 7, 3), (6, 5, 4, 3)], ids=str)
def test_limbs_of_unequal_widths(bits):
    log_range = sum(bits)
    rng = np.random.default_rng(sum(b << (5 * j) for j, b in enumerate(bits)))
    rows = 1031
    limbs = [(rng.integers(0, 1 << b, size=rows, dtype=np.uint32), b) for b in bits]
    natural = check_both_orders(log_range, [(limbs, None)], want_rejected=0)
    key = sum(a.astype(np.int64) << sum(bits[:j]) for j, (a, _) in enumerate(limbs))
    assert np.array_equal(natural, np.bincount(key, minlength=1 << log_range))
    # every limb at its largest value lands in the last bin, and one above it is rejected: per limb, in each limb's turn
    for j, b in enumerate(bits):
        edge = [(np.array([(1 << bb) - 1, (1 << bb) - 1 + (jj == j)], dtype=np.uint32), bb) for jj, bb in enumerate(bits)]
        natural = check_both_orders(log_range, [(edge, None)], want_rejected=1)
        assert natural[-1] == 1 and natural.sum() == 1


@pytest.mark.parametrize("weighted", [False, True])
def test_a_limb_outside_its_width_does_not_alias(weighted):
    """a = 2^bits_a, b = 0 would be the bin of (0, 1) after a + 2^bits_a b: it is rejected and that bin stays empty; a row with
    two bad limbs is rejected once."""
    ba, bb = 8, 6
    a = np.array([1 << ba, 5, 1 << ba, 0xFFFFFFFF, 7], dtype=np.uint32)
    b = np.array([0, 2, 1 << bb, 0xFFFFFFFF, 63], dtype=np.uint32)
    w = np.array([1, 1, 3, 2, 4], dtype=np.uint32) if weighted else None
    natural = check_both_orders(ba + bb, [([(a, ba), (b, bb)], w)], want_rejected=3)
    assert natural[1 << ba] == 0 and natural[5 + (2 << ba)] == 1 and natural[7 + (63 << ba)] == (4 if weighted else 1)
    assert natural.sum() == (5 if weighted else 2)


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("log_range", [BRANCHES["LDS", "acc64"], BRANCHES["GLOBAL", "acc64"]], ids=["LDS", "GLOBAL"])
def test_weights(log_range):
    rng = np.random.default_rng(300 + log_range)
    rows, n = 4099, 1 << log_range
    v = rng.integers(0, n, size=rows, dtype=np.uint32)
    junk = np.full(rows, 0xFFFFFFFF, dtype=np.uint32)
    # all 0: every bin 0 and nothing rejected, whatever the limbs hold
    natural = check_both_orders(log_range, [([(junk, log_range)], np.zeros(rows, dtype=np.uint32))], want_rejected=0)
    assert not natural.any()
    # 0/1, the disabled rows out of range
    w = rng.integers(0, 2, size=rows, dtype=np.uint32)
    natural = check_both_orders(log_range, [([(np.where(w, v, junk), log_range)], w)], want_rejected=0)
    assert np.array_equal(natural, np.bincount(v[w != 0], minlength=n))
    # three rows of P - 1 in one bin are -3: 32-bit accumulators wrap here
    natural = check_both_orders(log_range, [([(np.full(3, n - 1, dtype=np.uint32), log_range)], np.full(3, P - 1, dtype=np.uint32))])
    assert natural[n - 1] == P - 3
    # 2^16 rows of P - 1 in one bin
    natural = check_both_orders(log_range, [([(np.full(1 << 16, 9, dtype=np.uint32), log_range)], np.full(1 << 16, P - 1, dtype=np.uint32))])
    assert natural[9] == P - (1 << 16)
    # weight words >= P are added as they are and reduced with the sum
    big = np.array([P, P + 1, 0xFFFFFFFF, 0x80000000, 5], dtype=np.uint32)
    natural = check_both_orders(log_range, [([(np.array([1, 1, 2, 2, 2], dtype=np.uint32), log_range)], big)], want_rejected=0)
    assert natural[1] == 1 and natural[2] == (0xFFFFFFFF + 0x80000000 + 5) % P
    # random full words
    w = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)
    check_both_orders(log_range, [([(v, log_range)], w)])
    # a zero-weight row out of range is not rejected, a weight-1 row out of range is
    natural = check_both_orders(log_range, [([(np.array([n, n, 3], dtype=np.uint32), log_range)], np.array([0, 1, 1], dtype=np.uint32))],
                                want_rejected=1)
    assert natural[3] == 1 and natural.sum() == 1


@pytest.mark.parametrize("log_range", [13, 14, 15])
def test_a_null_weight_group_beside_a_weighted_one(log_range):
    rng = np.random.default_rng(41 + log_range)
    groups, offsets = draw(KP.mixed_call(log_range), rng, weights=lambda rows: rng.integers(0, P, size=rows, dtype=np.uint32))
    assert groups[0][1] is None and groups[1][1] is not None
    check_both_orders(log_range, groups, offsets, want_rejected=0)


# ------------------------------------------------------------------ combining equal keys of a wave
@pytest.mark.parametrize("where", list(BRANCHES), ids=BRANCH_IDS)
@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("rows", [63, 64, 65, 1 << 16])
def test_every_row_of_one_key(where, which, rows):
    log_range = BRANCHES[where]
    k = 0 if which == "first" else (1 << log_range) - 1
    w = np.ones(rows, dtype=np.uint32) if where[1] == "acc64" else None
    natural = check_both_orders(log_range, [([(np.full(rows, k, dtype=np.uint32), log_range)], w)], want_rejected=0)
    assert natural[k] == rows and natural.sum() == rows


@pytest.mark.parametrize("where", list(BRANCHES), ids=BRANCH_IDS)
def test_combining_patterns(where):
    log_range, n = BRANCHES[where], 1 << BRANCHES[where]
    weighted = where[1] == "acc64"
    rng = np.random.default_rng(900 + log_range + weighted)

    def weights(a):
        return np.asarray(a, dtype=np.uint32) if weighted else None

    rows = 1024 + 4 * 37 + 3                      # whole waves, a partial wave and a partial unit
    # one key, weights 1, 2, 3, ...: the sum is of the lanes' own weights, not the count times the leader's
    if weighted:
        natural = check_both_orders(log_range, [([(np.full(rows, 77, dtype=np.uint32), log_range)], weights(np.arange(1, rows + 1)))])
        assert natural[77] == rows * (rows + 1) // 2
        huge = (np.arange(rows, dtype=np.uint64) * 0x01000193 + 0xFFFF0000).astype(np.uint32)          # sums that pass 2^32 within a wave
        natural = check_both_orders(log_range, [([(np.full(rows, 78, dtype=np.uint32), log_range)], huge)])
        # every wave holds a weight of 2^26 or more, so its sum goes through the two 16-bit halves; the bin is the exact sum mod P
        assert all((huge[i:i + 256] >= 1 << 26).any() for i in range(0, rows, 256)) and sum(map(int, huge[:64])) >= 1 << 32
        assert natural[78] == sum(map(int, huge)) % P and natural.sum() == natural[78]
    # a uniform wave with one lane rejected, one lane of weight 0 (where there are weights) and one lane of another key
    v = np.full(rows, n - 2, dtype=np.uint32)
    w = np.full(rows, 3, dtype=np.uint32)
    v[4 * 5 + 1], v[4 * 9 + 2], w[4 * 17] = n, 11, 0            # rows of lanes 5, 9 and 17 of the first wave
    v[4 * 70], v[4 * 64] = 0xFFFFFFFF, 12                       # and in the second wave the FIRST lane holds the other key
    natural = check_both_orders(log_range, [([(v, log_range)], weights(w))], want_rejected=2)
    assert natural[11] == natural[12] == (3 if weighted else 1)
    assert natural[n - 2] == (3 * (rows - 5) if weighted else rows - 4)
    # two keys alternating: row by row, and lane by lane
    for period in (1, 4):
        v = np.where((np.arange(rows) // period) % 2, 5, n - 1).astype(np.uint32)
        check_both_orders(log_range, [([(v, log_range)], weights(rng.integers(1, 100, size=rows)))], want_rejected=0)
    # the four rows of each unit equal while neighbouring lanes differ
    v = np.repeat(rng.permutation(n)[:(rows + 3) // 4], 4)[:rows].astype(np.uint32)
    natural = check_both_orders(log_range, [([(v, log_range)], weights(np.full(rows, 2)))], want_rejected=0)
    assert set(np.unique(natural)) <= {0, 3, 4, 6, 8}
    # more distinct keys in a wave than there are rounds, each several times
    v = (np.arange(rows) % 11).astype(np.uint32)
    check_both_orders(log_range, [([(v, log_range)], weights(rng.integers(0, 3, size=rows)))], want_rejected=0)
    # every bin exactly once, from a permutation, split over two limbs
    lo = log_range // 2
    perm = rng.permutation(n).astype(np.uint32)
    natural = check_both_orders(log_range, [([(perm & ((1 << lo) - 1), lo), (perm >> lo, log_range - lo)], weights(np.ones(n)))], want_rejected=0)
    assert (natural == 1).all()


# ------------------------------------------------------------------ repeatability and scratch
def test_same_call_twice_then_a_smaller_table_into_a_prefix():
    """The entry zeroes what it accumulates in itself: a second call into the same column gives the same words, and a smaller
    table written into a prefix of that column finds no stale accumulator, whatever the order of branches and widths."""
    rng = np.random.default_rng(31)
    out = HipColumn(np.full(1 << 16, FILL, dtype=np.uint32))
    for logs in ((16, 3, 16), (15, 14, 13, 2, 14, 13)):
        for weighted in (False, True):
            for log_range in logs:
                v = rng.integers(0, 1 << log_range, size=5000, dtype=np.uint32)
                w = rng.integers(0, P, size=5000, dtype=np.uint32) if weighted else None
                groups = [([(v, log_range)], w), ([(v[:3], log_range)], None)]
                table, keep = descriptors(groups)
                want, _ = KM.multiplicities(log_range, groups, "coset")
                first, _ = run(log_range, table, 2, "coset", out=out)
                second, _ = run(log_range, table, 2, "coset", out=out)
                assert np.array_equal(first, want) and np.array_equal(second, want), (log_range, weighted)


# ------------------------------------------------------------------ parity with the old entry
@pytest.mark.parametrize("log_range", [1, 2, 8, 14, 15, 16])
def test_one_limb_without_weights_is_the_old_entry(log_range):
    rng = np.random.default_rng(100 + log_range)
    arrays = [rng.integers(0, 1 << log_range, size=n, dtype=np.uint32) for n in (0, 1, 255, 257, 4099)]
    arrays[2][254], arrays[4][5] = 1 << log_range, P - 1                   # two words outside the range: skipped by both
    cols = [HipColumn(a) for a in arrays]
    for order in ("coset", "natural"):
        old = LG.lookup_multiplicities(log_range, *cols, order=order, check=False).to_numpy()
        new = LG.lookup_multiplicities_keyed([LG.LookupGroup([(c, log_range)]) for c in cols], order=order, check=False).to_numpy()
        assert np.array_equal(old, new)
        want, rejected = KM.multiplicities(log_range, [([(a, log_range)], None) for a in arrays], order)
        assert np.array_equal(new, want) and rejected == 2


# ------------------------------------------------------------------ the Python entry
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


def test_python_entry_check_and_no_read_back(monkeypatch):
    a = np.array([1, 2, 300, 3], dtype=np.uint32)
    b = np.array([0, 1, 0, 9], dtype=np.uint32)
    en = np.array([1, 1, 0, 2], dtype=np.uint32)
    ca, cb, cen = HipColumn(a), HipColumn(b), HipColumn(en)
    want, _ = KM.multiplicities(12, [([(a, 8), (b, 4)], en)], "coset")
    got = LG.lookup_multiplicities_keyed([LG.LookupGroup([(ca, 8), (cb, 4)], weight=cen)])
    assert np.array_equal(got.to_numpy(), want)
    assert np.array_equal(LG.lookup_multiplicities_keyed([LG.LookupGroup([(a, 8), (b, 4)], weight=en)]).to_numpy(), want)      # arrays are uploaded
    with pytest.raises(ValueError, match="a checked value lies outside the range"):
        LG.lookup_multiplicities_keyed([LG.LookupGroup([(ca, 8), (cb, 4)])])
    with pytest.raises(ValueError, match="log_range"):
        LG.lookup_multiplicities_keyed([LG.LookupGroup([(ca, 8), (cb, 4)]), LG.LookupGroup([(ca, 8)])])
    with pytest.raises(ValueError, match="order"):
        LG.lookup_multiplicities_keyed([LG.LookupGroup([(ca, 8)])], order="rows")
    with pytest.raises(ValueError, match="one length"):
        LG.LookupGroup([(ca, 8), (HipColumn(a[:3]), 4)])
    L.sync()
    counter = SyncCounter(monkeypatch)
    out = LG.lookup_multiplicities_keyed([LG.LookupGroup([(ca, 8), (cb, 4)])], check=False)
    assert counter.n == 0 and "tstwo_lookup_multiplicities_keyed" in counter.names
    monkeypatch.undo()
    want, rejected = KM.multiplicities(12, [([(a, 8), (b, 4)], None)], "coset")
    assert rejected == 1 and np.array_equal(out.to_numpy(), want)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("where", list(BRANCHES), ids=BRANCH_IDS)
@pytest.mark.parametrize("order", ["coset", "natural"])
@pytest.mark.parametrize("with_rejected", [True, False])
def test_nothing_outside_the_outputs_is_written(where, order, with_rejected):
    log_range, weighted = BRANCHES[where], where[1] == "acc64"
    rng = np.random.default_rng(88 + log_range + weighted)
    lo = 5
    lens, offsets = (4099, 257, 0, 1), ((0, 4, 8), (4, 0, 0), (8, 12, 4), (12, 8, 0))          # bytes: limb 0, limb 1, weight
    regions, groups = [], []
    for g, (n, offs) in enumerate(zip(lens, offsets)):
        a, b = rng.integers(0, 1 << lo, size=n, dtype=np.uint32), rng.integers(0, 1 << (log_range - lo), size=n, dtype=np.uint32)
        w = rng.integers(0, 3, size=n, dtype=np.uint32) if weighted and g != 1 else None
        if g == 0:
            a[7], b[256], a[300], b[300] = 1 << lo, P - 1, 0xFFFFFFFF, 0xFFFFFFFF            # three rows outside the range
            if w is not None:
                w[7], w[256], w[300] = 1, 2, 0                                           # the third is switched off
        regions += [AR.rin(f"a{g}", a, offset=offs[0]), AR.rin(f"b{g}", b, offset=offs[1])]
        if w is not None:
            regions.append(AR.rin(f"w{g}", w, offset=offs[2]))
        groups.append(([(a, lo), (b, log_range - lo)], w))
    regions += [AR.rout("out", 1 << log_range), AR.rout("n_rejected", 1, offset=4)]
    with AR.Arena(regions) as ar:
        table = (L.LookupGroup * 4)()
        for g, (d, (limbs, w)) in enumerate(zip(table, groups)):
            d.limbs[0], d.limbs[1], d.bits[0], d.bits[1] = ar.addr(f"a{g}"), ar.addr(f"b{g}"), lo, log_range - lo
            d.n_limbs, d.len, d.weight = 2, lens[g], ar.addr(f"w{g}") if w is not None else None
        L.call("tstwo_lookup_multiplicities_keyed", table, 4, log_range, KM.ORDERS[order], ar.ptr("out"),
               ar.ptr("n_rejected") if with_rejected else None)
        res = ar.check()
    want, rejected = KM.multiplicities(log_range, groups, order)
    assert rejected == (2 if weighted else 3) and np.array_equal(res["out"], want)
    assert res["n_rejected"][0] == (rejected if with_rejected else SENTINEL)


# ------------------------------------------------------------------ arguments
def _table(*groups):
    """groups: (limbs = [(address, bits)], weight address or None, len)."""
    t = (L.LookupGroup * max(len(groups), 1))()
    for d, (limbs, weight, n) in zip(t, groups):
        for j, (addr, bits) in enumerate(limbs[:4]):
            d.limbs[j], d.bits[j] = addr, bits
        d.n_limbs, d.weight, d.len = len(limbs), weight, n
    return t


def test_every_limit_is_refused_before_anything_is_launched():
    col = HipColumn(np.arange(64, dtype=np.uint32) % 16)
    wcol = HipColumn(np.ones(64, dtype=np.uint32))
    out = HipColumn(np.full(256, FILL, dtype=np.uint32))
    rej = HipColumn(np.array([99], dtype=np.uint32))
    g = ([(col.ptr, 4), (col.ptr, 4)], wcol.ptr, 64)
    five = ([(col.ptr, 2), (col.ptr, 2), (col.ptr, 2), (col.ptr, 1), (col.ptr, 1)], None, 64)
    cases = {
        "log_range 0": ((_table(g), 1, 0, 1, out.ptr, rej.ptr), "log_range must be 1 to 28"),
        "log_range 29": ((_table(([(col.ptr, 28), (col.ptr, 1)], None, 64)), 1, 29, 1, out.ptr, rej.ptr), "log_range must be 1 to 28"),
        "no group": ((_table(g), 0, 8, 1, out.ptr, rej.ptr), "1 to 64 groups"),
        "65 groups": ((_table(*[g] * 65), 65, 8, 1, out.ptr, rej.ptr), "1 to 64 groups"),
        "no limb": ((_table(([], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "1 to 4 limbs per group"),
        "5 limbs": ((_table(five), 1, 8, 1, out.ptr, rej.ptr), "1 to 4 limbs per group"),
        "a limb of 0 bits": ((_table(([(col.ptr, 8), (col.ptr, 0)], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "every limb needs at least 1 bit"),
        "bits short of log_range": ((_table(([(col.ptr, 4), (col.ptr, 3)], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "the bits of every group must add up to log_range"),
        "second group's bits": ((_table(g, ([(col.ptr, 4), (col.ptr, 5)], None, 64)), 2, 8, 1, out.ptr, rej.ptr), "the bits of every group must add up to log_range"),
        "too many rows": ((_table(([(col.ptr, 8)], None, 2 ** 31 - 1)), 1, 8, 1, out.ptr, rej.ptr), "more than 2\\^31 - 2 rows"),
        "too many rows in all": ((_table(([(col.ptr, 8)], None, 2 ** 31 - 2), ([(col.ptr, 8)], None, 1)), 2, 8, 1, out.ptr, rej.ptr), "more than 2\\^31 - 2 rows"),
        "order 2": ((_table(g), 1, 8, 2, out.ptr, rej.ptr), "order must be 0 \\(natural\\) or 1 \\(coset\\)"),
        "null table": ((None, 1, 8, 1, out.ptr, rej.ptr), "null"),
        "null limb": ((_table(([(col.ptr, 4), (None, 4)], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "null"),
        "null out": ((_table(g), 1, 8, 1, None, rej.ptr), "null"),
        "out is a limb": ((_table(([(col.ptr, 4), (out.ptr, 4)], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "out overlaps a limb or weight column"),
        "out overlaps a limb": ((_table(([(out.ptr + 512, 8)], None, 64)), 1, 8, 1, out.ptr, rej.ptr), "out overlaps a limb or weight column"),
        "out overlaps a weight column": ((_table(([(col.ptr, 8)], out.ptr + 1020, 64)), 1, 8, 1, out.ptr, rej.ptr), "out overlaps a limb or weight column"),
        "n_rejected inside out": ((_table(g), 1, 8, 1, out.ptr, out.ptr + 16), "n_rejected lies inside out"),
    }
    for name, (args, text) in cases.items():
        with pytest.raises(L.TstwoError, match="^lookup: .*" + text) as e:
            L.call("tstwo_lookup_multiplicities_keyed", *args)
        assert e.value.code == BAD_ARG, name
    assert (out.to_numpy() == FILL).all() and rej.to_numpy()[0] == 99
    # and the entry works on the same arguments once they are within the limits
    got, n_rej = run(8, _table(g), 1, "natural", out=out)
    k = np.arange(64) % 16
    assert n_rej == 0 and np.array_equal(got, np.bincount(k + 16 * k, minlength=256))


def test_the_entry_is_refused_during_graph_capture():
    """Refused with its text, and the capture stays usable: a copy recorded after the refusal replays from the graph."""
    col = HipColumn(np.arange(64, dtype=np.uint32))
    out, copy = HipColumn.zeros(256), HipColumn.zeros(64)
    table = _table(([(col.ptr, 8)], None, 64))
    L.sync()
    L.call("tstwo_graph_begin_capture")
    h = C.c_void_p()
    try:
        with pytest.raises(L.TstwoError, match="^lookup: .*graph capture") as e:
            L.call("tstwo_lookup_multiplicities_keyed", table, 1, 8, 0, out.ptr, None)
        assert e.value.code == BAD_ARG
        L.call("tstwo_copy", C.c_void_p(copy.ptr), C.c_void_p(col.ptr), 4 * 64)
    finally:
        L.call("tstwo_graph_end_capture", C.byref(h))
    assert h.value
    try:
        L.sync()
        assert not copy.to_numpy().any() and not out.to_numpy().any()           # recorded, not run; the refused call left no trace
        L.call("tstwo_graph_launch", h)
        assert np.array_equal(copy.to_numpy(), np.arange(64))
    finally:
        L.call("tstwo_graph_destroy", h)
    L.call("tstwo_lookup_multiplicities_keyed", table, 1, 8, 0, out.ptr, None)
    assert np.array_equal(out.to_numpy(), np.bincount(np.arange(64), minlength=256))

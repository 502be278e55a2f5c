"""What tstwo_lookup_multiplicities_keyed computes, in numpy and Python integers (no GPU, no library call): the -m gpu files
compare with this, tests/test_cpu_lookup_keyed_plan.py compares it with np.bincount and range_check_multiplicities.

A group is (limbs, weight): limbs = [(array of words, bits), ...] with the least significant limb first, weight = an array of
words or None (every row weighs 1).  A row of weight 0 is skipped unchecked; a row of non-zero weight with a limb >= 2^bits is
rejected, once; every other row adds its weight, as the unsigned integer it is, to the bin of its key.  The sums are exact
(uint64: fewer than 2^31 rows of weight below 2^32) and reduced mod P at the end."""
import numpy as np

from tstwo_amd import constraint_framework as F

P = 2 ** 31 - 1
ORDERS = {"natural": 0, "coset": 1}


def multiplicities(log_range, groups, order):
    """(the column of 2^log_range words the entry writes, the number of rows it rejects)."""
    n = 1 << log_range
    sums, rejected = np.zeros(n, dtype=np.uint64), 0
    for limbs, weight in groups:
        assert sum(b for _, b in limbs) == log_range
        rows = len(limbs[0][0])
        w = np.ones(rows, dtype=np.uint64) if weight is None else np.asarray(weight).astype(np.uint64)
        assert w.size == rows
        live = w != 0
        ok = np.ones(rows, dtype=bool)
        key, shift = np.zeros(rows, dtype=np.uint64), 0
        for col, bits in limbs:
            col = np.asarray(col).astype(np.uint64)
            assert col.size == rows
            ok &= col < (1 << bits)
            key |= (col & np.uint64((1 << bits) - 1)) << np.uint64(shift)
            shift += bits
        rejected += int((live & ~ok).sum())
        use = live & ok
        np.add.at(sums, key[use].astype(np.int64), w[use])
    out = np.empty(n, dtype=np.uint32)
    positions = F._coset_positions(log_range) if ORDERS.get(order, order) == 1 else np.arange(n)
    out[positions] = (sums % np.uint64(P)).astype(np.uint32)
    return out, rejected

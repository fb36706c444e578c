"""krr_segmented_wquantile restated in plain Python, for the tests of the kernel and of the layers
above it.  Nothing here comes from the code under test.

A series of L slots and a table of integer weights indexed by AGE:

    slot i has age a = L - 1 - i (the last slot is "now") and weight table[min(a, len(table) - 1)];
    P = the present slots (every slot, or the non-NaN ones in the gapped layout), W = sum_P w;
    samples are ordered by the key of their bits (okey: -0.0 before +0.0, +-Inf ordinary values);
    with p = p_num / p_den percent, the answer is the smallest present sample v, with its own
    bits, such that C(v) * (100 * p_den) >= W * p_num, C(v) = the summed weight of the present
    samples whose key is <= v's.  Python integers: every product and sum is exact.

W == 0 (no sample, or no weight): the quiet NaN.  A NaN sample in the compact layout:
KRR_FLAG_NAN, the quiet NaN and W reported as 0.  With unit weights the rule is
sorted(x)[ceil(n p / 100) - 1]."""
import struct
from decimal import Decimal
from fractions import Fraction

import numpy as np

EMPTY, NAN = 4, 1
QNAN = 0x7FF8000000000000
MASK = (1 << 64) - 1
MAX_PASSES = 1 + -(-64 // 10) + 1  # one totals pass, ceil(64 / log2(1024 bins)) histogram passes, one collect


def bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def okey(u: int) -> int:
    """The kernels' order-preserving key of a float64's bits."""
    return (~u & MASK) if u >> 63 else (u | 1 << 63)


def fraction_of(percentile) -> tuple:
    f = Fraction(Decimal(str(percentile)))
    return f.numerator, f.denominator


def weights_of(L: int, table) -> list:
    """The weight of every slot of a series of L slots."""
    n = len(table)
    return [int(table[min(L - 1 - i, n - 1)]) for i in range(L)]


def wquantile_one(x, table, p_num: int, p_den: int):
    """(answer's bits, W) of one series whose NaN entries are absent slots."""
    xs = np.asarray(x, dtype=np.float64).tolist()
    pairs = sorted((okey(bits(v)), w, bits(v)) for v, w in zip(xs, weights_of(len(xs), table)) if v == v)
    W = sum(w for _, w, _ in pairs)
    if W == 0:
        return QNAN, 0
    c = 0
    for i, (k, w, b) in enumerate(pairs):
        c += w
        if i + 1 < len(pairs) and pairs[i + 1][0] == k:
            continue  # C(v) takes every sample with this key
        if c * (100 * p_den) >= W * p_num:
            return b, W
    raise AssertionError("p <= 100: the largest sample satisfies the rule")


class Sorted:
    """One series sorted ONCE, for many (table, percentile) questions: the same rule as
    ``wquantile_one`` (tests/test_wquantile_host.py holds the two against each other).  The
    cumulative weights are uint64 sums below 2^63, so exact; C * D >= W * num for an integer C is
    C >= ceil(W * num / D), taken in Python integers."""

    def __init__(self, x):
        x = np.asarray(x, dtype=np.float64)
        self.L = x.size
        slots = np.flatnonzero(~np.isnan(x))
        u = x[slots].view(np.uint64)
        keys = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
        order = np.argsort(keys, kind="stable")
        self.bits, self.keys, self.ages = u[order], keys[order], (self.L - 1 - slots[order])
        last = np.ones(self.keys.size, dtype=bool)  # the last sample of each run of equal keys
        last[:-1] = self.keys[1:] != self.keys[:-1]
        self.ends = np.flatnonzero(last)

    def answer(self, table, p_num: int, p_den: int):
        """(answer's bits, W)."""
        table = np.asarray(table, dtype=np.uint64)
        cum = np.cumsum(table[np.minimum(self.ages, table.size - 1)], dtype=np.uint64)
        W = int(cum[-1]) if cum.size else 0
        if W == 0:
            return QNAN, 0
        need = -(-W * p_num // (100 * p_den))
        at = self.ends[int(np.searchsorted(cum[self.ends], np.uint64(need), side="left"))]
        return int(self.bits[at]), W


def np_wquantile(vals, offs, table, p_num: int, p_den: int, gaps=False) -> dict:
    """The whole entry point as numpy arrays [S]: value, wsum (uint64), count, flags."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs)
    S = offs.size - 1
    value, wsum = np.zeros(S, np.uint64), np.zeros(S, np.uint64)
    count, flags = np.zeros(S, np.int64), np.zeros(S, np.int32)
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        n = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        count[s] = n
        value[s] = QNAN
        if n == 0:
            flags[s] = EMPTY
        elif not gaps and np.isnan(x).any():
            flags[s] = NAN
        else:
            value[s], wsum[s] = wquantile_one(x, table, p_num, p_den)
    return dict(value=value.view(np.float64), wsum=wsum, count=count, flags=flags)

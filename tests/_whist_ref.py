"""krr_segmented_whist and krr_whist_query restated in plain Python integers, for the tests of the
kernels and of the layers above them.  Nothing here comes from the code under test; the bits, the
key order, the weights of a series and the exact weighted quantile are tests/_wquantile_ref.py's.

Bins (m = mantissa_bits, e_lo = min_exponent, nbins = octaves << m, width = nbins + 4), by the
VALUE of a sample, in exact rational arithmetic (fractions.Fraction of a float is exact):

    [0] x < 0 (-Inf included)   [1] x == 0 (either sign)   [2] 0 < x < 2^e_lo
    [3 + i] 2^E (1 + j / 2^m) <= x < 2^E (1 + (j + 1) / 2^m), E = e_lo + (i >> m), j = i & (2^m - 1)
    [3 + nbins] x >= 2^(e_lo + octaves), +Inf included

A series of L slots, a table of integer weights indexed by age and an age base B: slot i has age
B + L - 1 - i and weight table[min(age, len(table) - 1)].  The row is the summed weight of the
present samples per bin, W its sum, wmin / wmax the least / greatest present sample of positive
weight under the key order (the quiet NaN when W == 0).  A NaN sample in the compact layout:
KRR_FLAG_NAN, a row of zeros, W = 0, the quiet NaNs.

A percentile p = p_num / p_den reads the first bin b with C(b) * 100 * p_den >= W * p_num, C the
cumulative weight; its bracket is the bin's value range clamped to [wmin, wmax] by key order."""
from fractions import Fraction

import numpy as np

from _wquantile_ref import EMPTY, NAN, QNAN, bits, okey, weights_of, wquantile_one  # noqa: F401

SKETCH_RANGE = 8
NEG_ZERO = 1 << 63


def width_of(m: int, e_lo: int, octaves: int) -> int:
    return (octaves << m) + 4


def pow2(e: int) -> Fraction:
    return Fraction(2) ** e


def lower_edge(m: int, e_lo: int, i: int) -> Fraction:
    """The lower edge of log-linear bin i (i = nbins: where the top bin starts)."""
    return pow2(e_lo + (i >> m)) * (1 + Fraction(i & ((1 << m) - 1), 1 << m))


def bin_of(v: float, m: int, e_lo: int, octaves: int) -> int:
    """The bin of a non-NaN sample, from its VALUE."""
    if v == float("inf"):
        return 3 + (octaves << m)
    if v < 0:
        return 0
    if v == 0:
        return 1
    x = Fraction(v)
    if x < pow2(e_lo):
        return 2
    if x >= pow2(e_lo + octaves):
        return 3 + (octaves << m)
    E = e_lo
    while x >= pow2(E + 1):  # E = floor(log2 x)
        E += 1
    j = int((x / pow2(E) - 1) * (1 << m))  # floor: the quotient is >= 0
    return 3 + ((E - e_lo) << m) + j


def bins_of(x, geom) -> np.ndarray:
    """``bin_of`` over an array of non-NaN samples, still from their VALUES: frexp splits x into
    f * 2^e with 0.5 <= |f| < 1 exactly (subnormals included), and (2 |f| - 1) * 2^m is exact in
    float64, so its floor is j.  tests/test_whist_host.py holds it against the rational form."""
    m, e_lo, octaves = geom
    nb = octaves << m
    x = np.asarray(x, dtype=np.float64)
    f, e = np.frexp(np.where(np.isfinite(x), x, 1.0))
    E = e.astype(np.int64) - 1
    j = np.floor((2 * np.abs(f) - 1) * (1 << m)).astype(np.int64)
    b = np.where(E < e_lo, 2, np.where(E >= e_lo + octaves, 3 + nb, 3 + (E - e_lo) * (1 << m) + j))
    b = np.where(np.isinf(x), 3 + nb, b)
    b = np.where(x < 0, 0, b)
    return np.where(x == 0, 1, b).astype(np.int64)


def slot_weights(L: int, table, base: int = 0) -> np.ndarray:
    """uint64 [L]: ``weights_of`` for a slice of L slots that ``base`` slots follow."""
    table = np.asarray(table, dtype=np.uint64)
    return table[np.minimum(base + L - 1 - np.arange(L, dtype=np.int64), table.size - 1)]


def whist_one(x, table, geom, base: int = 0):
    """(row: uint64 [width], W, wmin bits, wmax bits) of one series whose NaN entries are absent.
    Every sum stays below 2^63, so the uint64 sums are the integers' own."""
    x = np.asarray(x, dtype=np.float64)
    w = slot_weights(x.size, table, base)
    here = ~np.isnan(x)
    x, w = x[here], w[here]
    row = np.zeros(width_of(*geom), np.uint64)
    np.add.at(row, bins_of(x, geom), w)
    W = int(w.sum(dtype=np.uint64))
    assert W == sum(int(v) for v in row) < 1 << 63
    if W == 0:
        return row, 0, QNAN, QNAN
    u = x[w > 0].view(np.uint64)
    keys = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    return row, W, int(u[np.argmin(keys)]), int(u[np.argmax(keys)])


def np_whist(vals, offs, table, geom, gaps=False, base=None) -> dict:
    """The whole entry point as numpy arrays: hist uint64 [S, width], wsum, wmin / wmax (bits, uint64),
    count, flags, [S] each."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs)
    S = offs.size - 1
    hist = np.zeros((S, width_of(*geom)), np.uint64)
    wsum, wmin, wmax = np.zeros(S, np.uint64), np.full(S, QNAN, np.uint64), np.full(S, QNAN, np.uint64)
    count, flags = np.zeros(S, np.int64), np.zeros(S, np.int32)
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        n = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        count[s] = n
        if n == 0:
            flags[s] = EMPTY
        elif not gaps and np.isnan(x).any():
            flags[s] = NAN
        else:
            row, W, mn, mx = whist_one(x, table, geom, 0 if base is None else int(base[s]))
            hist[s], wsum[s], wmin[s], wmax[s] = row, W, mn, mx
    return dict(hist=hist, wsum=wsum, wmin=wmin, wmax=wmax, count=count, flags=flags)


def answer_bin(row, p_num: int, p_den: int) -> int:
    """The first bin whose cumulative weight reaches p percent of the row's sum; -1 for a row of zeros."""
    W = sum(int(w) for w in row)
    if W == 0:
        return -1
    c = 0
    for b, w in enumerate(row):
        c += int(w)
        if c * (100 * p_den) >= W * p_num:
            return b
    raise AssertionError("p <= 100: the last bin satisfies the rule")


def _fbits(x: Fraction) -> int:
    f = float(x) if x < pow2(1024) else float("inf")
    assert f == float("inf") or Fraction(f) == x  # an edge is a float64 exactly
    return bits(f)


def bracket(row, wmin: int, wmax: int, geom, p_num: int, p_den: int):
    """(bin, lower bits, upper bits, flags) of krr_whist_query for one row."""
    m, e_lo, octaves = geom
    nb = octaves << m
    b = answer_bin(row, p_num, p_den)
    if b < 0:
        return -1, QNAN, QNAN, EMPTY

    def omax(u, v):
        return u if okey(u) >= okey(v) else v

    def omin(u, v):
        return u if okey(u) <= okey(v) else v

    if b == 1:
        return b, 0, 0, 0
    if b == 0:
        return b, wmin, omin(NEG_ZERO, wmax), SKETCH_RANGE
    if b == 2:
        return b, omax(0, wmin), omin(_fbits(pow2(e_lo)), wmax), SKETCH_RANGE
    if b == 3 + nb:
        return b, omax(_fbits(pow2(e_lo + octaves)), wmin), wmax, SKETCH_RANGE
    i = b - 3
    return b, omax(_fbits(lower_edge(m, e_lo, i)), wmin), omin(_fbits(lower_edge(m, e_lo, i + 1)), wmax), 0

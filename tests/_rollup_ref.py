"""krr_segmented_rollup restated in plain Python, for the tests of the kernel and of the layers
above it.  Nothing here comes from the code under test.

A segment of L slots is cut into nw = ceil(L / W) windows; slot i belongs to window (i + ph) // W
with ph = 0 ("start": the last window may be partial) or ph = (W - L % W) % W ("end": the first
may be).  Per window, P = its present slots (every slot, or the non-NaN slots when ``gaps``):

    count = |P|
    min / max = the extremal sample under float comparison, its own bits, a zero extremum as
                +0.0; NaN when P is empty
    exact = the sum of P as a Fraction (or the float +-inf / nan where infinite samples make the
            IEEE sum that), 0 when P is empty
    bound = (m-1) u / (1 - (m-1) u) * sum|x|, m = count, u = 2^-53: a plain float64 sum of m terms
            in any order is within gamma_{m-1} sum|x| of the exact one (Higham, Accuracy and
            Stability of Numerical Algorithms, section 4.2)

and a window that holds a NaN sample in the compact layout is NaN in min, max and sum with
count = its slots (``nan`` is set)."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
EMPTY, NAN, CAPACITY = 4, 1, 2
START, END = 0, 1
SCALE = 2 ** 1074  # every finite float64 is an integer multiple of 2^-1074
INF = float("inf")


def scaled(v: float) -> int:
    n, d = v.as_integer_ratio()  # exact; d is a power of two <= 2^1074
    return n * (SCALE // d)


def phase(L: int, W: int, align: int) -> int:
    return (W - L % W) % W if align == END else 0


def window_bounds(L: int, W: int, align: int) -> list:
    """[(lo, hi)]: window w holds slots lo .. hi - 1."""
    ph, nw = phase(L, W, align), -(-L // W)
    return [(max(0, w * W - ph), min(L, (w + 1) * W - ph)) for w in range(nw)]


def window_one(xs: list, gaps: bool) -> dict:
    """One window from the list of its slots (Python floats)."""
    present = [v for v in xs if v == v]
    if not gaps and len(present) != len(xs):
        return dict(count=len(xs), min=np.nan, max=np.nan, exact=np.nan, bound=Fraction(0), nan=True)
    lo = hi = None
    for v in present:
        if lo is None or v < lo:
            lo = v
        if hi is None or v > hi:
            hi = v
    if lo is None:
        lo = hi = np.nan
    else:
        lo = 0.0 if lo == 0 else lo
        hi = 0.0 if hi == 0 else hi
    infs = {v for v in present if v in (INF, -INF)}
    if infs:
        exact, bound = (np.nan if len(infs) == 2 else infs.pop()), Fraction(0)
    else:
        m = len(present)
        exact = Fraction(sum(scaled(v) for v in present), SCALE)
        mag = Fraction(sum(abs(scaled(v)) for v in present), SCALE)
        bound = Fraction(m - 1) * U / (1 - Fraction(m - 1) * U) * mag if m > 1 else Fraction(0)
    return dict(count=len(present), min=lo, max=hi, exact=exact, bound=bound, nan=False)


def rollup_one(x, W: int, align: int, gaps: bool) -> list:
    """The windows of one series, oldest first."""
    xs = np.asarray(x, dtype=np.float64).tolist()
    return [window_one(xs[lo:hi], gaps) for lo, hi in window_bounds(len(xs), W, align)]


def np_rollup(vals, offs, window: int, align: int, gaps: bool = False, win_offsets=None) -> dict:
    """The whole entry point as numpy arrays: ``offsets`` (the exclusive cumulative sum of nw, or
    the caller's), flat ``wcount`` / ``min`` / ``max`` / ``sum`` (the exact sum rounded once to
    float64), the per-window ``exact`` and ``bound`` lists (None where no window is written), and
    ``count`` / ``flags`` [S] by the flag rules of the header (CAPACITY: the caller's span is too
    small, no window of that segment is written)."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs, dtype=np.int64)
    S = offs.size - 1
    nw = -(-np.diff(offs) // window)
    if win_offsets is None:
        win_offsets = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
    win_offsets = np.asarray(win_offsets, dtype=np.int64)
    n = int(win_offsets.max()) if win_offsets.size else 0
    out = dict(offsets=win_offsets, wcount=np.zeros(n, np.uint32), min=np.full(n, np.nan), max=np.full(n, np.nan),
               sum=np.zeros(n), exact=[None] * n, bound=[None] * n, written=np.zeros(n, bool),
               count=np.zeros(S, np.int64), flags=np.zeros(S, np.uint32))
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        nans = int(np.count_nonzero(np.isnan(x)))
        cnt = x.size - nans if gaps else x.size
        out["count"][s] = cnt
        if cnt == 0:
            out["flags"][s] = EMPTY
        elif nans and not gaps:
            out["flags"][s] = NAN
        if win_offsets[s + 1] - win_offsets[s] < nw[s]:
            out["flags"][s] |= CAPACITY
            continue
        for w, e in enumerate(rollup_one(x, window, align, gaps)):
            i = int(win_offsets[s]) + w
            out["wcount"][i], out["min"][i], out["max"][i] = e["count"], e["min"], e["max"]
            out["sum"][i] = float(e["exact"])
            out["exact"][i], out["bound"][i], out["written"][i] = e["exact"], e["bound"], True
    return out


def brute_window_of(i: int, L: int, W: int, align: int) -> int:
    """The window of slot i, found by walking: "end" counts windows back from the last slot."""
    if align == START:
        return i // W
    return (-(-L // W) - 1) - (L - 1 - i) // W

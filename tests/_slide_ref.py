"""krr_segmented_slide restated in plain Python and numpy, for the tests of the kernel and of the
layers above it.  Nothing here comes from the code under test.

Slot i of a segment of L slots has the window of slots [max(0, i - W + 1), i].  P = the window's
present slots (every slot, or the non-NaN slots when ``gaps``), c = |P|, and the window is emitted
iff c >= min_count.  Per slot:

    wcount = c, always
    min / max = the extremal sample under float comparison, a zero extremum as +0.0
    exact  = the sum of P as an integer multiple of 2^-1074 (``exact[i]`` / SCALE), or the float
             +-inf / nan where infinite samples make the IEEE sum that
    mag    = sum |x| over P on the same scale
    mean   = exact / c, rounded once to float64

A window that is not emitted is NaN in min, max and mean and has ``exact[i] is None``; an emitted
window that holds a NaN sample in the compact layout is NaN in all of them (``exact[i]`` is nan).
The truth of a window's sum is a difference of EXACT prefix sums, so it costs O(L) per window size;
a plain float64 sum of c terms in any order is within gamma_{c-1} sum|x| of it, gamma_k =
k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):
``sum_within_bound`` compares in integers."""
from fractions import Fraction

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

EMPTY, NAN = 4, 1
SCALE = 2 ** 1074  # every finite float64 is an integer multiple of 2^-1074
INF = float("inf")


def scaled(v: float) -> int:
    n, d = v.as_integer_ratio()  # exact; d is a power of two <= 2^1074
    return n * (SCALE // d)


def _prefix(flags) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(flags, dtype=np.int64)])


def slide_one(x, W: int, gaps: bool, exact: bool = True) -> dict:
    """Every window of one series, before min_count is applied: ``wcount``, ``nans`` (NaN slots of
    the window), ``pinf`` / ``ninf`` (its infinite samples), ``min`` / ``max`` over the non-NaN
    slots (NaN without one), and the exact ``total`` / ``mag`` of its finite samples as ints."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    i = np.arange(L)
    lo = np.maximum(0, i - W + 1)
    isn = np.isnan(x)

    def windowed(flags):
        p = _prefix(flags)
        return p[i + 1] - p[lo]

    nans = windowed(isn)
    out = dict(nans=nans, wcount=(windowed(~isn) if gaps else (i + 1 - lo)).astype(np.uint32),
               pinf=windowed(x == INF), ninf=windowed(x == -INF))
    if exact:
        fin = np.isfinite(x)
        P, A = [0], [0]
        for v, f in zip(x.tolist(), fin.tolist()):
            t = scaled(v) if f else 0
            P.append(P[-1] + t)
            A.append(A[-1] + abs(t))
        out["total"] = [P[k + 1] - P[a] for k, a in enumerate(lo.tolist())]
        out["mag"] = [A[k + 1] - A[a] for k, a in enumerate(lo.tolist())]
    if L:
        We = min(W, L)
        pad = np.concatenate([np.full(We - 1, np.nan), x])
        view = sliding_window_view(pad, We)
        with np.errstate(all="ignore"):
            out["min"], out["max"] = np.fmin.reduce(view, axis=1), np.fmax.reduce(view, axis=1)
    else:
        out["min"] = out["max"] = np.empty(0)
    return out


def np_slide(values, offsets, window: int, min_count: int, gaps: bool = False, exact: bool = True,
             means: bool = False, cache: dict = None) -> dict:
    """The whole entry point as numpy arrays laid out by ``offsets``: ``wcount`` (uint32),
    ``emitted`` and ``poison`` (bool), ``min`` / ``max`` (float64), the lists ``exact`` and ``mag``
    (``exact=False`` leaves them None: counts and extrema only), ``mean`` and ``sum`` (with
    ``means``: the exact value rounded once, else NaN) and ``count`` / ``flags`` [S] by the flag rules of krr_segmented_stats.  ``cache``: a
    dict the caller keeps per (values, gaps, window), so that several min_count share the windows."""
    vals, offs = np.asarray(values, dtype=np.float64), np.asarray(offsets, dtype=np.int64)
    S, n = offs.size - 1, vals.size
    out = dict(wcount=np.zeros(n, np.uint32), min=np.full(n, np.nan), max=np.full(n, np.nan),
               mean=np.full(n, np.nan), sum=np.full(n, np.nan), emitted=np.zeros(n, bool), poison=np.zeros(n, bool),
               exact=[None] * n, mag=[None] * n, count=np.zeros(S, np.int64), flags=np.zeros(S, np.uint32))
    for s in range(S):
        a, b = int(offs[s]), int(offs[s + 1])
        x = vals[a:b]
        nn = int(np.count_nonzero(np.isnan(x)))
        cnt = x.size - nn if gaps else x.size
        out["count"][s] = cnt
        if cnt == 0:
            out["flags"][s] = EMPTY
        elif nn and not gaps:
            out["flags"][s] = NAN
        if a == b:
            continue
        if cache is not None and s in cache:
            w = cache[s]
        else:
            w = slide_one(x, window, gaps, exact)
            if cache is not None:
                cache[s] = w
        c = w["wcount"]
        em = c >= min_count
        poison = em & (w["nans"] > 0) & (not gaps)
        good = em & ~poison
        out["wcount"][a:b], out["emitted"][a:b], out["poison"][a:b] = c, em, poison
        for k in ("min", "max"):
            v = np.where(good, w[k], np.nan)
            out[k][a:b] = np.where(v == 0, 0.0, v)
        for i in np.flatnonzero(em).tolist() if exact else ():
            if poison[i] or (w["pinf"][i] and w["ninf"][i]):
                e = np.nan
            elif w["pinf"][i] or w["ninf"][i]:
                e = INF if w["pinf"][i] else -INF
            else:
                e = w["total"][i]
                if means:
                    out["mean"][a + i] = float(Fraction(e, SCALE * int(c[i])))
                    out["sum"][a + i] = float(Fraction(e, SCALE))
            if not isinstance(e, int):
                out["mean"][a + i] = out["sum"][a + i] = e
            out["exact"][a + i], out["mag"][a + i] = e, w["mag"][i]
    return out


def sum_within_bound(got: float, exact: int, mag: int, c: int) -> bool:
    """|got - exact| <= (c-1) u / (1 - (c-1) u) * mag with u = 2^-53, in integers on SCALE:
    |got - exact| (2^53 - (c-1)) <= (c-1) mag."""
    if got != got or got in (INF, -INF):
        return False
    return abs(scaled(got) - exact) * (2 ** 53 - (c - 1)) <= (c - 1) * mag


def brute_slide(x, W: int, min_count: int, gaps: bool) -> list:
    """The same by a double loop over Python floats and Fractions, for short series: one dict per
    slot with count, emitted, min, max, total (Fraction, nan or +-inf; None when not emitted)."""
    xs = np.asarray(x, dtype=np.float64).tolist()
    res = []
    for i in range(len(xs)):
        win = [xs[j] for j in range(max(0, i - W + 1), i + 1)]
        present = [v for v in win if v == v]
        c = len(present) if gaps else len(win)
        r = dict(count=c, emitted=c >= min_count, min=np.nan, max=np.nan, total=None)
        if r["emitted"]:
            if not gaps and len(present) != len(win):
                r["total"] = np.nan
            else:
                lo = hi = None
                for v in present:
                    lo = v if lo is None or v < lo else lo
                    hi = v if hi is None or v > hi else hi
                r["min"], r["max"] = (0.0 if lo == 0 else lo), (0.0 if hi == 0 else hi)
                infs = {v for v in present if v in (INF, -INF)}
                if infs:
                    r["total"] = np.nan if len(infs) == 2 else infs.pop()
                else:
                    r["total"] = sum((Fraction(v) for v in present), Fraction(0))
        res.append(r)
    return res


def np_peak(mean, emitted) -> tuple:
    """(peak, slot) of one series from its per-slot means by the header's rules: any emitted NaN
    mean gives (nan, its first slot); else the largest emitted mean (a zero as +0.0) and the first
    slot that compares equal; (nan, -1) without an emitted window."""
    best, at = np.nan, -1
    for i, (m, e) in enumerate(zip(np.asarray(mean, dtype=np.float64).tolist(), np.asarray(emitted).tolist())):
        if not e:
            continue
        if m != m:
            return np.nan, i
        if at < 0 or m > best:
            best, at = m, i
    return (0.0 if best == 0 else best), at

"""krr_segmented_exceed restated in plain Python, for the tests of the kernel and of the layers
above it.  Nothing here comes from the code under test.

A series is a float64 array whose NaN entries are ABSENT slots (the gapped layout; a compact
series without NaN samples is the same thing with nothing absent).  For a threshold tau:

    above   = #{present x : x > tau}            (the float comparison, strict)
    excess  = sum of (x - tau) over those, EXACT: a Fraction of the float64 inputs
    longest = the longest run of consecutive present samples that are all above
    head    = the run that starts at the first present sample (0 if it is not above)
    tail    = the run that ends at the last present sample
    last    = slot index of the last sample above, -1 if none

and ``bound`` = m u / (1 - m u) * excess with m = above and u = 2^-53, in rationals: every term
of the kernel's float64 sum is one rounded subtraction, the terms are non-negative, and a plain
sum of m such terms in any order is within gamma_m of the exact one (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2)."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
EMPTY, NAN = 4, 1
INT_FIELDS = ("above", "longest", "head", "tail", "last")
SCALE = 2 ** 1074  # every finite float64 is an integer multiple of 2^-1074


def _scaled(v: float) -> int:
    n, d = v.as_integer_ratio()  # exact; d is a power of two <= 2^1074
    return n * (SCALE // d)


def exceed_one(x, tau) -> dict:
    """One series, one threshold.  ``excess`` is a Fraction, or the float +inf / nan where the
    IEEE sum is not finite (an infinite sample above, tau = -inf)."""
    tau = float(tau)
    above = longest = head = run = 0
    last, seen, first_run_open = -1, 0, True
    total, special = 0, None  # total: the exact sum of the samples above, in units of 2^-1074
    for i, v in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        if v != v:  # absent: transparent
            continue
        seen += 1
        if v > tau:
            above += 1
            run += 1
            last = i
            longest = max(longest, run)
            if first_run_open:
                head = run
            if v == float("inf") or tau == float("-inf"):
                special = float("inf")
            else:
                total += _scaled(v)
        else:
            run = 0
            first_run_open = False
    m = above
    exact = Fraction(total - m * _scaled(tau), SCALE) if m and special is None else Fraction(0)
    bound = Fraction(m) * U / (1 - Fraction(m) * U) * exact
    return dict(count=seen, above=above, excess=exact if special is None else special, bound=bound,
                longest=longest, head=head, tail=run, last=last)


def np_exceed(vals, offs, thresholds, gaps=False) -> dict:
    """The whole entry point as numpy arrays: [R, S] outputs and [S] count / flags, ``excess``
    the exact sum rounded once to float64.  Flag rules as the header states them."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs)
    thr = np.asarray(thresholds, dtype=np.float64)
    R, S = thr.shape
    assert S == offs.size - 1
    out = {k: np.zeros((R, S), np.int64) for k in INT_FIELDS}
    out["last"][:] = -1
    out["excess"] = np.zeros((R, S), np.float64)
    out["count"], out["flags"] = np.zeros(S, np.int64), np.zeros(S, np.int32)
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        n = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        out["count"][s] = n
        if n == 0:
            out["flags"][s] = EMPTY
        elif not gaps and np.isnan(x).any():
            out["flags"][s] = NAN
            out["excess"][:, s] = np.nan
        else:
            for r in range(R):
                e = exceed_one(x, thr[r, s])
                for k in INT_FIELDS:
                    out[k][r, s] = e[k]
                out["excess"][r, s] = float(e["excess"])
    return out


def compacted(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return x[~np.isnan(x)]

"""Exact moments of a float64 series and the error bounds krr_segmented_moments is held to.

The yardstick is exact arithmetic on the float64 inputs: every sample is an integer over a power of
two (``float.as_integer_ratio``), so with one common denominator 2^K the sums  Sx = sum x,
Sxx = sum x^2, Si = sum i, Sii = sum i^2, Six = sum i x  over the present slots are Python
integers, and one rational division each gives

    MEAN = Sx / n       M2 = Sxx - Sx^2 / n       TMEAN = Si / n       T2 = Sii - Si^2 / n
    CXT = Six - Si Sx / n.

No floating-point two-pass stands in as truth.  The bounds (u = 2^-53, A = max |x|, L slots):

    mean   n u A
    tmean  n u (L - 1)
    m2     n u sqrt(Sxx M2) + n^2 u^2 Sxx
    t2     n u T2 + n^2 u^2 Sii
    cxt    n u sqrt(Sxx T2) + n^2 u^2 sqrt(Sxx Sii)

are Chan, Golub and LeVeque's first-order bound n kappa u for updating algorithms (kappa =
sqrt(Sxx / M2)) plus the two-pass second-order term; they are not measurements of any code.  They
are evaluated in rationals too, square roots rounded DOWN (math.isqrt), so the bound applied is
never wider than the formula."""
from fractions import Fraction
from math import isqrt

import numpy as np

U = Fraction(1, 2 ** 53)
FIELDS = ("mean", "m2", "tmean", "t2", "cxt")


def _sqrt_floor(q: Fraction) -> Fraction:
    """A rational <= sqrt(q), within 2^-64 relative for the magnitudes met here."""
    if q <= 0:
        return Fraction(0)
    p, d = q.numerator, q.denominator
    shift = max(0, 256 - (p * d).bit_length())
    shift += shift & 1
    return Fraction(isqrt((p * d) << shift), d << (shift // 2))


def exact_moments(slots: np.ndarray, first_slot: int = 0):
    """``slots``: the segment's L slots, NaN = absent.  Returns None without a present slot, else a
    dict of Fractions: n, L, the five moments, and A, Sxx, Sii for the bounds.  ``first_slot``
    shifts the slot index (the series continues an earlier one)."""
    slots = np.asarray(slots, dtype=np.float64)
    idx = np.nonzero(~np.isnan(slots))[0]
    n = int(idx.size)
    if n == 0:
        return None
    ratios = [float(v).as_integer_ratio() for v in slots[idx].tolist()]
    K = max(d.bit_length() - 1 for _, d in ratios)
    X = [p << (K - (d.bit_length() - 1)) for p, d in ratios]
    I = [int(i) + first_slot for i in idx.tolist()]
    Sx, Sxx = sum(X), sum(x * x for x in X)
    Si, Sii = sum(I), sum(i * i for i in I)
    Six = sum(i * x for i, x in zip(I, X))
    s = Fraction(1, 1 << K)
    return {"n": n, "L": int(slots.size), "mean": Fraction(Sx, n) * s, "m2": Fraction(n * Sxx - Sx * Sx, n) * s * s,
            "tmean": Fraction(Si, n), "t2": Fraction(n * Sii - Si * Si, n), "cxt": Fraction(n * Six - Si * Sx, n) * s,
            "A": max(abs(x) for x in X) * s, "Sxx": Sxx * s * s, "Sii": Fraction(Sii), "last": first_slot + int(slots.size) - 1}


def bounds(e: dict) -> dict:
    """The five bounds of the module docstring for exact_moments' result, as Fractions."""
    n, nu = e["n"], e["n"] * U
    return {"mean": nu * e["A"],
            "tmean": nu * e["last"],
            "m2": nu * _sqrt_floor(e["Sxx"] * e["m2"]) + nu * nu * e["Sxx"],
            "t2": nu * e["t2"] + nu * nu * e["Sii"],
            "cxt": nu * _sqrt_floor(e["Sxx"] * e["t2"]) + nu * nu * _sqrt_floor(e["Sxx"] * e["Sii"])}


def ratios(got: dict, e: dict) -> dict:
    """|got - exact| / bound per field (floats; 0 where both error and bound are 0, inf where only
    the bound is).  ``got``: field -> a finite float."""
    b = bounds(e)
    out = {}
    for k in FIELDS:
        if got.get(k) is None:
            continue
        err = abs(Fraction(float(got[k])) - e[k])
        out[k] = 0.0 if err == 0 else (float("inf") if b[k] == 0 else float(err / b[k]))
    return out


def rounded(e: dict) -> dict:
    """The exact moments rounded once to float64: what a stand-in for the kernel returns."""
    return {k: float(e[k]) for k in FIELDS}

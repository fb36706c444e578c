"""The host side of the fleet histogram (krr_amd.api.HistogramBins, default_bins, the ABI's
declarations) and the restatement itself (tests/_whist_ref.py), without a device.  The property the
whole feature rests on is checked here in integers: the bin that answers a percentile of the
histogram is the bin of the exact weighted percentile of the samples."""
import os
import re

import numpy as np
import pytest

from _whist_ref import (QNAN, SKETCH_RANGE, answer_bin, bin_of, bins_of, bits, bracket, lower_edge, okey, pow2,
                        slot_weights, weights_of, whist_one, width_of, wquantile_one)
from _wquantile_ref import fraction_of
from krr_amd.api import HistogramBins, default_bins  # noqa: F401  (the feature: absent, nothing here runs)
from krr_amd.core.models.allocations import ResourceType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = [(3, -2, 4), (0, -1022, 3), (4, -10, 20), (4, 20, 20), (10, 1020, 3), (2, 1020, 4), (0, 0, 1)]
INF = float("inf")


def _probe(geom) -> np.ndarray:
    """Every edge of the bins, the float one ulp below and above each, +-0, subnormals, negatives,
    the ends of the range and +-Inf."""
    m, e_lo, octaves = geom
    nb = octaves << m
    step = max(1, nb // 64)
    ids = sorted(set(range(0, nb + 1, step)) | {0, 1, nb - 1, nb})
    edges = np.array([float(lower_edge(m, e_lo, i)) if lower_edge(m, e_lo, i) < pow2(1024) else INF for i in ids])
    finite = edges[np.isfinite(edges)]
    extra = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, -1.0, -1e300, 1e300,
             1.7976931348623157e308, INF, -INF, 1.0, 0.1, 3e8]
    return np.concatenate([edges, np.nextafter(finite, 0.0), np.nextafter(finite, INF), extra])


@pytest.mark.parametrize("geom", GEOMS)
def test_bin_of_equals_the_rational_restatement(geom):
    b = HistogramBins(*geom)
    x = _probe(geom)
    want = np.array([bin_of(float(v), *geom) for v in x])
    assert np.array_equal(b.bin_of(x), want)
    assert np.array_equal(bins_of(x, geom), want)  # the vectorised restatement the GPU tests use
    rng = np.random.default_rng(geom[0] + 7)
    r = np.concatenate([rng.normal(0, 1, 300), rng.gamma(2.0, 0.05, 300), np.floor(rng.normal(2e8, 2e7, 300)),
                        np.ldexp(rng.random(300) + 1, rng.integers(-1074, 1023, 300))])
    want = np.array([bin_of(float(v), *geom) for v in r])
    assert np.array_equal(b.bin_of(r), want) and np.array_equal(bins_of(r, geom), want)
    assert b.bin_of(np.nan) == -1 and b.bin_of([[1.0, np.nan]]).shape == (1, 2)
    assert (np.diff(b.bin_of(np.sort(r))) >= 0).all()  # never decreases with the value


@pytest.mark.parametrize("geom", GEOMS)
def test_edges_are_exact(geom):
    m, e_lo, octaves = geom
    b = HistogramBins(*geom)
    e = b.edges()
    assert e.dtype == np.float64 and e.shape == (b.nbins + 1,) and b.width == width_of(*geom) == b.nbins + 4
    for i in sorted({0, 1, b.nbins // 2, b.nbins - 1, b.nbins}):
        want = lower_edge(m, e_lo, i)
        assert (e[i] == INF and want == pow2(1024)) or want == _frac(e[i]), i
    assert (np.diff(e) > 0).all()
    fin = e[np.isfinite(e)]
    assert np.array_equal(b.bin_of(fin), np.minimum(3 + np.arange(fin.size), 3 + b.nbins))  # an edge opens its bin
    assert np.array_equal(b.bin_of(np.nextafter(fin, 0.0)), 2 + np.arange(fin.size))          # the float below closes one
    assert (fin[1:] / fin[:-1] <= 1 + 2.0 ** -m).all()                                           # relative width


def _frac(v):
    from fractions import Fraction

    return Fraction(float(v))


@pytest.mark.parametrize("bad", [(-1, 0, 4), (11, 0, 4), (3, 0, 0), (3, -1023, 4), (3, 1020, 5), (10, 0, 4),
                                 (3.0, 0, 4), (True, 0, 4), ("3", 0, 4)])
def test_bad_bins_raise(bad):
    with pytest.raises(ValueError):
        HistogramBins(*bad)


def test_default_bins():
    cpu, mem = default_bins(ResourceType.CPU), default_bins(ResourceType.Memory)
    assert cpu == HistogramBins(4, -10, 20) and mem == HistogramBins(4, 20, 20) and default_bins("cpu") == cpu
    assert cpu.width == mem.width == 324
    assert cpu.edges()[0] == 2.0 ** -10 and cpu.edges()[-1] == 2.0 ** 10
    assert mem.edges()[0] == 2.0 ** 20 and mem.edges()[-1] == 2.0 ** 40
    assert (cpu.edges()[1:] / cpu.edges()[:-1]).max() == 1.0625
    p = cpu.params()
    assert (p.mantissa_bits, p.min_exponent, p.octaves) == (4, -10, 20)
    assert hash(cpu) == hash(HistogramBins(4, -10, 20))  # a cache key


def test_header_and_exports():
    from krr_amd import _native, api

    text = open(os.path.join(ROOT, "include", "krr_amd.h")).read()
    for name in ("krr_segmented_whist", "krr_whist_query"):
        assert re.search(r"^int " + name + r"\(krr_ctx\* ctx,", text, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    assert re.search(r"#define KRR_ABI_VERSION 3\b", text)
    for name in ("FleetHistogram", "HistogramBins", "default_bins"):
        assert name in api.__all__ and getattr(api, name) is getattr(api.batch, name)
    assert callable(_native.Context.segmented_whist) and callable(_native.Context.whist_query)
    assert callable(api.FleetBatch.histogram)


def test_slot_weights_equal_weights_of():
    table = [5, 0, 9, 2]
    for L in (0, 1, 3, 4, 9):
        assert slot_weights(L, table).tolist() == weights_of(L, table)
        for base in (1, 2, 7):
            assert slot_weights(L, table, base).tolist() == weights_of(L + base, table)[:L]


def _series(rng, n):
    kind = rng.integers(0, 5)
    if kind == 0:
        x = rng.normal(0, 1, n)
    elif kind == 1:
        x = rng.gamma(2.0, 0.5, n)
    elif kind == 2:
        x = rng.integers(-2, 3, n) * 0.5
        x[(x == 0) & (rng.random(n) < 0.5)] = -0.0
    elif kind == 3:
        x = np.ldexp(rng.random(n) + 1, rng.integers(-6, 6, n)) * rng.choice([-1, 1, 1, 1], n)
    else:
        x = rng.choice([0.25, 0.2499999999999999, 4.0, 3.9999999999999996, 1.0, 1e-3, INF, -INF, 0.0], n)
    if rng.random() < 0.5:
        x[rng.random(n) < 0.2] = np.nan
    return x


def test_answer_bin_is_the_bin_of_the_exact_weighted_percentile():
    """A few hundred random small series: the first bin whose cumulative weight reaches p percent
    holds the smallest sample whose cumulative weight does.  Then the bracket encloses that sample
    and, in a log-linear bin, ends within (1 + 2^-m) of it."""
    rng = np.random.default_rng(17)
    geom = (3, -2, 4)
    tables = [np.array([1], np.uint64), np.array([0, 9, 2], np.uint64), np.array([2 ** 32], np.uint64),
              (2 ** 32 >> (np.arange(40) // 3)).astype(np.uint64)]
    checked = empty = lumped = 0
    for _ in range(400):
        x = _series(rng, int(rng.integers(0, 60)))
        table = tables[int(rng.integers(0, len(tables)))]
        row, W, mn, mx = whist_one(x, table, geom)
        assert W == sum(w for v, w in zip(x.tolist(), weights_of(x.size, table)) if v == v)
        for p in ("0.000001", "50", "90", "95", "99.9", "100"):
            num, den = fraction_of(p)
            vb, W2 = wquantile_one(x, table, num, den)
            b, lo, hi, flags = bracket(row, mn, mx, geom, num, den)
            assert W2 == W and b == answer_bin(row, num, den)
            if W == 0:
                assert (b, lo, hi, vb) == (-1, QNAN, QNAN, QNAN)
                empty += 1
                continue
            v = np.array([vb], np.uint64).view(np.float64)[0]
            assert b == bin_of(float(v), *geom), (x, table, p)
            assert okey(lo) <= okey(vb) <= okey(hi) or (b == 1 and lo == hi == 0)
            assert (flags == SKETCH_RANGE) == (b in (0, 2, width_of(*geom) - 1))
            if 3 <= b < width_of(*geom) - 1:
                h = np.array([hi], np.uint64).view(np.float64)[0]
                assert h <= v * (1 + 2.0 ** -geom[0])
            else:
                lumped += 1
            if p == "100":
                assert hi == mx or b == 1
            checked += 1
    assert checked > 1200 and empty > 20 and lumped > 100


def test_slices_add_up_in_the_restatement():
    rng = np.random.default_rng(23)
    geom = (3, -2, 4)
    table = np.array([7, 0, 2 ** 32, 3, 0, 5], np.uint64)
    for _ in range(50):
        x = _series(rng, int(rng.integers(3, 40)))
        whole = whist_one(x, table, geom)
        for k in (1, x.size // 2, x.size - 1):
            old, new = whist_one(x[:k], table, geom, base=x.size - k), whist_one(x[k:], table, geom)
            assert np.array_equal(old[0] + new[0], whole[0]) and old[1] + new[1] == whole[1]


def test_bits_helper():
    assert bits(-0.0) == 1 << 63 and okey(bits(-0.0)) < okey(bits(0.0))

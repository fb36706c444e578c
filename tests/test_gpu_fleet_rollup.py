"""krr_amd.api.batch.FleetBatch.rollup on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) and a gapped fleet of a few
dozen small objects through the real engine against the plain restatement (tests/_rollup_ref.py:
counts and extrema exactly, the sum within (m-1) u / (1 - (m-1) u) sum|x| of the exact rational
sum), host-packed, chunked, resident in HBM and per pod; then what is built on the windows —
``as_batch`` with a percentile, ``peak``, ``fold``, ``dense``, the cache — and
examples/smoothed_strategy.py.

A window mean is float(sum) / count, one rounded division of a sum within its bound B of the exact
one: it lies within  tol = B / count + u |mean|  of the exact mean.  An order statistic and numpy's
linear interpolation between two of them move by at most the largest change of any element, so a
percentile (or the maximum) of the kernel's means lies within the largest tol of the object's
windows of the same percentile of the restatement's means, plus the interpolation's own rounding
(two operations: 2 u |value|)."""
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from _rollup_ref import END, START, U, np_rollup, rollup_one
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories
from test_fleet_rollup_host import _np_fold

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1
ALIGNS = {"start": START, "end": END}
nan = np.nan


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, r):
    return np.array([float(x) for samples in h[r].values() for x in samples])


def _hold(ru, series_list, gaps):
    """Every object's windows against the restatement; returns per object the restatement's means
    (NaN for an empty window) and the tolerance of each mean (see the module docstring)."""
    W, align = ru.window, ALIGNS[ru.align]
    assert ru.n_objects == len(series_list) and ru.offsets[0] == 0
    means, tols = [], []
    for s, x in enumerate(series_list):
        wins = rollup_one(x, W, align, gaps)
        present = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        assert ru.n_windows[s] == len(wins) == -(-x.size // W) and ru.slots[s] == x.size, s
        assert ru.count[s] == present and ru.flags[s] == (EMPTY if present == 0 else 0), s
        assert ru.of(s, "wcount").tolist() == [e["count"] for e in wins], s
        for k in ("min", "max"):
            want = np.array([e[k] for e in wins], dtype=np.float64)
            assert np.array_equal(ru.of(s, k).view(np.uint64), want.view(np.uint64)), (s, k)
        m, t = np.full(len(wins), nan), np.zeros(len(wins))
        for w, e in enumerate(wins):
            g = float(ru.of(s, "sum")[w])
            if e["count"] == 0:
                assert g == 0.0 and not np.signbit(g) and np.isnan(ru.of(s, "mean")[w]), (s, w)
                continue
            assert abs(Fraction(g) - e["exact"]) <= e["bound"], (s, w, g)
            exact_mean = e["exact"] / e["count"]
            m[w] = float(exact_mean)
            tol = e["bound"] / e["count"] + U * abs(exact_mean)
            t[w] = float(tol) * (1 + 2.0 ** -50)  # rounded up
            assert abs(Fraction(float(ru.of(s, "mean")[w])) - exact_mean) <= tol, (s, w)
        means.append(m)
        tols.append(t)
    return means, tols


def _resident(ps, dev):
    import torch

    from krr_amd.core.packing import PackedSeries

    return PackedSeries(torch.from_numpy(np.ascontiguousarray(ps.values, dtype=np.float64)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(ps.offsets, dtype=np.int64)).to(dev),
                        int(ps.max_len), ps.gaps_are_nan)


def _gapped_series(seed, S=36):
    """A NaN-gapped series of S segments of up to 400 slots (two empty, one all gaps, about 30%
    of the slots absent and a stretch of 40 absent slots in the long ones)."""
    from krr_amd.core.packing import PackedSeries

    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 401, S)
    lens[[2, 9]] = 0
    lens[[4, 7]] = [257, 384]
    segs = []
    for s, n in enumerate(lens.tolist()):
        x = rng.gamma(2.0, 0.05, n) if s % 2 else np.floor(rng.normal(2e8, 2e7, n))
        x[rng.random(n) < 0.3] = nan
        if n > 150:
            x[60:100] = nan
        segs.append(x)
    segs[5][:] = nan
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return PackedSeries(np.concatenate(segs), offs, int(lens.max()), True), segs


@pytest.mark.parametrize("align", list(ALIGNS))
def test_host_packed_fleet_whole_and_in_chunks(histories, align):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    batch = FleetBatch(histories, device=0)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    for r in (CPU, MEM):
        series = [_flat(h, r) for h in histories]
        for W in (1, 5, 7, 64):
            ru = batch.rollup(r, W, align)
            _hold(ru, series, gaps=False)
            assert len(list(eng._series_parts(small.series(r)))) >= 5
            c = small.rollup(r, W, align)  # chunks re-base the offsets: the sums' last bits may differ, the bound holds
            _hold(c, series, gaps=False)
            assert np.array_equal(c.offsets, ru.offsets)
            for k in ("wcount", "min", "max"):
                assert np.array_equal(getattr(c, k), getattr(ru, k), equal_nan=True), k


def test_per_pod_view(histories):
    from krr_amd.api import FleetBatch

    pods = FleetBatch(histories, device=0).per_pod(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    for align in ALIGNS:
        ru = pods.rollup(CPU, 5, align)
        assert ru.n_objects == len(kept) == pods.pod_groups[-1]
        _hold(ru, kept, gaps=False)


@pytest.mark.parametrize("align", list(ALIGNS))
def test_fleet_resident_in_hbm_and_what_is_built_on_the_windows(histories, align):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries, pack_resource

    dev = torch.device("cuda:0")
    host = FleetBatch(histories, device=0)
    fleet = PackedFleet(_resident(pack_resource(histories, CPU), dev), _resident(pack_resource(histories, MEM), dev))
    batch = FleetBatch.from_fleet(fleet, device=0)
    for r in (CPU, MEM):
        ru = batch.rollup(r, 5, align)
        _hold(ru, [_flat(h, r) for h in histories], gaps=False)
        want = host.rollup(r, 5, align)  # the same offsets: the same bits
        for k in ("wcount", "min", "max", "sum", "mean", "offsets", "count", "flags", "slots"):
            assert np.array_equal(getattr(ru, k), getattr(want, k), equal_nan=True), k
        assert ru.tensor("sum").is_cuda and ru.tensor("mean").is_cuda
    ps, segs = _gapped_series(41)
    gapped = FleetBatch.from_fleet(PackedFleet(_resident(ps, dev), _resident(ps, dev)), device=0)
    for W in (5, 60):
        ru = gapped.rollup(CPU, W, align)
        means, tols = _hold(ru, segs, gaps=True)
        assert (ru.wcount == 0).any() and (ru.wcount > 0).any()  # windows absent wholly occur
        # a percentile of smoothed usage: the kernel on the restatement's means, uploaded as a gapped series
        lens = [m.size for m in means]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ref_ps = PackedSeries(np.concatenate(means), offs, max(lens), True)
        ref = FleetBatch.from_fleet(PackedFleet(ref_ps, ref_ps), device=0)
        smooth = ru.as_batch("mean")
        assert ru.as_batch("mean") is smooth and smooth.series(CPU).values.is_cuda
        for p, mode in (("95", "linear"), ("50", "linear"), ("99", "sorted_lower")):
            got, gf = smooth.percentile(CPU, p, mode=mode, return_flags=True)
            want, wf = ref.percentile(CPU, p, mode=mode, return_flags=True)
            assert np.array_equal(gf, wf) and np.array_equal(smooth.counts(CPU, p, mode), ref.counts(CPU, p, mode))
            for s in range(len(segs)):
                if np.isnan(want[s]):
                    assert np.isnan(got[s]) and gf[s] == EMPTY, s
                else:
                    assert abs(got[s] - want[s]) <= tols[s].max() + 2 * 2.0 ** -53 * abs(want[s]), (s, p, mode)
        # the sustained peak: the largest window mean; of the window maxima it is the series' maximum itself
        peak = ru.peak()
        top = ru.peak("max")
        for s, x in enumerate(segs):
            if np.isnan(means[s]).all():
                assert np.isnan(peak[s]) and np.isnan(top[s])
            else:
                assert abs(peak[s] - np.nanmax(means[s])) <= tols[s].max(), s
                assert top[s] == np.nanmax(x) and peak[s] == np.nanmax(ru.of(s, "mean"))
        assert np.array_equal(peak, smooth.stats(CPU).max, equal_nan=True)
        # a further rollup of the window means: 12 windows of 5 slots per window
        again = smooth.rollup(CPU, 12, align)
        assert again.n_windows.tolist() == [-(-int(n) // 12) for n in ru.n_windows]
        # fold: the device's result against loops over the flat arrays
        for period in (1, 4, 24):
            prof = ru.fold(period)
            cnt, mn, mx, sm = _np_fold(ru, period)
            assert np.array_equal(prof.count, cnt) and np.array_equal(prof.sum, sm)
            assert np.array_equal(prof.min, mn, equal_nan=True) and np.array_equal(prof.max, mx, equal_nan=True)
            assert prof.count.sum(axis=1).tolist() == ru.count.tolist()
        # dense: justified by the alignment
        d = ru.dense("max")
        assert d.shape == (len(segs), int(ru.n_windows.max()))
        for s in range(len(segs)):
            nw = int(ru.n_windows[s])
            row, pad = (d[s, d.shape[1] - nw:], d[s, :d.shape[1] - nw]) if align == "end" else (d[s, :nw], d[s, nw:])
            assert np.array_equal(row, ru.of(s, "max"), equal_nan=True) and np.isnan(pad).all(), s


def test_second_call_does_not_launch(histories, monkeypatch):
    from krr_amd import _native
    from krr_amd.api import FleetBatch

    calls = []
    real = _native.Context.segmented_rollup
    monkeypatch.setattr(_native.Context, "segmented_rollup",
                        lambda self, series, window, align, *a, **k: (calls.append((series.n_segments, window, align)),
                                                                      real(self, series, window, align, *a, **k))[1])
    batch = FleetBatch(histories, device=0)
    ru = batch.rollup(CPU, 5)
    assert calls == [(N, 5, END)]  # "end" is the default
    assert batch.rollup(CPU, 5) is ru and batch.rollup(CPU, 5, "end") is ru and calls == [(N, 5, END)]
    batch.rollup(CPU, 5, "start")
    batch.rollup(MEM, 5)
    assert calls == [(N, 5, END), (N, 5, START), (N, 5, END)]


def test_as_batch_refuses_a_nan_sample():
    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries

    vals = np.array([1.0, 2.0, nan, 4.0, 5.0, 6.0, 7.0])
    ps = PackedSeries(vals, np.array([0, 4, 7]), 4, False)  # compact layout: the NaN is a sample
    ru = FleetBatch.from_fleet(PackedFleet(ps, ps), device=0).rollup(CPU, 2, "start")
    assert ru.flags.tolist() == [NAN, 0] and ru.wcount.tolist() == [2, 2, 2, 1]
    assert np.array_equal(ru.sum, [3.0, nan, 11.0, 7.0], equal_nan=True)
    assert np.array_equal(ru.max, [2.0, nan, 6.0, 7.0], equal_nan=True)
    with pytest.raises(ValueError, match="NaN"):
        ru.as_batch("mean")
    with pytest.raises(ValueError, match="NaN"):
        ru.peak()


def test_smoothed_strategy_equals_a_numpy_computation_per_object(histories):
    """The example's requests against numpy per object: the CPU request and limit within the
    tolerance of the window means (module docstring), memory exactly."""
    import decimal

    from examples.smoothed_strategy import SmoothedSettings, SmoothedStrategy
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import reference_context
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.utils.prom_decimal import prom_decimal

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    strategy = SmoothedStrategy(SmoothedSettings(window_slots=5, cpu_percentile=Decimal(95),
                                                 memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    raw = strategy.run_batch(histories, objects)
    assert len(raw) == N == len(BatchedRunner(strategy).recommend(objects, histories))
    for o, h in enumerate(histories):
        x, m = _flat(h, CPU), _flat(h, MEM)
        if x.size == 0:
            assert o in (3, 11)
            assert raw[o][CPU].request.is_nan() and raw[o][CPU].limit.is_nan() and raw[o][MEM].request.is_nan()
            continue
        wins = rollup_one(x, 5, END, False)
        means = np.array([float(e["exact"] / e["count"]) for e in wins])
        tol = max(float(e["bound"] / e["count"] + U * abs(e["exact"] / e["count"])) for e in wins) * (1 + 2.0 ** -50)
        want = float(np.percentile(means, 95))
        assert abs(float(raw[o][CPU].request) - want) <= tol + 2 * 2.0 ** -53 * abs(want), o
        assert abs(float(raw[o][CPU].limit) - means.max()) <= tol, o
        with decimal.localcontext(reference_context()):
            mem = prom_decimal(float(m.max())) * (1 + Decimal(10) / 100)
        assert raw[o][MEM].request == mem == raw[o][MEM].limit, o

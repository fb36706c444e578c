"""krr_amd.api.batch.FleetBatch.sliding / sustained_peak on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) and a gapped fleet of a few
dozen small objects through the real engine against the plain restatement (tests/_slide_ref.py:
counts and extrema exactly, the sum within (c-1) u / (1 - (c-1) u) sum|x| of the exact sum, the
mean one division of the kernel's sum), host-packed, chunked, resident in HBM and per pod; then
what is built on the windows — ``as_batch`` with a percentile, the peak, ``dense``, the cache — the
burst that a rollup's grid splits, and examples/burst_strategy.py.

A sliding mean is float(sum) / count, one rounded division of a sum within its bound B of the exact
one: it lies within  tol = B / count + u |mean|  of the exact mean.  An order statistic and numpy's
linear interpolation between two of them move by at most the largest change of any element, so a
percentile (or the maximum) of the kernel's means lies within the largest tol of the object's
windows of the same percentile of the restatement's means, plus the interpolation's own rounding
(two operations: 2 u |value|).  Where the samples are integers below 2^53 / window every sum is
exact and the means are the restatement's bit for bit."""
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from _slide_ref import SCALE, np_peak, np_slide, sum_within_bound
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories
from test_gpu_fleet_rollup import _flat, _gapped_series, _resident

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1
ALL = ("mean", "sum", "max", "min", "wcount")
U = Fraction(1, 2 ** 53)
nan = np.nan


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _hold(sl, series_list, gaps):
    """Every object's windows against the restatement; returns per object the restatement's means
    (NaN where no window is emitted) and the tolerance of each mean (see the module docstring)."""
    W, mc = sl.window, sl.min_count
    assert sl.n_objects == len(series_list) and sl.offsets[0] == 0
    means, tols = [], []
    for s, x in enumerate(series_list):
        r = np_slide(x, np.array([0, x.size]), W, mc, gaps, means=True)
        present = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        assert sl.slots[s] == x.size and sl.offsets[s + 1] - sl.offsets[s] == x.size, s
        assert sl.count[s] == present and sl.flags[s] == (EMPTY if present == 0 else 0), s
        assert np.array_equal(sl.of(s, "wcount").view(np.uint32), r["wcount"]), s
        for k in ("min", "max"):
            assert np.array_equal(_u64(sl.of(s, k)), _u64(np.where(np.isnan(r[k]), nan, r[k]))), (s, k)
        t = np.zeros(x.size)
        gs, gm = sl.of(s, "sum"), sl.of(s, "mean")
        for i in range(x.size):
            if not r["emitted"][i]:
                assert np.isnan(gs[i]) and np.isnan(gm[i]), (s, i)
                continue
            c, e = int(r["wcount"][i]), r["exact"][i]
            assert sum_within_bound(float(gs[i]), e, r["mag"][i], c), (s, i)
            assert gm[i] == gs[i] / c, (s, i)
            bound = Fraction(c - 1) * U / (1 - Fraction(c - 1) * U) * Fraction(r["mag"][i], SCALE)
            tol = bound / c + U * abs(Fraction(e, SCALE * c))
            t[i] = float(tol) * (1 + 2.0 ** -50)  # rounded up
            assert abs(Fraction(float(gm[i])) - Fraction(e, SCALE * c)) <= tol, (s, i)
        pk, at = np_peak(gm, r["emitted"])  # the header's rule on the kernel's own means
        assert np.array_equal(sl.peak[s], pk, equal_nan=True) and sl.peak_slot[s] == at, s
        means.append(r["mean"])
        tols.append(t)
    return means, tols


def test_host_packed_fleet_whole_and_in_chunks(histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    batch = FleetBatch(histories, device=0)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    for r in (CPU, MEM):
        series = [_flat(h, r) for h in histories]
        for W, mc in ((1, None), (5, None), (5, 1), (7, 4), (64, 1)):
            sl = batch.sliding(r, W, mc, stats=ALL)
            assert sl.min_count == (W if mc is None else mc)
            _hold(sl, series, gaps=False)
            assert len(list(eng._series_parts(small.series(r)))) >= 5
            c = small.sliding(r, W, mc, stats=ALL)  # chunks re-base the offsets: the sums' last bits may differ
            _hold(c, series, gaps=False)
            assert np.array_equal(c.offsets, sl.offsets)
            for k in ("wcount", "min", "max"):
                assert np.array_equal(c._flat(k), sl._flat(k), equal_nan=True), k
            pk, at = batch.sustained_peak(r, W, mc, return_slot=True)
            assert np.array_equal(_u64(pk), _u64(sl.peak)) and np.array_equal(at, sl.peak_slot)


def test_per_pod_view(histories):
    from krr_amd.api import FleetBatch

    pods = FleetBatch(histories, device=0).per_pod(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    sl = pods.sliding(CPU, 5, 3, stats=ALL)
    assert sl.n_objects == len(kept) == pods.pod_groups[-1]
    _hold(sl, kept, gaps=False)
    assert np.array_equal(_u64(pods.sustained_peak(CPU, 5, 3)), _u64(sl.peak))


def test_fleet_resident_in_hbm_and_what_is_built_on_the_windows(histories):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries, pack_resource

    dev = torch.device("cuda:0")
    host = FleetBatch(histories, device=0)
    fleet = PackedFleet(_resident(pack_resource(histories, CPU), dev), _resident(pack_resource(histories, MEM), dev))
    batch = FleetBatch.from_fleet(fleet, device=0)
    for r in (CPU, MEM):
        sl = batch.sliding(r, 5, 2, stats=ALL)
        means, _ = _hold(sl, [_flat(h, r) for h in histories], gaps=False)
        want = host.sliding(r, 5, 2, stats=ALL)  # the same offsets: the same bits
        for k in ALL:
            assert np.array_equal(sl._flat(k), want._flat(k), equal_nan=True), k
        for k in ("offsets", "count", "flags", "slots", "peak_slot"):
            assert np.array_equal(getattr(sl, k), getattr(want, k)), k
        assert np.array_equal(_u64(sl.peak), _u64(want.peak)) and sl.tensor("mean").is_cuda
        if r == MEM:  # integer samples: every sum is exact, the means are the restatement's
            assert np.array_equal(_u64(sl._flat("mean")), _u64(np.concatenate(means)))
    mean_only = batch.sliding(CPU, 5, 2)
    assert mean_only.stats == ("mean",)
    assert np.array_equal(_u64(mean_only._flat("mean")), _u64(batch.sliding(CPU, 5, 2, stats=ALL)._flat("mean")))
    with pytest.raises(ValueError, match="stats="):
        mean_only.tensor("max")
    ps, segs = _gapped_series(43)
    gapped = FleetBatch.from_fleet(PackedFleet(_resident(ps, dev), _resident(ps, dev)), device=0)
    for W, mc in ((5, 3), (60, 20)):
        sl = gapped.sliding(CPU, W, mc, stats=ALL)
        means, tols = _hold(sl, segs, gaps=True)
        emitted = ~np.isnan(sl._flat("mean"))
        assert emitted.any() and (~emitted).any() and (sl._flat("wcount") == 0).any()
        # a percentile of the sliding means: the kernel on the restatement's means, uploaded as a gapped series
        ref_ps = PackedSeries(np.concatenate(means), ps.offsets, ps.max_len, True)
        ref = FleetBatch.from_fleet(PackedFleet(ref_ps, ref_ps), device=0)
        smooth = sl.as_batch("mean")
        assert sl.as_batch("mean") is smooth and smooth.series(CPU).values.is_cuda
        for p, mode in (("95", "linear"), ("50", "linear"), ("99", "sorted_lower")):
            got, gf = smooth.percentile(CPU, p, mode=mode, return_flags=True)
            want, wf = ref.percentile(CPU, p, mode=mode, return_flags=True)
            assert np.array_equal(gf, wf) and np.array_equal(smooth.counts(CPU, p, mode), ref.counts(CPU, p, mode))
            for s in range(len(segs)):
                if np.isnan(want[s]):
                    assert np.isnan(got[s]) and gf[s] == EMPTY, s
                elif s % 2 == 0:  # integer samples: the same series bit for bit
                    assert got[s] == want[s], (s, p, mode)
                else:
                    assert abs(got[s] - want[s]) <= tols[s].max() + 2 * 2.0 ** -53 * abs(want[s]), (s, p, mode)
        # the sustained peak: the largest sliding mean, also as the maximum of the means' series
        peak = gapped.sustained_peak(CPU, W, mc)
        assert np.array_equal(_u64(peak), _u64(sl.peak))
        assert np.array_equal(peak, smooth.stats(CPU).max, equal_nan=True)
        for s in range(len(segs)):
            if np.isnan(means[s]).all():
                assert np.isnan(peak[s]) and sl.peak_slot[s] == -1
            else:
                assert abs(peak[s] - np.nanmax(means[s])) <= tols[s].max(), s
        # the other stats are series too; a rollup applies to them
        assert sl.as_batch("max").rollup(CPU, 12).n_windows.tolist() == [-(-x.size // 12) for x in segs]
        # dense: right-justified
        d = sl.dense("max")
        assert d.shape == (len(segs), max(x.size for x in segs))
        for s, x in enumerate(segs):
            assert np.array_equal(d[s, d.shape[1] - x.size:], sl.of(s, "max"), equal_nan=True)
            assert np.isnan(d[s, :d.shape[1] - x.size]).all(), s


def test_a_burst_that_straddles_the_rollup_grid():
    """The reason the feature exists: five slots at 0.9 over a floor of 0.1 that lie across a
    boundary of the 5-slot grid.  The sustained peak finds the whole burst, the rollup's peak on
    either grid reports less."""
    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries

    segs = []
    for L, at in ((41, 13), (1500, 1022), (1500, 1278), (37, 29)):
        x = np.full(L, 0.125)
        x[at:at + 5] = 0.875
        segs.append(x)
    offs = np.concatenate([[0], np.cumsum([x.size for x in segs])]).astype(np.int64)
    ps = PackedSeries(np.concatenate(segs), offs, 1500, False)
    batch = FleetBatch.from_fleet(PackedFleet(ps, ps), device=0)
    peak, at = batch.sustained_peak(CPU, 5, return_slot=True)
    assert peak.tolist() == [0.875] * 4 and at.tolist() == [17, 1026, 1282, 33]
    for align in ("start", "end"):
        grid = batch.rollup(CPU, 5, align).peak()
        assert (grid < 0.875).all() and (grid >= 0.5).all(), align  # the larger part of the burst at best
    assert batch.rollup(CPU, 5, "start").peak()[0] == (3 * 0.875 + 2 * 0.125) / 5
    assert (offs[1:-1] % 2 == 1).all()  # odd start offsets too


def test_second_call_does_not_launch(histories, monkeypatch):
    from krr_amd import _native
    from krr_amd.api import FleetBatch

    calls = []
    real = _native.Context.segmented_slide
    monkeypatch.setattr(_native.Context, "segmented_slide",
                        lambda self, series, window, minc, *a, **k: (calls.append((series.n_segments, window, minc)),
                                                                     real(self, series, window, minc, *a, **k))[1])
    batch = FleetBatch(histories, device=0)
    sl = batch.sliding(CPU, 5)
    assert calls == [(N, 5, 5)]  # min_count=None is the window
    assert batch.sliding(CPU, 5) is sl and batch.sliding(CPU, 5, 5, ("mean",)) is sl and calls == [(N, 5, 5)]
    batch.sustained_peak(CPU, 5)
    batch.sustained_peak(CPU, 5, return_slot=True)
    batch.sliding(MEM, 5, 1)
    assert calls == [(N, 5, 5), (N, 5, 5), (N, 5, 1)]


def test_as_batch_refuses_a_nan_sample():
    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries

    vals = np.array([1.0, 2.0, nan, 4.0, 5.0, 6.0, 7.0])
    ps = PackedSeries(vals, np.array([0, 4, 7]), 4, False)  # compact layout: the NaN is a sample
    sl = FleetBatch.from_fleet(PackedFleet(ps, ps), device=0).sliding(CPU, 2, 1, stats=ALL)
    assert sl.flags.tolist() == [NAN, 0] and sl._flat("wcount").tolist() == [1, 2, 2, 2, 1, 2, 2]
    assert np.array_equal(sl._flat("sum"), [1.0, 3.0, nan, nan, 5.0, 11.0, 13.0], equal_nan=True)
    assert np.array_equal(sl._flat("max"), [1.0, 2.0, nan, nan, 5.0, 6.0, 7.0], equal_nan=True)
    assert np.isnan(sl.peak[0]) and sl.peak_slot.tolist() == [2, 2] and sl.peak[1] == 6.5
    with pytest.raises(ValueError, match="NaN"):
        sl.as_batch("mean")


def test_burst_strategy_equals_a_numpy_computation_per_object(histories):
    """The example's requests against numpy per pod: the CPU request and limit within the
    tolerance of the sliding means (module docstring), memory exactly."""
    import decimal

    from examples.burst_strategy import BurstSettings, BurstStrategy
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import reference_context
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.utils.prom_decimal import prom_decimal

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    strategy = BurstStrategy(BurstSettings(window_slots=5, cpu_percentile=Decimal(95),
                                           memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    raw = strategy.run_batch(histories, objects)
    assert len(raw) == N == len(BatchedRunner(strategy).recommend(objects, histories))
    sized = 0
    for o, h in enumerate(histories):
        m = _flat(h, MEM)
        reqs, lims, tol = [], [], 0.0
        for samples in h[CPU].values():
            x = np.array([float(v) for v in samples])
            if x.size < 5:
                continue  # no full window
            r = np_slide(x, np.array([0, x.size]), 5, 5, False, means=True)
            means = r["mean"][4:]
            for i in range(4, x.size):
                bound = 4 * U / (1 - 4 * U) * Fraction(r["mag"][i], SCALE)
                tol = max(tol, float(bound / 5 + U * abs(Fraction(r["exact"][i], SCALE * 5))) * (1 + 2.0 ** -50))
            reqs.append(float(np.percentile(means, 95)))
            lims.append(means.max())
        if not reqs:
            assert raw[o][CPU].request.is_nan() and raw[o][CPU].limit.is_nan(), o
        else:
            sized += 1
            assert abs(float(raw[o][CPU].request) - max(reqs)) <= tol + 2 * 2.0 ** -53 * max(reqs), o
            assert abs(float(raw[o][CPU].limit) - max(lims)) <= tol, o
        if m.size == 0:
            assert o in (3, 11) and raw[o][MEM].request.is_nan()
            continue
        with decimal.localcontext(reference_context()):
            mem = prom_decimal(float(m.max())) * (1 + Decimal(10) / 100)
        assert raw[o][MEM].request == mem == raw[o][MEM].limit, o
    assert sized >= 10

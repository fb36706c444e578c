"""krr_amd.api.batch.FleetBatch.exceedance on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) through the real engine
against the plain restatement (tests/_exceed_ref.py: integers exactly, the excess within
m u / (1 - m u) E of the exact rational sum), host-packed, chunked, in groups of four thresholds and
resident in HBM; two halves ``concat``-ed against the whole; then examples/sustained_strategy.py
through the BatchedRunner."""
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from _exceed_ref import INT_FIELDS, exceed_one
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY = 4
nan = np.nan


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, r):
    return np.array([float(x) for samples in h[r].values() for x in samples])


def _hold(ex, series_list, thr, extra_bound=None):
    """Every series and row: integers equal the restatement's, excess within its bound (plus
    ``extra_bound[r][s]``, a Fraction, where given); EMPTY where there is no sample."""
    assert ex.count.size == len(series_list) and ex.above.shape == thr.shape
    assert np.array_equal(ex.thresholds, thr, equal_nan=True)
    for s, x in enumerate(series_list):
        present = int(np.count_nonzero(~np.isnan(x)))
        assert ex.count[s] == present and ex.slots[s] == x.size, s
        assert ex.flags[s] == (EMPTY if present == 0 else 0), s
        for r in range(thr.shape[0]):
            e = exceed_one(x, thr[r, s])
            assert [int(getattr(ex, k)[r, s]) for k in INT_FIELDS] == [e[k] for k in INT_FIELDS], (s, r)
            g = float(ex.excess[r, s])
            if e["above"] == 0:
                assert g == 0.0 and not np.signbit(g), (s, r)
            elif isinstance(e["excess"], Fraction):
                bound = e["bound"] if extra_bound is None else extra_bound[r][s]
                assert abs(Fraction(g) - e["excess"]) <= bound, (s, r, g)
            else:
                assert g == e["excess"], (s, r)


def _thresholds(histories, r, rows):
    """[rows, N]: per object, quantiles of its own samples (ties with samples occur), NaN for
    objects without samples, and a last row below everything."""
    thr = np.full((rows, N), nan)
    for o, h in enumerate(histories):
        x = np.sort(_flat(h, r))
        if x.size:
            for j in range(rows - 1):
                thr[j, o] = x[int((x.size - 1) * (0.3 + 0.69 * j / max(rows - 2, 1)))]
            thr[rows - 1, o] = x[0] - 1.0
    return thr


def test_host_packed_fleet_in_groups_and_chunks(histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    batch = FleetBatch(histories, device=0)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    for r in (CPU, MEM):
        series = [_flat(h, r) for h in histories]
        thr = _thresholds(histories, r, 6)  # two groups: four rows and two
        ex = batch.exceedance(r, thr)
        _hold(ex, series, thr)
        assert batch.exceedance(r, thr.copy()) is ex
        one = batch.exceedance(r, thr[4])  # a single row equals its row of the grouped result, bit for bit
        for k in INT_FIELDS + ("excess",):
            assert np.array_equal(getattr(one, k)[0].view(np.uint64), getattr(ex, k)[4].view(np.uint64)), k
        assert len(list(eng._series_parts(small.series(r)))) >= 5
        c = small.exceedance(r, thr)  # chunks re-base the offsets: the sums' last bits may differ, the bound holds
        _hold(c, series, thr)
        assert np.array_equal(c.count, ex.count) and np.array_equal(c.flags, ex.flags)
    pods = batch.per_pod(CPU)
    kept = [(o, np.array([float(v) for v in x])) for o, h in enumerate(histories) for x in h[CPU].values() if len(x)]
    thr = np.repeat(_thresholds(histories, CPU, 2), np.diff(pods.pod_groups), axis=1)
    assert thr.shape == (2, len(kept))
    _hold(pods.exceedance(CPU, thr), [x for _, x in kept], thr)


def _resident(ps, dev):
    import torch

    from krr_amd.core.packing import PackedSeries

    return PackedSeries(torch.from_numpy(np.ascontiguousarray(ps.values, dtype=np.float64)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(ps.offsets, dtype=np.int64)).to(dev),
                        int(ps.max_len), ps.gaps_are_nan)


def _gapped_series(seed, S=14):
    """A NaN-gapped series of S segments of up to 3,000 slots (two empty, one all gaps)."""
    from krr_amd.core.packing import PackedSeries

    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 3001, S)
    lens[[2, 9]] = 0
    segs = []
    for s, n in enumerate(lens.tolist()):
        x = rng.gamma(2.0, 0.05, n) if s % 2 else np.floor(rng.normal(2e8, 2e7, n))
        x[rng.random(n) < 0.2] = nan
        segs.append(x)
    segs[5][:] = nan
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return PackedSeries(np.concatenate(segs), offs, int(lens.max()), True), segs


def _own_thresholds(segs, qs=(0.5, 0.9, 0.99)):
    thr = np.full((len(qs), len(segs)), nan)
    for s, x in enumerate(segs):
        p = np.sort(x[~np.isnan(x)])
        if p.size:
            thr[:, s] = [p[int((p.size - 1) * q)] for q in qs]
    return thr


def test_fleet_resident_in_hbm(histories):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, pack_resource

    dev = torch.device("cuda:0")
    host = FleetBatch(histories, device=0)
    fleet = PackedFleet(_resident(pack_resource(histories, CPU), dev), _resident(pack_resource(histories, MEM), dev))
    batch = FleetBatch.from_fleet(fleet, device=0)
    for r in (CPU, MEM):
        thr = _thresholds(histories, r, 3)
        ex = batch.exceedance(r, thr)
        _hold(ex, [_flat(h, r) for h in histories], thr)
        want = host.exceedance(r, thr)  # the same offsets: the same bits
        for k in INT_FIELDS + ("excess", "count", "flags", "slots"):
            assert np.array_equal(getattr(ex, k), getattr(want, k)), k
    ps, segs = _gapped_series(41)
    gapped = FleetBatch.from_fleet(PackedFleet(_resident(ps, dev), _resident(ps, dev)), device=0)
    thr = _own_thresholds(segs)
    _hold(gapped.exceedance(MEM, thr), segs, thr)


def test_two_halves_concat_to_the_whole():
    """Each series cut at a position of its own (inside runs, at gaps, at 0 and at the end), the
    halves run separately on the device and merged on the host: the integers are the whole
    series', the excess within the two halves' summed bounds."""
    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries

    ps, segs = _gapped_series(43)
    rng = np.random.default_rng(44)
    cuts = [int(rng.integers(0, x.size + 1)) for x in segs]
    cuts[0], cuts[1] = 0, segs[1].size
    thr = _own_thresholds(segs)

    def batch_of(parts):
        lens = [p.size for p in parts]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        s = PackedSeries(np.concatenate(parts), offs, max(max(lens), 1), True)
        return FleetBatch.from_fleet(PackedFleet(s, s), device=0)

    first = batch_of([x[:k] for x, k in zip(segs, cuts)]).exceedance(CPU, thr)
    second = batch_of([x[k:] for x, k in zip(segs, cuts)]).exceedance(CPU, thr)
    _hold(first, [x[:k] for x, k in zip(segs, cuts)], thr)
    merged = first.concat(second)
    summed = [[exceed_one(x[:k], thr[r, s])["bound"] + exceed_one(x[k:], thr[r, s])["bound"]
               for s, (x, k) in enumerate(zip(segs, cuts))] for r in range(thr.shape[0])]
    _hold(merged, segs, thr, extra_bound=summed)
    whole = batch_of(segs).exceedance(CPU, thr)
    for k in INT_FIELDS + ("count", "flags", "slots"):
        assert np.array_equal(getattr(merged, k), getattr(whole, k)), k
    assert np.array_equal(merged.since_last, whole.since_last)


def test_sustained_strategy_through_the_batched_runner(histories, monkeypatch):
    """recommend() over the fleet equals the strategy's own per-object run(): the candidates are
    samples and the choice is made on integers, so the requests are equal, not close."""
    from examples.sustained_strategy import SustainedSettings, SustainedStrategy
    from krr_amd import _native
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner
    from test_fleet_exceed_host import sustained_request

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    calls = []
    real = _native.Context.segmented_exceed
    monkeypatch.setattr(_native.Context, "segmented_exceed",
                        lambda self, series, thr, n, *a, **k: (calls.append((series.n_segments, n)),
                                                               real(self, series, thr, n, *a, **k))[1])
    strategy = SustainedStrategy(SustainedSettings(max_share=0.3, max_sustained_slots=1, memory_percentile=Decimal(90),
                                                   memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    runner = BatchedRunner(strategy)
    got = runner.recommend(objects, histories)
    assert calls == [(N, 4)]  # one launch over the fleet, four thresholds
    raw = strategy.run_batch(histories, objects)
    assert len(got) == N
    for o, (h, obj) in enumerate(zip(histories, objects)):
        one = strategy.run(h, obj)
        want = format_result(one, runner.cpu_min_value, runner.memory_min_value)
        for r in (CPU, MEM):
            for field in ("request", "limit"):
                a, b = getattr(got[o][r], field), getattr(want[r], field)
                assert (a is None and b is None) or (a.is_nan() and b.is_nan()) or (a == b and str(a) == str(b)), (o, r)
        loop = sustained_request(h, (50, 75, 90, 95), 0.3, 1)
        if loop is None:
            assert o in (3, 11) and raw[o][CPU].request.is_nan()
        else:
            assert raw[o][CPU].request == loop == one[CPU].request, o

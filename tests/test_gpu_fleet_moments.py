"""krr_amd.api.batch.FleetBatch.moments on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) through the real engine,
against exact rational arithmetic and within krr_segmented_moments' own bounds
(tests/_moments_ref.py), then examples/trend_strategy.py through the BatchedRunner."""
from decimal import Decimal

import numpy as np
import pytest

from _moments_ref import FIELDS, exact_moments, ratios
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY = 4


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, r):
    return np.array([float(x) for samples in h[r].values() for x in samples])


def _hold(mo, series_list):
    """Every series' five moments within the bounds of its exact moments; EMPTY where it has none."""
    assert mo.count.size == len(series_list) and mo.has_trend
    for s, x in enumerate(series_list):
        assert mo.count[s] == x.size == mo.slots[s], s
        if x.size == 0:
            assert mo.flags[s] == EMPTY and all(np.isnan(getattr(mo, k)[s]) for k in FIELDS), s
            continue
        r = ratios({k: getattr(mo, k)[s] for k in FIELDS}, exact_moments(x))
        assert mo.flags[s] == 0 and all(v <= 1.0 for v in r.values()), (s, r)


def test_fleet_and_pod_moments_within_the_bounds(histories):
    from krr_amd.api import FleetBatch

    batch = FleetBatch(histories, device=0)
    assert batch.n_objects == N
    _hold(batch.moments(CPU), [_flat(h, CPU) for h in histories])
    _hold(batch.moments(MEM), [_flat(h, MEM) for h in histories])
    pods = batch.per_pod(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    _hold(pods.moments(CPU), kept)
    assert np.array_equal(np.diff(pods.pod_groups), [sum(1 for x in h[CPU].values() if len(x)) for h in histories])
    # the launch without the trend: the same mean and m2, bit for bit
    light = FleetBatch(histories, device=0).moments(MEM, trend=False)
    full = batch.moments(MEM)
    assert not light.has_trend
    for k in ("mean", "m2"):
        assert np.array_equal(getattr(light, k).view(np.uint64), getattr(full, k).view(np.uint64)), k
    assert np.array_equal(light.count, full.count) and np.array_equal(light.flags, full.flags)


def test_forced_chunks(histories):
    """Chunks re-base the offsets, so a segment may start at the other parity and its last bits
    may differ: count and flags are equal, the values stay within the bounds."""
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small, whole = FleetBatch(histories, engine=eng), FleetBatch(histories, device=0)
    for r in (CPU, MEM):
        assert len(list(eng._series_parts(small.series(r)))) >= 5
        a, c = whole.moments(r), small.moments(r)
        assert np.array_equal(a.count, c.count) and np.array_equal(a.flags, c.flags) and np.array_equal(a.slots, c.slots)
        _hold(c, [_flat(h, r) for h in histories])


def test_trend_strategy_through_the_batched_runner(histories, monkeypatch):
    """recommend() over the fleet equals the strategy's own per-object run().  A pod's moments from
    the fleet-wide launch and from a launch over its object alone may differ in the last bits
    (another start parity), far below the rounding format_result applies; the unrounded requests
    are held to 1e-12 relative, above twice n kappa u for these pods (n <= 40, kappa < 10)."""
    from examples.trend_strategy import TrendHeadroomSettings, TrendHeadroomStrategy
    from krr_amd import _native
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    calls = []
    real = _native.Context.segmented_moments
    monkeypatch.setattr(_native.Context, "segmented_moments",
                        lambda self, series, *a, **k: (calls.append(series.n_segments), real(self, series, *a, **k))[1])
    strategy = TrendHeadroomStrategy(TrendHeadroomSettings(cpu_sigmas=2.0, horizon_slots=30.0,
                                                           memory_percentile=Decimal(90),
                                                           memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    runner = BatchedRunner(strategy)
    got = runner.recommend(objects, histories)
    n_pods = sum(1 for h in histories for x in h[CPU].values() if len(x))
    assert calls == [n_pods]  # one launch over every pod of the fleet
    raw = strategy.run_batch(histories, objects)
    assert len(got) == N
    for o, (h, obj) in enumerate(zip(histories, objects)):
        one = strategy.run(h, obj)
        want = format_result(one, runner.cpu_min_value, runner.memory_min_value)
        for r in (CPU, MEM):
            for field in ("request", "limit"):
                a, b = getattr(got[o][r], field), getattr(want[r], field)
                assert (a is None and b is None) or (a.is_nan() and b.is_nan()) or (a == b and str(a) == str(b)), (o, r)
        if o in (3, 11):
            assert got[o][CPU].request.is_nan() and raw[o][CPU].request.is_nan()
        else:
            assert float(raw[o][CPU].request) == pytest.approx(float(one[CPU].request), rel=1e-12)
    # and the number is the strategy's definition, from numpy alone
    x = [np.array([float(v) for v in s]) for s in histories[0][CPU].values() if len(s)]
    per_pod = [p.mean() + 2.0 * p.std() + max(np.polyfit(np.arange(p.size), p, 1)[0] if p.size > 1 else 0.0, 0.0) * 30.0
               for p in x]
    assert float(raw[0][CPU].request) == pytest.approx(max(per_pod), rel=1e-9)

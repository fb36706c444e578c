"""krr_amd.api.batch.FleetBatch.weighted_percentile on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) through the real engine
against the plain restatement (tests/_wquantile_ref.py), bit for bit: host-packed, chunked, per
pod and resident in HBM with gaps; a window table against the unit-weight answer of the last k
slots; then examples/recency_strategy.py through the BatchedRunner."""
from decimal import Decimal

import numpy as np
import pytest

from _wquantile_ref import EMPTY, MAX_PASSES, Sorted, bits, fraction_of, weights_of, wquantile_one
from krr_amd.api import decay_weights, window_weights  # noqa: F401  (the feature: absent, nothing here runs)
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
nan = np.nan


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, r):
    return np.array([float(x) for samples in h[r].values() for x in samples])


def _hold(values, flags, series_list, table, p):
    """Every series: the value's bits equal the restatement's, NaN where it has no weight."""
    assert values.shape == flags.shape == (len(series_list),)
    num, den = fraction_of(p)
    for s, x in enumerate(series_list):
        b, W = wquantile_one(x, table, num, den)
        present = int(np.count_nonzero(~np.isnan(x)))
        assert flags[s] == (EMPTY if present == 0 else 0), s
        if W == 0:
            assert np.isnan(values[s]), s
        else:
            assert int(values[s:s + 1].view(np.uint64)[0]) == b, (s, values[s])


def test_host_packed_fleet_pods_and_chunks(histories):
    from krr_amd.api import FleetBatch, decay_weights, window_weights
    from krr_amd.core.engine import SimpleEngine

    batch = FleetBatch(histories, device=0)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    tables = {"decay": decay_weights(6, 130), "unit": np.array([1], np.uint64), "short": np.array([0, 9, 2], np.uint64)}
    for r in (CPU, MEM):
        series = [_flat(h, r) for h in histories]
        for name, table in tables.items():
            for p in ("50", "95", "99.9", "100"):
                v, f = batch.weighted_percentile(r, p, table, return_flags=True)
                _hold(v, f, series, table, p)
        assert len(list(eng._series_parts(small.series(r)))) >= 5
        table = tables["decay"]
        c, cf = small.weighted_percentile(r, "95", table, return_flags=True)  # integer sums: chunking changes no bit
        w, wf = batch.weighted_percentile(r, "95", table, return_flags=True)
        assert np.array_equal(c.view(np.uint64), w.view(np.uint64)) and np.array_equal(cf, wf)
        ws = batch.weight_sums(r, table)
        assert np.array_equal(ws, [sum(weights_of(x.size, table)) / 2 ** 32 for x in series])
        raw = eng.wquantile_series(small.series(r), table, "95")
        assert raw["passes"].min() >= 1 and raw["passes"].max() <= MAX_PASSES and raw["wsum"].dtype == np.uint64
        # "the percentile of the last k slots" without re-packing — under THIS rule (ceil rank), which is not
        # percentile(mode="sorted_lower")'s index rule: the restatement decides, not percentile()
        for k in (1, 7, 30):
            v = batch.weighted_percentile(r, "90", window_weights(k, 200))
            for o, x in enumerate(series):
                b, W = Sorted(x[-k:]).answer([1], 90, 1)
                assert (W == 0 and np.isnan(v[o])) or int(v[o:o + 1].view(np.uint64)[0]) == b, (k, o)
    pods = batch.per_pod(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    v, f = pods.weighted_percentile(CPU, "95", tables["decay"], return_flags=True)
    _hold(v, f, kept, tables["decay"], "95")
    dec = batch.to_decimal(v, f)
    own = {s for h in histories for x in h[CPU].values() for s in x}
    assert all(d in own for d in dec)  # a sample's own bits


def test_gapped_fleet_resident_in_hbm():
    import torch

    from krr_amd.api import FleetBatch, decay_weights
    from krr_amd.core.packing import PackedFleet, PackedSeries

    rng = np.random.default_rng(51)
    lens = rng.integers(1, 3001, 14)
    lens[[2, 9]] = 0
    segs = []
    for s, n in enumerate(lens.tolist()):
        x = rng.gamma(2.0, 0.05, n) if s % 2 else np.floor(rng.normal(2e8, 2e7, n))
        x[rng.random(n) < 0.2] = nan
        segs.append(x)
    segs[5][:] = nan
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = torch.device("cuda:0")
    ps = PackedSeries(torch.from_numpy(np.concatenate(segs)).to(dev), torch.from_numpy(offs).to(dev), int(lens.max()), True)
    batch = FleetBatch.from_fleet(PackedFleet(ps, ps), device=0)
    for table in (decay_weights(300, 3000), decay_weights(20, 3000)):
        for p in ("50", "95"):
            v, f = batch.weighted_percentile(MEM, p, table, return_flags=True)
            _hold(v, f, segs, table, p)


def test_recency_strategy_through_the_batched_runner(histories, monkeypatch):
    """recommend() over the fleet equals the strategy's own per-object run(), and the CPU request
    is the max over the pods of the restatement's weighted p95: samples, so equal, not close."""
    from examples.recency_strategy import RecencySettings, RecencyStrategy
    from krr_amd import _native
    from krr_amd.api import decay_weights
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    calls = []
    real = _native.Context.segmented_wquantile
    monkeypatch.setattr(_native.Context, "segmented_wquantile",
                        lambda self, series, *a, **k: (calls.append(series.n_segments), real(self, series, *a, **k))[1])
    strategy = RecencyStrategy(RecencySettings(half_life_slots=6, memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    runner = BatchedRunner(strategy)
    got = runner.recommend(objects, histories)
    n_pods = sum(1 for h in histories for x in h[CPU].values() if len(x))
    assert calls == [n_pods]  # one launch over every pod of the fleet
    raw = strategy.run_batch(histories, objects)
    table = decay_weights(6, max(len(x) for h in histories for x in h[CPU].values()))
    for o, (h, obj) in enumerate(zip(histories, objects)):
        one = strategy.run(h, obj)
        want = format_result(one, runner.cpu_min_value, runner.memory_min_value)
        for r in (CPU, MEM):
            for field in ("request", "limit"):
                a, b = getattr(got[o][r], field), getattr(want[r], field)
                assert (a is None and b is None) or (a.is_nan() and b.is_nan()) or (a == b and str(a) == str(b)), (o, r)
        pods = [x for x in h[CPU].values() if len(x)]
        if not pods:
            assert o in (3, 11) and raw[o][CPU].request.is_nan()
            continue
        per_pod = []
        for x in pods:
            b, _ = wquantile_one([float(s) for s in x], table, 95, 1)
            per_pod.append(next(s for s in x if bits(float(s)) == b))
        assert raw[o][CPU].request == max(per_pod) == one[CPU].request, o
        assert raw[o][CPU].limit >= raw[o][CPU].request
        assert raw[o][MEM].request == max(s for x in h[MEM].values() for s in x) * Decimal("1.1")

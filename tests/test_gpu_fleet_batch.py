"""krr_amd.api.batch.FleetBatch on the MI355X: 50 objects of 0-3 pods with up to 3,000 samples
per pod, against Python over the Decimal lists and the CPU oracle.

CPU samples are multiples of 1/1024 and memory samples integers, so every partial sum is exact in
float64 whatever the order: the mean a strategy computes from a fleet-wide launch and from a
launch over one object alone (another start offset, so possibly another summation order) are then
the same number, and the example strategy's batched and per-object results can be compared with
``==``."""
import json
import math
from decimal import Decimal
from types import SimpleNamespace

import numpy as np
import pytest

from krr_amd.core.models.allocations import ResourceAllocations, ResourceType

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
MODES = ["ref_index", "sorted_lower", "linear"]
PCTS = ["50", "95", "99"]
N_OBJECTS = 50
EMPTY = 4


@pytest.fixture(scope="module")
def world():
    """Objects, their float samples per pod, the HistoryData (Decimal lists) and the per-pod
    query_range bodies — built once."""
    from krr_amd.api.models import K8sObjectData
    from krr_amd.utils.prom_decimal import prom_decimal, prom_format

    rng = np.random.default_rng(33)
    objects, histories, bodies = [], [], {"cpu": [], "memory": []}

    def doc(xs):
        result = [{"metric": {}, "values": [[1700000000 + 60 * i, prom_format(float(v))] for i, v in enumerate(xs)]}]
        return json.dumps({"status": "success", "data": {"resultType": "matrix", "result": result if len(xs) else []}},
                          separators=(",", ":")).encode()

    for o in range(N_OBJECTS):
        pods = [f"o{o}-p{p}" for p in range(int(rng.integers(0, 4)))]
        lens = [int(rng.integers(1, 3001)) for _ in pods]
        if o % 10 == 9 and lens:
            lens[0] = 0  # a pod without samples: dropped by every packer
        cpu = [np.round(rng.gamma(2.0, 0.05 * (1 + 4 * (i == 0)), n) * 1024) / 1024 for i, n in enumerate(lens)]
        mem = [np.floor(rng.normal(2e8, 2e7, n)) for n in lens]
        objects.append(K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=pods, namespace="ns",
                                     kind="Deployment", allocations=ResourceAllocations(requests={}, limits={})))
        histories.append({CPU: {p: [prom_decimal(float(v)) for v in x] for p, x in zip(pods, cpu)},
                          MEM: {p: [prom_decimal(float(v)) for v in x] for p, x in zip(pods, mem)}})
        bodies["cpu"].append([doc(x) for x in cpu])
        bodies["memory"].append([doc(x) for x in mem])
    assert sum(len(o.pods) == 0 for o in objects) >= 3
    return SimpleNamespace(objects=objects, histories=histories, bodies=bodies)


@pytest.fixture(scope="module")
def batch(world):
    from krr_amd.api import FleetBatch

    return FleetBatch(world.histories, device=0)


def _flat(h, r):
    return [x for samples in h[r].values() for x in samples]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _sum_bound(ps):
    """n * 2^-53 * sum|x| per segment (tests/test_gpu_stats.py derives it)."""
    vals, offs = np.abs(np.asarray(ps.values)), np.asarray(ps.offsets)
    return np.array([(offs[s + 1] - offs[s]) * 2.0 ** -53 * math.fsum(vals[offs[s]:offs[s + 1]].tolist())
                     for s in range(offs.size - 1)])


@pytest.mark.parametrize("resource", [CPU, MEM])
def test_stats_equal_python_over_the_decimal_lists(world, batch, resource):
    st = batch.stats(resource)
    mn, mx = batch.to_decimal(st.min, st.flags), batch.to_decimal(st.max, st.flags)
    for o, h in enumerate(world.histories):
        x = _flat(h, resource)
        assert st.count[o] == len(x)
        if not x:
            assert st.flags[o] == EMPTY and mn[o].is_nan() and mx[o].is_nan() and st.sum[o] == 0 and np.isnan(st.mean[o])
            continue
        assert (mn[o], mx[o]) == (min(x), max(x)), o
        assert st.sum[o] == float(sum(x)) and st.mean[o] == st.sum[o] / len(x), o  # exact data: any order
    assert batch.exact_mask(resource) is None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resource", [CPU, MEM])
def test_percentiles_equal_the_oracle(batch, resource, mode):
    from krr_amd.core.engine import percentile_params
    from oracle import oracle

    ps = batch.series(resource)
    got, flags = batch.percentiles(resource, PCTS, mode=mode, return_flags=True)
    assert got.shape == (len(PCTS), N_OBJECTS)
    for j, p in enumerate(PCTS):
        prm = percentile_params(Decimal(p), mode)
        ov, on, of = oracle.percentile(ps.values, ps.offsets, prm.mode, prm.p_num, prm.p_den, prm.q)
        same = (got[j].view(np.uint64) == ov.view(np.uint64)) | (np.isnan(got[j]) & np.isnan(ov))
        if mode == "linear":  # the sign of a zero LINEAR result is unspecified
            same |= (got[j] == 0) & (ov == 0)
        assert same.all(), (p, np.nonzero(~same)[0][:8])
        assert np.array_equal(flags[j], of.astype(np.uint32))
        assert np.array_equal(batch.counts(resource, p, mode=mode), on)
    one = batch.percentile(resource, "95", mode=mode)
    assert np.array_equal(one, got[1], equal_nan=True)


def test_per_pod_equals_python_per_pod(world, batch):
    pods = batch.per_pod(CPU)
    kept = [[x for x in h[CPU].values() if len(x)] for h in world.histories]
    flat = [x for k in kept for x in k]
    assert np.array_equal(np.diff(pods.pod_groups), [len(k) for k in kept]) and pods.n_objects == len(flat)
    st = pods.stats(CPU)
    assert pods.to_decimal(st.max) == [max(x) for x in flat] and pods.to_decimal(st.min) == [min(x) for x in flat]
    assert np.array_equal(st.count, [len(x) for x in flat])
    assert np.array_equal(st.sum, [float(sum(x)) for x in flat])
    p95 = pods.to_decimal(pods.percentile(CPU, "95", mode="sorted_lower"))
    assert p95 == [sorted(x)[int((len(x) - 1) * Decimal(95) / 100)] for x in flat]
    # the max over an object's pods of each pod's p95, folded on the host from pod_groups
    g = pods.pod_groups
    v = pods.percentile(CPU, "95", mode="sorted_lower")
    for o, k in enumerate(kept):
        if k:
            assert v[g[o]:g[o + 1]].max() == float(max(sorted(x)[int((len(x) - 1) * Decimal(95) / 100)] for x in k))
    with pytest.raises(ValueError, match="pod boundaries"):
        batch.per_pod(MEM)


def test_tiny_chunks_equal_the_unchunked_run(world, batch):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    eng = SimpleEngine(0)
    eng.chunk_bytes = 64 << 10  # 8,192 samples per chunk: a dozen or more chunks per resource
    small = FleetBatch(world.histories, engine=eng)
    for r in (CPU, MEM):
        a, c = batch.stats(r), small.stats(r)
        assert len(list(eng._series_parts(small.series(r)))) >= 8
        assert _same_bits(a.min, c.min) and _same_bits(a.max, c.max)
        assert np.array_equal(a.count, c.count) and np.array_equal(a.flags, c.flags)
        # chunking re-bases the offsets (another parity, another summation order): the bound
        assert (np.abs(a.sum - c.sum) <= _sum_bound(batch.series(r))).all()
        assert np.array_equal(a.sum, c.sum)  # ... and on this exact data no difference at all
        va = batch.percentiles(r, PCTS, mode="sorted_lower")
        vc = small.percentiles(r, PCTS, mode="sorted_lower")
        assert np.array_equal(va, vc, equal_nan=True)


def test_device_packed_fleet_equals_the_host_packed_one(world, batch):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.device_pack import default_packer
    from krr_amd.core.packing import PackedFleet

    cpu, mem = default_packer(0).pack_many([world.bodies["cpu"], world.bodies["memory"]])
    assert cpu.via == mem.via == "device" and isinstance(cpu.series.values, torch.Tensor) and cpu.series.values.is_cuda
    dev = FleetBatch.from_fleet(PackedFleet(cpu.series, mem.series))
    assert dev.n_objects == N_OBJECTS
    for r in (CPU, MEM):
        a, c = batch.stats(r), dev.stats(r)
        assert _same_bits(a.min, c.min) and _same_bits(a.max, c.max) and np.array_equal(a.sum, c.sum)
        assert np.array_equal(a.count, c.count) and np.array_equal(a.flags, c.flags)
        for mode in MODES:
            assert np.array_equal(batch.percentiles(r, PCTS, mode=mode), dev.percentiles(r, PCTS, mode=mode),
                                  equal_nan=True)
    hp, dp = batch.per_pod(CPU), dev.per_pod(CPU)
    assert np.array_equal(hp.pod_groups, dp.pod_groups)
    assert _same_bits(hp.stats(CPU).max, dp.stats(CPU).max) and np.array_equal(hp.stats(CPU).sum, dp.stats(CPU).sum)
    # the body packers keep the pod boundaries of every series they pack, memory included
    # (pack_resource, behind FleetBatch(histories), attaches them to the CPU series only)
    mp = dev.per_pod(MEM)
    flat = [x for h in world.histories for x in h[MEM].values() if len(x)]
    assert np.array_equal(mp.pod_groups, hp.pod_groups)
    assert mp.to_decimal(mp.stats(MEM).max) == [max(x) for x in flat]


def test_example_strategy_through_the_batched_runner(world, monkeypatch):
    from examples.batch_strategy import MeanHeadroomSettings, MeanHeadroomStrategy
    from krr_amd import _native
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner

    calls = []
    real_stats, real_pct = _native.Context.segmented_stats, _native.Context.segmented_percentiles
    monkeypatch.setattr(_native.Context, "segmented_stats",
                        lambda self, series, *a, **k: (calls.append(("stats", series.n_segments)),
                                                       real_stats(self, series, *a, **k))[1])
    monkeypatch.setattr(_native.Context, "segmented_percentiles",
                        lambda self, series, *a, **k: (calls.append(("pct", series.n_segments)),
                                                       real_pct(self, series, *a, **k))[1])
    strategy = MeanHeadroomStrategy(MeanHeadroomSettings(cpu_headroom=Decimal("1.3"), memory_percentile=Decimal("97.5"),
                                                         memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    runner = BatchedRunner(strategy)
    got = runner.recommend(world.objects, world.histories)
    # one launch per resource for the whole fleet: the CPU mean, the memory percentile
    assert calls == [("stats", N_OBJECTS), ("pct", N_OBJECTS)]
    want = [format_result(strategy.run(h, o), runner.cpu_min_value, runner.memory_min_value)
            for h, o in zip(world.histories, world.objects)]
    assert len(got) == N_OBJECTS
    for o, (g, w) in enumerate(zip(got, want)):
        for r in (CPU, MEM):
            for field in ("request", "limit"):
                a, b = getattr(g[r], field), getattr(w[r], field)
                assert (a is None and b is None) or (a.is_nan() and b.is_nan()) or (a == b and str(a) == str(b)), (o, r)
    # and the numbers are the strategy's definition, from Python alone
    with_data = next(o for o, h in enumerate(world.histories) if _flat(h, CPU))
    x, m = _flat(world.histories[with_data], CPU), _flat(world.histories[with_data], MEM)
    raw = strategy.run(world.histories[with_data], world.objects[with_data])
    assert raw[CPU].request == Decimal(repr(float(sum(x)) / len(x))) * Decimal("1.3")
    assert raw[MEM].request == sorted(m)[int((len(m) - 1) * Decimal("97.5") / 100)] * Decimal("1.1")
    empty = next(o for o, h in enumerate(world.histories) if not _flat(h, CPU))
    assert got[empty][CPU].request.is_nan() and got[empty][MEM].request.is_nan()

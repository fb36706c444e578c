"""cpu_aggregation = "pods_max" from raw Prometheus bodies on the MI355X: a fleet packed by the
device packer (pod boundaries as tensors in HBM, krr_json_pod_bounds) runs through
``SimpleEngine`` with those tensors as they are and gives, bit for bit, what the host-packed
fleet gives; ``BatchedRunner.recommend_from_bodies`` / ``recommend_from_grouped`` give the host
parser's strings with every parser; ``integration.install`` with the body-level loaders gives the
reference loader's results.

CPU samples are finite throughout: a NaN CPU sample raises InvalidOperation under sorted_lower
in the reference's own rule (tests/test_gpu_pods_max.py leaves such histories out as well)."""
import asyncio
import json
import re
import sys
import types
from decimal import Decimal
from types import SimpleNamespace

import numpy as np
import pytest

from krr_amd.core.models.allocations import ResourceAllocations, ResourceType  # noqa: F401 (the stand-in runner's module types)

pytestmark = pytest.mark.gpu

MODES = ["ref_index", "sorted_lower", "linear"]
N_OBJECTS = 80
EMPTY = b'{"status":"success","data":{"resultType":"matrix","result":[]}}'


def _build():
    """80 objects of 0-4 pods; some pods have no series (dropped bodies); every fifth object
    with two or more pods has ONE hot pod among idle ones, so that the max over the pods'
    percentiles is not the percentile of the concatenation."""
    from krr_amd.api.models import K8sObjectData
    from krr_amd.utils.prom_decimal import prom_format

    rng = np.random.default_rng(21)
    objects, series = [], {}
    for o in range(N_OBJECTS):
        pods = [f"o{o}-p{p}" for p in range(int(rng.integers(0, 5)))]
        hot = int(rng.integers(0, len(pods))) if len(pods) >= 2 and o % 5 == 0 else -1
        for i, p in enumerate(pods):
            if hot < 0 and rng.random() < 0.15:
                continue  # no series for this pod
            n = int(rng.integers(1, 400))
            scale = 0.01 if hot >= 0 and i != hot else (0.3 if i == hot else 0.05)
            series[("cpu", p)] = [prom_format(float(round(v, 5))) for v in rng.gamma(2.0, scale, n)]
            series[("memory", p)] = [prom_format(float(int(v))) for v in rng.normal(2e8, 2e7, n)]
        # two interleaved clusters: the grouped loader packs each apart and reorders the segments
        objects.append(K8sObjectData(cluster=f"k{o % 2}", name=f"app-{o}", container="main" if o % 3 else "side",
                                     pods=pods, namespace="ns" if o % 2 else "other", kind="Deployment",
                                     allocations=ResourceAllocations(requests={}, limits={})))
    return objects, series


def _result(rt, pods, series, labelled):
    return [{"metric": {"pod": p} if labelled else {}, "values": [[1700000000 + 60 * i, v] for i, v in
                                                                  enumerate(series[(rt, p)])]}
            for p in pods if (rt, p) in series]


def _doc(result) -> bytes:
    return json.dumps({"status": "success", "data": {"resultType": "matrix", "result": result}},
                      separators=(",", ":")).encode()


@pytest.fixture(scope="module")
def world():
    """The fleet, its per-pod and grouped bodies, and the host packer's fleet — built once."""
    from krr_amd.core.fleet_query import FleetQueryPlan
    from krr_amd.core.packing import PackedFleet
    from krr_amd.core.prom_native import pack_query_range_bodies

    objects, series = _build()
    per_pod = {rt: [[_doc(_result(rt, [p], series, False)) for p in o.pods] for o in objects]
               for rt in ("cpu", "memory")}
    plan = FleetQueryPlan(objects)
    grouped = {rt: [_doc(_result(rt, g.pods, series, True)) for g in plan.groups] for rt in ("cpu", "memory")}
    host = PackedFleet(pack_query_range_bodies(per_pod["cpu"]), pack_query_range_bodies(per_pod["memory"]))
    assert host.cpu.n_pods > N_OBJECTS and any(b == EMPTY for bodies in per_pod["cpu"] for b in bodies)
    return SimpleNamespace(objects=objects, series=series, per_pod=per_pod, plan=plan, grouped=grouped, host=host)


@pytest.fixture(scope="module")
def device_fleet(world):
    from krr_amd.core.device_pack import default_packer
    from krr_amd.core.packing import PackedFleet

    cpu, mem = default_packer(0).pack_many([world.per_pod["cpu"], world.per_pod["memory"]])
    assert cpu.via == mem.via == "device"
    return PackedFleet(cpu.series, mem.series)


def _params(p, mode):
    from krr_amd.core.engine import percentile_params

    return percentile_params(Decimal(p), mode)


def _same_raw(got, want):
    for k in ("cpu_value", "mem_value"):
        assert np.array_equal(getattr(got, k).view(np.uint64), getattr(want, k).view(np.uint64)), k
    for k in ("cpu_count", "cpu_flags", "mem_count", "mem_flags"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.pods is not None and want.pods is not None
    assert np.array_equal(got.pods["pod_value"].view(np.uint64), want.pods["pod_value"].view(np.uint64))
    for k in ("pod_count", "pod_flags", "cpu_pod"):
        assert np.array_equal(got.pods[k], want.pods[k]), k


@pytest.mark.parametrize("mode", MODES)
def test_engine_on_device_packed_fleet_equals_host_packed(world, device_fleet, mode):
    import torch

    from krr_amd.core.engine import SimpleEngine

    assert isinstance(device_fleet.cpu.pod_offsets, torch.Tensor) and device_fleet.cpu.pod_offsets.is_cuda
    eng = SimpleEngine(0)
    prm = _params(99, mode)
    want = eng.run_packed(world.host, prm, aggregation="pods_max", return_pods=True)
    got = eng.run_packed(device_fleet, prm, aggregation="pods_max", return_pods=True)
    _same_raw(got, want)
    assert want.pods["pod_count"].size == world.host.cpu.n_pods and (want.pods["cpu_pod"] > 0).any()
    if mode != "ref_index":
        flat = eng.run_packed(device_fleet, prm)
        assert (got.cpu_value > flat.cpu_value).any()  # the hot pod decides, not the flat percentile


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pcts", [(95, 99), (66, 96)])
def test_engine_multi_on_device_packed_fleet_equals_host_packed(world, device_fleet, pcts, mode):
    from krr_amd.core.engine import SimpleEngine

    eng = SimpleEngine(0)
    plist = [_params(p, mode) for p in pcts]
    want = eng.run_packed_multi(world.host, plist, aggregation="pods_max", return_pods=True)
    got = eng.run_packed_multi(device_fleet, plist, aggregation="pods_max", return_pods=True)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        _same_raw(g, w)


def test_series_without_pod_boundaries_is_still_refused(device_fleet):
    """A resident series put together by hand without the fields: the ValueError, before any launch."""
    from krr_amd.core.engine import SimpleEngine
    from krr_amd.core.packing import PackedFleet, PackedSeries

    bare = PackedFleet(PackedSeries(device_fleet.cpu.values, device_fleet.cpu.offsets, device_fleet.cpu.max_len),
                       device_fleet.mem)
    with pytest.raises(ValueError, match="device packer"):
        SimpleEngine(0).run_packed(bare, _params(99, "linear"), aggregation="pods_max")
    with pytest.raises(ValueError, match="device packer"):
        SimpleEngine(0).run_packed_multi(bare, [_params(95, "linear"), _params(99, "linear")], aggregation="pods_max")


def _strategy(kind, aggregation="pods_max"):
    from krr_amd.strategies.simple import SimpleStrategy, SimpleStrategySettings
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    if kind == "simple":
        return SimpleStrategy(SimpleStrategySettings(cpu_aggregation=aggregation))
    return SimpleLimitStrategy(SimpleLimitStrategySettings(cpu_aggregation=aggregation))


def _strings(results):
    return [tuple(str(getattr(r[rt], f)) for rt in ResourceType for f in ("request", "limit")) for r in results]


@pytest.fixture(scope="module")
def host_strings(world):
    """kind -> the per-pod host path's rounded results as strings."""
    from krr_amd.core.runner import BatchedRunner

    return {kind: _strings(BatchedRunner(_strategy(kind), 5, 10).recommend_from_bodies(
        world.per_pod["cpu"], world.per_pod["memory"], parser="host")) for kind in ("simple", "simple_limit")}


@pytest.mark.parametrize("parser", ["device", "hybrid"])
@pytest.mark.parametrize("kind", ["simple", "simple_limit"])
def test_recommend_from_bodies_equals_the_host_parser(world, host_strings, kind, parser):
    from krr_amd.core.runner import BatchedRunner

    got = BatchedRunner(_strategy(kind), 5, 10).recommend_from_bodies(world.per_pod["cpu"], world.per_pod["memory"],
                                                                      parser=parser)
    assert _strings(got) == host_strings[kind] and len(got) == N_OBJECTS


@pytest.mark.parametrize("parser", ["host", "device", "hybrid"])
@pytest.mark.parametrize("kind", ["simple", "simple_limit"])
def test_recommend_from_grouped_equals_the_per_pod_host_path(world, host_strings, kind, parser):
    from krr_amd.core.runner import BatchedRunner

    got = BatchedRunner(_strategy(kind), 5, 10).recommend_from_grouped(world.plan, world.grouped["cpu"],
                                                                       world.grouped["memory"], parser=parser)
    assert _strings(got) == host_strings[kind]


@pytest.mark.parametrize("kind", ["simple", "simple_limit"])
def test_pods_max_differs_from_concat_on_this_fleet(world, host_strings, kind):
    from krr_amd.core.runner import BatchedRunner

    flat = _strings(BatchedRunner(_strategy(kind, "concat"), 5, 10).recommend_from_bodies(
        world.per_pod["cpu"], world.per_pod["memory"]))
    differs = [a != b for a, b in zip(flat, host_strings[kind])]
    assert any(differs) and not all(differs)
    # memory is the same rule under both
    assert [s[2:] for s in flat] == [s[2:] for s in host_strings[kind]]


# ---- krr_amd.integration.install() over a Prometheus stand-in ---------------------------------

class Session:
    """Answers the reference's per-pod query and the grouped ``sum by (pod)`` query."""

    def __init__(self, series):
        self.series = series

    def get(self, url, params=None, verify=None, headers=None):
        q = params["query"]
        rt = "cpu" if "cpu_usage" in q else "memory"
        m = re.search(r'pod=~"([^"]*)"', q)
        if m:
            body = _doc(_result(rt, m.group(1).split("|"), self.series, True))
        else:
            body = _doc(_result(rt, [re.search(r'pod="([^"]*)"', q).group(1)], self.series, False))
        return SimpleNamespace(status_code=200, content=body)


class Runner:
    """runner.py:17-137's attributes that install() and the loaders read."""

    def __init__(self, strategy, series):
        self._strategy = strategy
        self.config = SimpleNamespace(cpu_min_value=5, memory_min_value=10)
        self._series = series

    def _get_prometheus_loader(self, cluster):
        series = self._series

        class Loader:  # prometheus.py:108-155's output shape: {pod: [Decimal]}, empty pods dropped
            prometheus = SimpleNamespace(_session=Session(series), url="http://p", headers={}, ssl_verification=True)

            async def gather_data(self, obj, resource, period, *, timeframe):
                rt = "cpu" if resource == ResourceType.CPU else "memory"
                return {p: [Decimal(v) for v in series[(rt, p)]] for p in obj.pods if (rt, p) in series}

        return Loader()

    async def _gather_objects_recommendations(self, objects):
        raise AssertionError("install() did not patch the runner")


@pytest.fixture(scope="module")
def reference_strategy():
    """An object of the reference SimpleStrategy's shape (class robusta_krr.strategies.simple.
    SimpleStrategy, settings with ``__fields_set__``)."""
    from krr_amd.strategies.simple import SimpleStrategySettings

    mod = types.ModuleType("robusta_krr.strategies.simple")

    class SimpleStrategy:
        def __init__(self, settings):
            self.settings = settings

    SimpleStrategy.__module__ = mod.__name__
    mod.SimpleStrategy = SimpleStrategy
    return mod, SimpleStrategy(SimpleStrategySettings())


def _install_and_gather(world, ref_strategy, **switches):
    from krr_amd import integration

    integration.install(Runner, cpu_aggregation="pods_max", **switches)
    try:
        got = asyncio.run(Runner(ref_strategy, world.series)._gather_objects_recommendations(world.objects))
    finally:
        integration.uninstall(Runner)
    return [(str(a.requests[ResourceType.CPU]), str(a.limits[ResourceType.CPU]), str(a.requests[ResourceType.Memory]),
             str(a.limits[ResourceType.Memory])) for a in got]


@pytest.fixture(scope="module")
def reference_loader_results(world, reference_strategy):
    mod, strat = reference_strategy
    with pytest.MonkeyPatch.context() as m:
        m.setitem(sys.modules, "robusta_krr.strategies.simple", mod)
        return _install_and_gather(world, strat, loader="reference")


@pytest.mark.parametrize("loader,parser", [("bodies", "device"), ("bodies", "hybrid"), ("bodies", "host"),
                                           ("grouped", "device"), ("grouped", "hybrid"), ("grouped", "host")])
def test_install_pods_max_with_body_loaders_equals_reference_loader(monkeypatch, world, reference_strategy,
                                                                    reference_loader_results, loader, parser):
    mod, strat = reference_strategy
    monkeypatch.setitem(sys.modules, "robusta_krr.strategies.simple", mod)
    got = _install_and_gather(world, strat, loader=loader, parser=parser)
    assert len(got) == N_OBJECTS and got == reference_loader_results
    concat = None
    if (loader, parser) == ("bodies", "device"):  # the switch is what makes the difference
        from krr_amd import integration

        integration.install(Runner, loader=loader)
        try:
            concat = asyncio.run(Runner(strat, world.series)._gather_objects_recommendations(world.objects))
        finally:
            integration.uninstall(Runner)
        assert any(str(a.requests[ResourceType.CPU]) != g[0] for a, g in zip(concat, got))

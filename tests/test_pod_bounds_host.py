"""Pod boundaries (PackedSeries.pod_offsets / pod_groups, cpu_aggregation = "pods_max") kept by
the host-side packers of grouped bodies and where fleets are joined (runs anywhere, CPU only).

The per-pod host packer (``pack_query_range_bodies``) is the reference: the grouped packer
(``FleetQueryPlan.pack``) and ``integration._reorder`` must give its fields, element for element,
on the same samples."""
import asyncio
import json
import re
from types import SimpleNamespace

import numpy as np
import pytest

from krr_amd import integration
from krr_amd.core.fleet_query import FleetQueryPlan, pod_query
from krr_amd.core.models.allocations import ResourceType
from krr_amd.core.packing import PackedSeries, pod_fields
from krr_amd.core.prom_native import pack_query_range_bodies
from krr_amd.strategies.simple import SimpleStrategySettings
from krr_amd.utils.prom_decimal import prom_format


class Session:
    """A Prometheus stand-in answering the per-pod and the grouped query forms."""

    def __init__(self, series):
        self.series = series

    def get(self, url, params=None, verify=None, headers=None):
        q = params["query"]
        rt = "cpu" if "cpu_usage" in q else "memory"
        m = re.search(r'pod=~"([^"]*)"', q)
        if m:
            res = [{"metric": {"pod": p}, "values": [[i, prom_format(v)] for i, v in enumerate(self.series[(rt, p)])]}
                   for p in m.group(1).split("|") if (rt, p) in self.series]
        else:
            p = re.search(r'pod="([^"]*)"', q).group(1)
            res = ([{"metric": {}, "values": [[i, prom_format(v)] for i, v in enumerate(self.series[(rt, p)])]}]
                   if (rt, p) in self.series else [])
        body = json.dumps({"status": "success", "data": {"resultType": "matrix", "result": res}}).encode()
        return SimpleNamespace(status_code=200, content=body)


def _fleet(seed=3, clusters=2):
    """23 objects of 0-3 pods, some pods without a series."""
    rng = np.random.default_rng(seed)
    objects, series = [], {}
    for o in range(23):
        pods = [f"c{o % 2}-o{o}-p{p}" for p in range(int(rng.integers(0, 4)))]
        for p in pods:
            if rng.random() < 0.85:
                n = int(rng.integers(1, 60))
                series[("cpu", p)] = rng.gamma(2.0, 0.05, n)
                series[("memory", p)] = np.floor(rng.normal(2e8, 2e7, n))
        objects.append(SimpleNamespace(cluster=f"k{o % clusters}", namespace="ns" if o % 3 else "other",
                                       container="main", pods=pods, name=f"o{o}"))
    return objects, series


def _runner(session):
    prom = SimpleNamespace(_session=session, url="http://p", headers={}, ssl_verification=True)
    return SimpleNamespace(_get_prometheus_loader=lambda cluster: SimpleNamespace(prometheus=prom))


def _same_pod_fields(got: PackedSeries, want: PackedSeries):
    assert want.pod_offsets is not None and want.pod_groups is not None
    assert got.pod_offsets is not None and got.pod_groups is not None
    for g, w in ((got.pod_offsets, want.pod_offsets), (got.pod_groups, want.pod_groups)):
        g = np.asarray(g)
        assert g.dtype == np.int64 and np.array_equal(g, w)


def test_grouped_host_packer_keeps_the_pod_boundaries():
    objects, series = _fleet(clusters=1)
    assert any(len(o.pods) == 0 for o in objects) and any(len(o.pods) == 3 for o in objects)
    assert any(("cpu", p) not in series for o in objects for p in o.pods)  # pods without a series
    prom = _runner(Session(series))._get_prometheus_loader(None).prometheus
    q = integration.query_range_fn(prom, 0, 1, "1m")
    plan = FleetQueryPlan(objects)
    grouped = plan.fetch(q)
    for rt in ResourceType:
        per_pod = [[q(pod_query(rt, o.namespace, p, o.container)) for p in o.pods] for o in objects]
        want = pack_query_range_bodies(per_pod)
        got = plan.pack(grouped[rt])
        assert np.array_equal(got.offsets, want.offsets)
        _same_pod_fields(got, want)
        assert want.n_pods > 0 and got.pod_offsets[-1] == got.offsets[-1]
        # the other return forms carry them too
        _same_pod_fields(plan.pack(grouped[rt], want_timestamps=True, return_pod_counts=True)[0], want)
    fleet = plan.pack_fleet(grouped[ResourceType.CPU], grouped[ResourceType.Memory])
    _same_pod_fields(fleet.cpu, pack_query_range_bodies(
        [[q(pod_query(ResourceType.CPU, o.namespace, p, o.container)) for p in o.pods] for o in objects]))


def test_grouped_loader_across_clusters_keeps_the_pod_boundaries():
    """Two interleaved clusters: each cluster's grouped bodies are packed apart and put back in
    fleet order (integration._reorder); every object keeps its own pods."""
    objects, series = _fleet()
    settings = SimpleStrategySettings()
    runner = _runner(Session(series))
    cpu_b, mem_b = asyncio.run(integration.fetch_pod_bodies(runner, objects, settings))
    got = asyncio.run(integration.fetch_grouped_fleet(runner, objects, settings))
    for g, w in ((got.cpu, pack_query_range_bodies(cpu_b)), (got.mem, pack_query_range_bodies(mem_b))):
        assert np.array_equal(g.offsets, w.offsets)
        assert np.array_equal(g.values.view(np.int64), w.values.view(np.int64))
        _same_pod_fields(g, w)


def _series_of(objs, pod_lens, values_of):
    """The PackedSeries of objects ``objs`` (in that order), each the concatenation of its pods."""
    lens = [n for o in objs for n in pod_lens[o]]
    vals = np.concatenate([values_of[o] for o in objs] + [np.zeros(0)])
    offs = np.concatenate([[0], np.cumsum([sum(pod_lens[o]) for o in objs])]).astype(np.int64)
    ps = PackedSeries(vals, offs, int(np.diff(offs).max(initial=0)))
    ps.pod_offsets, ps.pod_groups = pod_fields(lens, [len(pod_lens[o]) for o in objs])
    return ps


def _parts(seed):
    rng = np.random.default_rng(seed)
    n = 17
    pod_lens = [[int(x) for x in rng.integers(1, 9, size=int(rng.integers(0, 4)))] for _ in range(n)]
    pod_lens[0], pod_lens[n - 1] = [], [3]
    values_of = [rng.random(sum(p)) for p in pod_lens]
    order = [int(x) for x in rng.permutation(n)]
    cuts = [0, 5, 6, n]
    parts = [_series_of(order[a:b], pod_lens, values_of) for a, b in zip(cuts[:-1], cuts[1:])]
    return parts, order, _series_of(list(range(n)), pod_lens, values_of)


@pytest.mark.parametrize("seed", [1, 2])
def test_reorder_carries_the_pod_boundaries(seed):
    parts, order, want = _parts(seed)
    got = integration._reorder(parts, order)
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.values, want.values)
    _same_pod_fields(got, want)
    for k in range(len(parts)):  # a part without the fields: the result has none
        bare = [PackedSeries(p.values, p.offsets, p.max_len) if j == k else p for j, p in enumerate(parts)]
        res = integration._reorder(bare, order)
        assert res.pod_offsets is None and res.pod_groups is None
        assert np.array_equal(res.values, want.values)


@pytest.mark.parametrize("host_part", [None, 1])
def test_reorder_of_tensor_series_carries_the_pod_boundaries(host_part):
    """The torch path (series in HBM; here CPU tensors), all tensor parts or one numpy part among
    them as after a host fallback: the numpy path's fields, as int64 tensors."""
    import torch

    parts, order, want = _parts(5)

    def tensors(p):
        t = PackedSeries(torch.from_numpy(p.values), torch.from_numpy(p.offsets), p.max_len)
        t.pod_offsets, t.pod_groups = torch.from_numpy(p.pod_offsets), torch.from_numpy(p.pod_groups)
        return t

    got = integration._reorder([p if k == host_part else tensors(p) for k, p in enumerate(parts)], order)
    assert isinstance(got.pod_offsets, torch.Tensor) and got.pod_offsets.dtype == torch.int64
    assert np.array_equal(got.values.numpy(), want.values)
    _same_pod_fields(PackedSeries(None, None, 0, pod_offsets=got.pod_offsets.numpy(),
                                  pod_groups=got.pod_groups.numpy()), want)
    assert got.pod_max_len == int(np.diff(want.pod_offsets).max())

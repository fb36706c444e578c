"""cpu_aggregation = "pods_max" above the engine, without a GPU: the strategy's dispatch, the
pod-level exact path (krr_amd.core.exact.resolve_pods) and the runner, with the device engine
stood in for by the CPU oracle (tests/_standin.py) and the fold by its numpy restatement
(test_gpu_group_max.fold).  tests/test_gpu_pods_max.py runs the same golden check on the MI355X."""
import dataclasses
import decimal
from decimal import Decimal

import numpy as np
import pytest

from _standin import oracle_run_packed
from test_gpu_group_max import fold
from test_gpu_pods_max import COUNTS, hist, load, obj, same_decimal, split_cases, three_objects


def standin_run_packed(self, fleet, params, aggregation="concat", return_pods=False):
    """SimpleEngine.run_packed: the flat stand-in, or for "pods_max" the oracle over the pod
    segments, the fold, and krr_locate's answers over the pod segments."""
    from krr_amd.core.packing import PackedFleet, pod_view

    if aggregation != "pods_max":
        return oracle_run_packed(self, fleet, params)
    view = pod_view(fleet.cpu)
    pod_raw = oracle_run_packed(self, PackedFleet(view, dataclasses.replace(fleet.mem, exact=None, sources=None)),
                                params)
    plain_cpu = dataclasses.replace(fleet.cpu, exact=None, sources=None)
    raw = oracle_run_packed(self, PackedFleet(plain_cpu, fleet.mem), params)  # the memory half and its locate
    wv, wn, wf, wa = fold(np.asarray(fleet.cpu.pod_groups), pod_raw.cpu_value[None], pod_raw.cpu_count,
                          pod_raw.cpu_flags[None])
    raw.cpu_value, raw.cpu_count, raw.cpu_flags = wv[0].view(np.float64), wn, wf[0]
    if return_pods:
        raw.pods = {"pod_value": pod_raw.cpu_value, "pod_count": pod_raw.cpu_count, "pod_flags": pod_raw.cpu_flags,
                    "cpu_pod": wa[0], "locate": {"cpu": pod_raw.locate["cpu"]} if (pod_raw.locate or {}).get("cpu")
                    else None}
    return raw


@pytest.fixture()
def standin(monkeypatch):
    from krr_amd.core import engine

    monkeypatch.setattr(engine.SimpleEngine, "run_packed", standin_run_packed)


@pytest.mark.parametrize("mode", ["ref_index", "sorted_lower"])
@pytest.mark.parametrize("fixture", list(COUNTS))
def test_strategy_equals_max_of_per_pod_proposals(standin, fixture, mode):
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.strategies.simple import PercentileMode, SimpleStrategy, SimpleStrategySettings

    cases = load(fixture)
    kept, left_out, multi = split_cases(cases)
    n_cases, n_out, n_multi = COUNTS[fixture]
    assert len(cases) == n_cases and left_out == n_out and multi >= n_multi
    kw = dict(percentile_mode=PercentileMode(mode))
    concat = SimpleStrategy(SimpleStrategySettings(**kw))
    pods_max = SimpleStrategy(SimpleStrategySettings(cpu_aggregation="pods_max", **kw))
    # as one batch per strategy (the MI355X test calls calculate_cpu_proposal pod by pod); a NaN
    # among the MEMORY samples makes max() raise in either aggregation: those run one by one
    mem_nan = [any(Decimal(s).is_nan() for v in c["mem"].values() for s in v) for c in kept]
    for c in (c for c, bad in zip(kept, mem_nan) if bad):
        try:
            concat.run_batch([hist(c)], [obj(c["name"])])
        except decimal.InvalidOperation:
            with pytest.raises(decimal.InvalidOperation):
                pods_max.run_batch([hist(c)], [obj(c["name"])])
    kept = [c for c, bad in zip(kept, mem_nan) if not bad]
    hs = [hist(c) for c in kept]
    objs = [obj(c["name"]) for c in kept]
    got, flat = pods_max.run_batch(hs, objs), concat.run_batch(hs, objs)
    singles = [{ResourceType.CPU: {pod: samples}, ResourceType.Memory: {}}
               for h in hs for pod, samples in h[ResourceType.CPU].items() if samples]
    per_pod = iter(concat.run_batch(singles, [obj("pod")] * len(singles)))
    for c, h, r, f in zip(kept, hs, got, flat):
        mine = [next(per_pod)[ResourceType.CPU].request for samples in h[ResourceType.CPU].values() if samples]
        want = max(mine) if mine else Decimal("NaN")
        assert same_decimal(r[ResourceType.CPU].request, want), (c["name"], r[ResourceType.CPU].request, want)
        assert same_decimal(r[ResourceType.Memory].request, f[ResourceType.Memory].request), c["name"]


def test_runner_rounds_the_per_object_results(standin):
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import SimpleStrategy, SimpleStrategySettings

    strat = SimpleStrategy(SimpleStrategySettings(cpu_aggregation="pods_max"))
    hs = three_objects()
    objs = [obj(f"o{i}") for i in range(3)]
    got = BatchedRunner(strat, 5, 10).recommend(objs, hs)
    want = [format_result(r, 5, 10) for r in strat.run_batch(hs, objs)]
    flat = SimpleStrategy(SimpleStrategySettings()).run_batch(hs, objs)
    for g, w in zip(got, want):
        for res in (ResourceType.CPU, ResourceType.Memory):
            assert str(g[res].request) == str(w[res].request) and str(g[res].limit) == str(w[res].limit)
    assert strat.run_batch(hs, objs)[0][ResourceType.CPU].request > flat[0][ResourceType.CPU].request


def test_integration_install_switch(standin, monkeypatch):
    """install(cpu_aggregation="pods_max") on a reference-shaped Runner with the HistoryData
    loader: the allocations of BatchedRunner over the pods_max strategy."""
    import asyncio
    import sys

    from krr_amd import integration
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import SimpleStrategy, SimpleStrategySettings
    from test_gpu_exact import Runner, _stand_in_reference_strategy

    mod, ref_strategy = _stand_in_reference_strategy("cli_99_5")
    monkeypatch.setitem(sys.modules, "robusta_krr.strategies.simple", mod)
    kept, _, _ = split_cases(load("simple_strategy_exact.json"))
    cases = [c for c in kept if not any(Decimal(s).is_nan() for v in c["mem"].values() for s in v)]
    objects = [obj(f"app-{i:03d}") for i in range(len(cases))]
    with pytest.raises(ValueError):
        integration.install(Runner, cpu_aggregation="pods_mean")
    integration.install(Runner, cpu_aggregation="pods_max")
    try:
        assert integration.hip_strategy(ref_strategy, "pods_max").settings.aggregation() == "pods_max"
        assert integration.hip_strategy(ref_strategy).settings.aggregation() == "concat"
        got = asyncio.run(Runner(ref_strategy, cases, 5, 10)._gather_objects_recommendations(objects))
    finally:
        integration.uninstall(Runner)
    strat = SimpleStrategy(SimpleStrategySettings(cpu_percentile="99", memory_buffer_percentage="5",
                                                  cpu_aggregation="pods_max"))
    want = BatchedRunner(strat, 5, 10).allocations(objects, [hist(c) for c in cases])
    flat = BatchedRunner(SimpleStrategy(SimpleStrategySettings(cpu_percentile="99", memory_buffer_percentage="5")),
                         5, 10).allocations(objects, [hist(c) for c in cases])
    assert len(got) == len(cases) >= 30
    for g, w in zip(got, want):
        assert str(g.requests[ResourceType.CPU]) == str(w.requests[ResourceType.CPU])
        assert str(g.requests[ResourceType.Memory]) == str(w.requests[ResourceType.Memory])
    assert any(str(w.requests[ResourceType.CPU]) != str(f.requests[ResourceType.CPU]) for w, f in zip(want, flat))

"""simple_limit under cpu_aggregation = "pods_max" above the engine, without a GPU: the settings,
the strategy's dispatch, the pod-level exact path per percentile (krr_amd.core.exact.resolve_pods)
and the runner, with ``SimpleEngine.run_packed_multi`` stood in for by the CPU oracle over the pod
segments and the fold by its numpy restatement with P rows (test_gpu_group_max.fold).
tests/test_gpu_pods_multi.py runs the same golden check on the MI355X."""
import dataclasses

import numpy as np
import pytest

from _standin import oracle_run_packed
from test_gpu_group_max import fold
from test_gpu_pods_max import COUNTS, MODES
from test_gpu_pods_multi import PAIRS, golden_check, runner_check


def standin_run_packed_multi(self, fleet, params_list, aggregation="concat", return_pods=False):
    """SimpleEngine.run_packed_multi: one flat stand-in per percentile, or for "pods_max" the
    oracle over the pod segments per percentile, ONE fold of the P rows, and krr_locate's answers
    over the pod segments per percentile."""
    from krr_amd.core.packing import PackedFleet, pod_view

    if aggregation != "pods_max":
        return [oracle_run_packed(self, fleet, params) for params in params_list]
    view = pod_view(fleet.cpu)
    plain_mem = dataclasses.replace(fleet.mem, exact=None, sources=None)
    pod_raws = [oracle_run_packed(self, PackedFleet(view, plain_mem), params) for params in params_list]
    plain_cpu = dataclasses.replace(fleet.cpu, exact=None, sources=None)
    wv, wn, wf, wa = fold(np.asarray(fleet.cpu.pod_groups), np.stack([r.cpu_value for r in pod_raws]),
                          pod_raws[0].cpu_count, np.stack([r.cpu_flags for r in pod_raws]))
    raws = []
    for j, (params, pod_raw) in enumerate(zip(params_list, pod_raws)):
        raw = oracle_run_packed(self, PackedFleet(plain_cpu, fleet.mem), params)  # the memory half and its locate
        raw.cpu_value, raw.cpu_count, raw.cpu_flags = wv[j].view(np.float64), wn, wf[j]
        if return_pods:
            raw.pods = {"pod_value": pod_raw.cpu_value, "pod_count": pod_raw.cpu_count,
                        "pod_flags": pod_raw.cpu_flags, "cpu_pod": wa[j],
                        "locate": {"cpu": pod_raw.locate["cpu"]} if (pod_raw.locate or {}).get("cpu") else None}
        raws.append(raw)
    return raws


@pytest.fixture()
def standin(monkeypatch):
    from krr_amd.core import engine

    monkeypatch.setattr(engine.SimpleEngine, "run_packed_multi", standin_run_packed_multi)
    monkeypatch.setattr(engine.SimpleEngine, "run_packed", oracle_run_packed)
    monkeypatch.setattr(engine.SimpleEngine, "context", lambda self: None)


@pytest.mark.parametrize("pair", PAIRS, ids="-".join)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fixture", list(COUNTS))
def test_strategy_equals_max_of_per_pod_proposals(standin, fixture, mode, pair):
    golden_check(fixture, mode, pair)


@pytest.mark.parametrize("mode", MODES)
def test_runner_and_three_objects(standin, mode):
    runner_check(mode)


def test_settings():
    import pydantic.v1 as pd

    from krr_amd.core.models.config import Config
    from krr_amd.strategies.simple import CpuAggregation
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings as S

    s = S(cpu_aggregation="pods_max")
    assert s.cpu_aggregation is CpuAggregation.PODS_MAX  # the field is kept
    assert s.simple_settings().aggregation() == "pods_max"
    assert S().cpu_aggregation is CpuAggregation.CONCAT and S().simple_settings().aggregation() == "concat"
    with pytest.raises(pd.ValidationError):
        S(cpu_aggregation="pods_mean")
    strat = Config(strategy="simple_limit", other_args={"cpu_aggregation": "pods_max", "cpu_limit": "99"}).create_strategy()
    assert type(strat) is SimpleLimitStrategy
    assert strat.settings.cpu_aggregation is CpuAggregation.PODS_MAX and str(strat.settings.cpu_limit) == "99"
    assert Config(strategy="simple_limit").create_strategy().settings.cpu_aggregation is CpuAggregation.CONCAT


@pytest.mark.parametrize("aggregation", ["concat", "pods_max"])
def test_sharded_entry_points_refuse(aggregation):
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings
    from test_gpu_pods_max import three_objects

    strat = SimpleLimitStrategy(SimpleLimitStrategySettings(cpu_aggregation=aggregation))
    runner = BatchedRunner(strat)
    fleet = strat.pack(three_objects())
    for call in (lambda: runner.recommend_shard(fleet), lambda: runner.recommend_packed_sharded(fleet),
                 lambda: runner.recommend_bodies_shard([[b"{}"]], [[b"{}"]]),
                 lambda: strat.settings.run_fleet_records(fleet), lambda: strat.format_raw(None, 5, 10)):
        with pytest.raises(NotImplementedError, match="one CPU value"):
            call()


def test_engine_refusals(monkeypatch):
    """The engine's own checks come before it touches the device: a CPU series without pod
    boundaries, and an aggregation it does not know."""
    from krr_amd.core import engine
    from krr_amd.core.packing import PackedFleet, PackedSeries
    from krr_amd.strategies.simple_limit import SimpleLimitStrategySettings

    monkeypatch.setattr(engine.SimpleEngine, "context", lambda self: None)
    offs = np.array([0, 3], dtype=np.int64)
    fleet = PackedFleet(PackedSeries(np.array([1.0, 2.0, 3.0]), offs, 3), PackedSeries(np.array([1.0, 2.0, 3.0]), offs, 3))
    with pytest.raises(ValueError, match="device packer"):
        SimpleLimitStrategySettings(cpu_aggregation="pods_max").run_fleet_multi(fleet)
    params = SimpleLimitStrategySettings().params_list()
    with pytest.raises(ValueError, match="unknown cpu aggregation 'pods_mean'"):
        engine.SimpleEngine(0).run_packed_multi(fleet, params, aggregation="pods_mean")


def test_abi():
    from krr_amd import _native

    assert "krr_simple_run_pods_multi" in _native.EXPORTED_SYMBOLS
    lib = _native.load_library()
    assert lib.krr_abi_version() == 3
    assert lib.krr_simple_run_pods_multi(None, None, None, None, None, 2, None, None, None, None, None, None, None,
                                         None, None, None, None) == -1

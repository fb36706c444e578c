"""simple_limit above the kernels (no GPU: the engine stood in for by the CPU oracle, one
oracle.percentile call per percentile): settings, registry, every fixture row through run /
run_batch / BatchedRunner, and the sharded entry points' refusal."""
import os
import sys
from decimal import Decimal

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _limit_cases as lc  # noqa: E402
import _standin_multi  # noqa: E402


@pytest.fixture
def standin(monkeypatch):
    _standin_multi.install(monkeypatch)


def test_registry_finds_simple_limit():
    from krr_amd.core.abstract.strategies import BaseStrategy
    from krr_amd.core.models.config import Config
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    assert BaseStrategy.find("simple_limit") is SimpleLimitStrategy
    assert BaseStrategy.find("Simple_Limit") is SimpleLimitStrategy
    assert SimpleLimitStrategy.get_settings_type() is SimpleLimitStrategySettings
    assert set(BaseStrategy.get_all()) >= {"simple", "simple_limit"}
    strat = Config(strategy="simple_limit").create_strategy()
    assert type(strat) is SimpleLimitStrategy and SimpleLimitStrategy.__bases__[0].__name__ == "BaseStrategy"
    st = strat.settings
    assert (st.cpu_request, st.cpu_limit, st.memory_buffer_percentage) == (66, 96, 5)
    assert st.percentile_mode.value == "sorted_lower" and st.device == 0


def test_settings_validation():
    import pydantic.v1 as pd

    from krr_amd.strategies.simple_limit import SimpleLimitStrategySettings as S

    with pytest.raises(pd.ValidationError, match="cpu_limit must be at least cpu_request"):
        S(cpu_request=96, cpu_limit=66)
    with pytest.raises(pd.ValidationError, match="cpu_limit must be at least cpu_request"):
        S(cpu_request="97")  # above the default limit
    with pytest.raises(pd.ValidationError, match="cpu_limit must be at least cpu_request"):
        S(cpu_limit=Decimal("65.9"))  # below the default request
    for bad in (dict(cpu_request=0), dict(cpu_limit=Decimal("100.1")), dict(cpu_request=-1),
                dict(memory_buffer_percentage=0), dict(device=-1), dict(percentile_mode="median")):
        with pytest.raises(pd.ValidationError):
            S(**bad)
    s = S(cpu_request="99", cpu_limit="99")  # equal is allowed
    assert s.cpu_request == s.cpu_limit == Decimal("99")
    assert [p.mode for p in s.params_list()] == [1, 1]


@pytest.mark.parametrize("path", lc.PATHS)
@pytest.mark.parametrize("pair", lc.PAIRS, ids=lambda p: f"{p[0][:6]}-{p[1][:6]}")
@pytest.mark.parametrize("mode", ["ref_index", "sorted_lower"])
def test_fixture_rows(standin, mode, pair, path):
    lc.check_exact_modes(pair, path, mode)


@pytest.mark.parametrize("path", lc.PATHS)
@pytest.mark.parametrize("pair", lc.PAIRS, ids=lambda p: f"{p[0][:6]}-{p[1][:6]}")
def test_fixture_rows_linear(standin, pair, path):
    lc.check_linear(pair, path)


def test_sorted_limit_is_never_below_the_request(standin):
    from krr_amd.core.models.allocations import ResourceType

    strat = lc.strategy(("66", "96"), "direct", "sorted_lower")
    cases = [c for c in lc.DOC["cases"] if lc.expected(c, ("66", "96"), "direct", "sorted_lower")[2] is None]
    seen = 0
    for r in strat.run_batch([lc.hist(c) for c in cases]):
        cpu = r[ResourceType.CPU]
        if not cpu.request.is_nan():
            assert cpu.limit >= cpu.request
            seen += cpu.limit > cpu.request
    assert seen >= 5


def test_recommend_packed_and_result_packed(standin):
    from krr_amd.core.runner import BatchedRunner

    strat = lc.strategy(("95", "99"), "cli", "sorted_lower")
    cases = [c for c in lc.DOC["cases"] if (lc.expected(c, ("95", "99"), "cli", "sorted_lower")[1] is not None)]
    objs, hs = [lc.obj(c["name"]) for c in cases], [lc.hist(c) for c in cases]
    runner = BatchedRunner(strat)
    fleet = strat.pack(hs)
    want = [lc.rows(r) for r in runner.recommend(objs, hs)]
    assert [lc.rows(r) for r in runner.recommend_packed(fleet)] == want
    assert any(w["cpu_limit"] not in (None, w["cpu_request"]) for w in want)
    al = runner.allocations_packed(fleet)
    assert [a.dict() for a in al] == [a.dict() for a in runner.allocations(objs, hs)]
    assert runner.result_packed(objs, fleet).dict() == runner.collect_result(objs, hs).dict()


def test_other_strategies_keep_their_path(standin):
    """``simple`` has no packed hook: its CPU limit stays None through every runner method."""
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import SimpleStrategy, SimpleStrategySettings

    runner = BatchedRunner(SimpleStrategy(SimpleStrategySettings()))
    assert runner._packed_hook() is None
    cases = [c for c in lc.DOC["cases"] if c["name"] in ("one_sample", "ties", "random_0")]
    objs, hs = [lc.obj(c["name"]) for c in cases], [lc.hist(c) for c in cases]
    assert all(a.limits[ResourceType.CPU] is None for a in runner.allocations(objs, hs))
    assert all(r[ResourceType.CPU].limit is None for r in runner.recommend(objs, hs))


def test_sharded_entry_points_refuse():
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    strat = SimpleLimitStrategy(SimpleLimitStrategySettings())
    runner = BatchedRunner(strat)
    fleet = strat.pack([lc.hist(lc.DOC["cases"][1])])
    for call in (lambda: runner.recommend_shard(fleet), lambda: runner.recommend_packed_sharded(fleet),
                 lambda: runner.recommend_bodies_shard([[b"{}"]], [[b"{}"]]),
                 lambda: strat.settings.run_fleet_records(fleet)):
        with pytest.raises(NotImplementedError, match="one CPU value"):
            call()

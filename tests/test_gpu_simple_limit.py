"""simple_limit on the MI355X: the fixture rows of tests/golden/simple_limit.json through
SimpleLimitStrategy and BatchedRunner (the checks of test_simple_limit.py, with the real
engine), raw query_range bodies, and a chunked engine run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _limit_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", lc.PATHS)
@pytest.mark.parametrize("mode", ["ref_index", "sorted_lower"])
def test_gpu_fixture_rows(mode, path):
    for pair in lc.PAIRS:
        lc.check_exact_modes(pair, path, mode)


@pytest.mark.parametrize("path", lc.PATHS)
def test_gpu_fixture_rows_linear(path):
    for pair in lc.PAIRS:
        lc.check_linear(pair, path)


def _body(xs):
    vals = ",".join(f'[{1700000000 + 60 * i},"{float(x)!r}"]' for i, x in enumerate(xs))
    return ('{"status":"success","data":{"resultType":"matrix","result":[{"metric":{},"values":[' + vals +
            ']}]}}').encode()


@pytest.mark.parametrize("parser", ["device", "host"])
def test_gpu_recommend_from_bodies_equals_recommend(parser):
    from decimal import Decimal

    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.runner import BatchedRunner

    rng = np.random.default_rng(41)
    strat = lc.strategy(("66", "96"), "direct", "sorted_lower")
    cpu_pods = [[np.round(rng.gamma(2.0, 0.05, int(n)), 5) for n in rng.integers(1, 400, int(k))]
                for k in (1, 3, 2, 1, 4, 2)]
    mem_pods = [[np.floor(rng.normal(2e8, 2e7, int(n))) for n in rng.integers(1, 300, len(pods))] for pods in cpu_pods]
    cpu_bodies = [[_body(p) for p in pods] for pods in cpu_pods]
    mem_bodies = [[_body(p) for p in pods] for pods in mem_pods]
    hs = [{ResourceType.CPU: {f"p{i}": [Decimal(repr(float(x))) for x in p] for i, p in enumerate(cp)},
           ResourceType.Memory: {f"p{i}": [Decimal(repr(float(x))) for x in p] for i, p in enumerate(mp)}}
          for cp, mp in zip(cpu_pods, mem_pods)]
    runner = BatchedRunner(strat)
    want = [lc.rows(r) for r in runner.recommend([lc.obj(f"o{i}") for i in range(len(hs))], hs)]
    got = [lc.rows(r) for r in runner.recommend_from_bodies(cpu_bodies, mem_bodies, parser=parser)]
    assert got == want
    assert all(w["cpu_limit"] is not None for w in want)
    assert sum(Decimal(w["cpu_limit"]) > Decimal(w["cpu_request"]) for w in want) >= 4


def test_gpu_chunked_engine_run_equals_unchunked():
    from krr_amd.core.engine import SimpleEngine, percentile_params
    from krr_amd.core.packing import PackedFleet, PackedSeries

    rng = np.random.default_rng(43)
    lens = rng.integers(0, 3000, 60)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cpu = np.round(rng.gamma(2.0, 0.05, int(offs[-1])), 4)
    mem = np.floor(rng.normal(2e8, 2e7, cpu.size))
    fleet = PackedFleet(PackedSeries(cpu, offs, int(lens.max())), PackedSeries(mem, offs, int(lens.max())))
    plist = [percentile_params(p, "sorted_lower") for p in (66, 96, 99)]
    whole = SimpleEngine(0).run_packed_multi(fleet, plist)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 8 * int(offs[-1]) // 3  # both resources hold 16 B per slot: about six chunks
    assert len(eng._chunk_bounds(fleet)) >= 4
    parts = eng.run_packed_multi(fleet, plist)
    assert len(whole) == len(parts) == 3
    for a, b in zip(whole, parts):
        for f in ("cpu_value", "cpu_count", "cpu_flags", "mem_value", "mem_count", "mem_flags"):
            x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
            assert np.array_equal(x, y, equal_nan=x.dtype == np.float64), f
    assert not np.array_equal(whole[0].cpu_value, whole[2].cpu_value, equal_nan=True)
    # and the single-percentile engine path agrees per percentile
    for j, prm in enumerate(plist):
        one = SimpleEngine(0).run_packed(fleet, prm)
        assert np.array_equal(one.cpu_value, whole[j].cpu_value, equal_nan=True)
        assert np.array_equal(one.mem_value, whole[j].mem_value, equal_nan=True)

"""TEST INFRASTRUCTURE shared by test_simple_limit.py (CPU, oracle stand-in) and
test_gpu_simple_limit.py: tests/golden/simple_limit.json's rows through SimpleLimitStrategy and
BatchedRunner, string for string against what the reference gives per percentile."""
from __future__ import annotations

import decimal
import json
import math
import os
from decimal import Decimal

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "simple_limit.json")) as fh:
    DOC = json.load(fh)

PAIRS = [tuple(p) for p in DOC["pairs"]]
PATHS = list(DOC["paths"])
MODES = ["ref_index", "sorted_lower", "linear"]
MODE_KEY = {"ref_index": "ref_index", "sorted_lower": "sorted"}


def hist(case):
    from krr_amd.core.models.allocations import ResourceType

    return {ResourceType.CPU: {k: [Decimal(s) for s in v] for k, v in case["cpu"].items() if v},
            ResourceType.Memory: {k: [Decimal(s) for s in v] for k, v in case["mem"].items() if v}}


def obj(name):
    from krr_amd.api.models import K8sObjectData, ResourceAllocations
    from krr_amd.core.models.allocations import ResourceType

    cur = {ResourceType.CPU: Decimal("0.1"), ResourceType.Memory: Decimal("100000000")}
    return K8sObjectData(cluster=None, name=name, container="c", pods=["p"], namespace="ns", kind="Deployment",
                         allocations=ResourceAllocations(requests=dict(cur), limits=dict(cur)))


def d(x):
    return None if x is None else str(x)


def rows(res):
    from krr_amd.core.models.allocations import ResourceType

    return {"cpu_request": d(res[ResourceType.CPU].request), "cpu_limit": d(res[ResourceType.CPU].limit),
            "mem_request": d(res[ResourceType.Memory].request), "mem_limit": d(res[ResourceType.Memory].limit)}


def strategy(pair, path, mode):
    """The strategy as each settings path builds it: the CLI's strings through Config.other_args,
    or direct construction with ints (a Decimal where the percentile is no integer)."""
    from krr_amd.core.models.config import Config
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    pr, pl = pair
    if path == "cli":
        cfg = Config(strategy="simple_limit", other_args={"cpu_request": pr, "cpu_limit": pl,
                                                          "memory_buffer_percentage": "5", "percentile_mode": mode})
        strat = cfg.create_strategy()
        assert type(strat) is SimpleLimitStrategy
        return strat
    conv = [int(p) if p.isdigit() else Decimal(p) for p in (pr, pl)]
    return SimpleLimitStrategy(SimpleLimitStrategySettings(cpu_request=conv[0], cpu_limit=conv[1],
                                                           percentile_mode=mode))


def _is_err(x):
    return isinstance(x, dict)


def expected(case, pair, path, mode):
    """(raw rows or None, rounded rows incl. 'alloc' or None, exception name or None) the fixture
    holds for a sorted / ref_index run; None for linear (checked by value, see check_linear)."""
    want = case["results"][f"{pair[0]}|{pair[1]}|{path}"]
    key = MODE_KEY[mode]
    vals, mem = want[key], want["mem"]
    for x in vals + [mem]:
        if _is_err(x):
            return None, None, x["error"]
    raw = {"cpu_request": vals[0], "cpu_limit": vals[1], "mem_request": mem, "mem_limit": mem}
    rd = want["rounded"][key]
    return raw, (None if "rounded_error" in rd else rd), None


def check_exact_modes(pair, path, mode):
    """run, run_batch, BatchedRunner.recommend / allocations / collect_result over every fixture
    case of a sorted_lower / ref_index setting."""
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner

    strat = strategy(pair, path, mode)
    good, rounded = [], []
    for c in DOC["cases"]:
        raw, rd, err = expected(c, pair, path, mode)
        if err:
            with pytest.raises(getattr(decimal, err)):
                strat.run(hist(c), obj(c["name"]))
            continue
        good.append((c, raw, rd))
        assert rows(strat.run(hist(c), obj(c["name"]))) == raw, (c["name"], pair, path, mode)
    assert len(good) >= 15
    got = strat.run_batch([hist(c) for c, _, _ in good], [obj(c["name"]) for c, _, _ in good])
    for (c, raw, rd), r in zip(good, got):
        assert rows(r) == raw, (c["name"], pair, path, mode)
        if rd is not None:
            want = {k: v for k, v in rd.items() if k != "alloc"}
            assert rows(format_result(r, 5, 10)) == want, c["name"]
            rounded.append((c, rd))
    runner = BatchedRunner(strat)
    objs, hs = [obj(c["name"]) for c, _ in rounded], [hist(c) for c, _ in rounded]
    rec = runner.recommend(objs, hs)
    al = runner.allocations(objs, hs)
    assert len(rec) == len(al) == len(rounded)
    for (c, rd), r, a in zip(rounded, rec, al):
        assert rows(r) == {k: v for k, v in rd.items() if k != "alloc"}, c["name"]
        for rt in ResourceType:
            assert d(a.requests[rt]) == rd["alloc"]["requests"][rt.value], (c["name"], rt)
            assert d(a.limits[rt]) == rd["alloc"]["limits"][rt.value], (c["name"], rt)
    res = runner.collect_result(objs, hs)
    assert len(res.scans) == len(rounded)
    for (c, rd), scan in zip(rounded, res.scans):
        assert d(scan.recommended.limits[ResourceType.CPU].value) == rd["alloc"]["limits"]["cpu"], c["name"]
        assert d(scan.recommended.requests[ResourceType.CPU].value) == rd["alloc"]["requests"]["cpu"], c["name"]


def check_linear(pair, path):
    """linear: both CPU values equal numpy's float64 (the Decimal of its shortest repr), the memory
    the reference's."""
    from krr_amd.core.models.allocations import ResourceType

    strat = strategy(pair, path, "linear")
    cases = [c for c in DOC["cases"]
             if not _is_err(c["results"][f"{pair[0]}|{pair[1]}|{path}"]["mem"])]
    got = strat.run_batch([hist(c) for c in cases], [obj(c["name"]) for c in cases])
    n = 0
    for c, r in zip(cases, got):
        want = c["results"][f"{pair[0]}|{pair[1]}|{path}"]
        assert d(r[ResourceType.Memory].request) == want["mem"], c["name"]
        cpu = r[ResourceType.CPU]
        if "linear_hex" not in want:
            assert cpu.request.is_nan() and cpu.limit.is_nan(), c["name"]
            continue
        for v, hx in zip((cpu.request, cpu.limit), want["linear_hex"]):
            if hx == "nan":
                assert v.is_nan(), c["name"]
            else:
                assert float(v) == float.fromhex(hx) and not math.isnan(float(v)), (c["name"], v, hx)
            n += 1
        one = strat.run(hist(c), obj(c["name"]))
        assert rows(one) == rows(r), c["name"]
    assert n >= 30
    # BatchedRunner.recommend / allocations: the reference's rounding of those same values
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner, to_allocations

    keep, want = [], []
    for c, r in zip(cases, got):
        try:
            want.append(format_result(r, 5, 10))
            keep.append(c)
        except (decimal.DecimalException, OverflowError, ValueError):  # ceil(Infinity / NaN), as the reference
            continue
    assert len(keep) >= 15
    runner = BatchedRunner(strat)
    objs, hs = [obj(c["name"]) for c in keep], [hist(c) for c in keep]
    assert [rows(r) for r in runner.recommend(objs, hs)] == [rows(w) for w in want]
    assert [a.dict() for a in runner.allocations(objs, hs)] == [to_allocations(w).dict() for w in want]

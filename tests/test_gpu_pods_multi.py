"""simple_limit under cpu_aggregation = "pods_max" on the MI355X: krr_simple_run_pods_multi row by
row, bit for bit, against krr_simple_run_pods with that row's percentile alone and against
oracle.percentile over the pod CSR folded by the numpy restatement of krr_group_max
(test_gpu_group_max.fold, P rows) plus oracle.seg_max; then the engine's chunks and the strategy
against the Python max() of the flat strategy's own per-pod proposals.  Outputs are pre-filled
with sentinels, so an unwritten slot is seen; the shared cases assert ``multi_plan(...).shared``
so that none passes by falling back to the per-percentile launches."""
import decimal
from decimal import Decimal

import numpy as np
import pytest

from test_gpu_group_max import fold
from test_gpu_multi_pct import BIG
from test_gpu_pods_max import (COUNTS, MODES, hist, load, make_fleet, obj, oracle_pods, run_pods, same_decimal,
                               split_cases, three_objects)

pytestmark = pytest.mark.gpu

SETS = [(95, 99), (90, 95, 99, 100), (BIG, 99), (66, 96)]
SENTINELS = {"cpu_value": -777.0, "cpu_count": -7, "cpu_flags": -1, "cpu_pod": -99, "mem_value": -777.0,
             "mem_count": -7, "mem_flags": -1, "pod_value": -777.0, "pod_count": -7, "pod_flags": -1}


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


def params_of(ps, mode):
    from krr_amd.core.engine import percentile_params

    return [percentile_params(Decimal(str(p)), mode) for p in ps]


def fleet_of(pod_lens, per_object, seed, gaps):
    """make_fleet's arrays for given pod lengths and pods per object."""
    rng = np.random.default_rng(seed)
    pod_offs = np.concatenate([[0], np.cumsum(pod_lens)]).astype(np.int64)
    groups = np.concatenate([[0], np.cumsum(per_object)]).astype(np.int64)
    x = np.round(rng.gamma(2.0, 0.05, int(pod_offs[-1])), 3) + 0.001
    if gaps:
        x[rng.random(x.size) < 0.1] = np.nan
    mem_offs = np.concatenate([[0], np.cumsum(rng.integers(0, 500, len(per_object)))]).astype(np.int64)
    mem = np.floor(rng.normal(2e8, 2e7, int(mem_offs[-1])))
    return x, pod_offs, groups, pod_offs[groups], mem, mem_offs


def run_multi(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist, n_rows=None, slack=0):
    """krr_simple_run_pods_multi into sentinel-filled outputs of ``n_rows`` rows (default
    len(plist)) and ``slack`` more elements per row than the fleet needs."""
    import torch

    ctx, dev = gpu
    S, n_pods = groups.size - 1, pod_offs.size - 1
    P = len(plist) if n_rows is None else n_rows
    pcs = ctx.series(torch.from_numpy(x).to(dev), torch.from_numpy(pod_offs).to(dev),
                     max(int(np.diff(pod_offs).max(initial=0)), 1), gaps)
    ms = ctx.series(torch.from_numpy(mem).to(dev), torch.from_numpy(mem_offs).to(dev),
                    max(int(np.diff(mem_offs).max(initial=0)), 1), gaps)
    out = {}
    for k, dt, rows, n in (("cpu_value", torch.float64, P, S), ("cpu_count", torch.int64, 0, S),
                           ("cpu_flags", torch.int32, P, S), ("cpu_pod", torch.int64, P, S),
                           ("mem_value", torch.float64, 0, S), ("mem_count", torch.int64, 0, S),
                           ("mem_flags", torch.int32, 0, S), ("pod_value", torch.float64, P, n_pods),
                           ("pod_count", torch.int64, 0, n_pods), ("pod_flags", torch.int32, P, n_pods)):
        out[k] = torch.full((rows, n + slack) if rows else (n + slack,), SENTINELS[k], dtype=dt, device=dev)
    try:
        ctx.simple_run_pods_multi(pcs, torch.from_numpy(groups).to(dev), ms, plist, out)
    finally:
        torch.cuda.synchronize()
        run_multi.last = {k: t.cpu().numpy() for k, t in out.items()}
    return run_multi.last


def untouched(host):
    return all((a == SENTINELS[k]).all() for k, a in host.items())


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check_rows(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist, tag):
    """Every row against the single launch for its percentile and against the references."""
    from oracle import oracle

    host = run_multi(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist)
    pods = [oracle_pods(x, pod_offs, prm, gaps) for prm in plist]
    pv = np.stack([p[0] for p in pods])
    pf = np.stack([p[2].astype(np.uint32) for p in pods])
    wv, wn, wf, wa = fold(groups, pv, pods[0][1], pf)
    for j, prm in enumerate(plist):
        one, _ = run_pods(gpu, x, pod_offs, groups, mem, mem_offs, gaps, prm, records=False)
        for k in ("pod_value", "pod_flags", "cpu_value", "cpu_flags", "cpu_pod"):
            assert np.array_equal(bits(host[k][j]), bits(one[k])), (tag, j, k)
        for k in ("pod_count", "cpu_count", "mem_value", "mem_count", "mem_flags"):
            assert np.array_equal(bits(host[k]), bits(one[k])), (tag, j, k)
        assert np.array_equal(host["pod_value"][j].view(np.uint64), pv[j].view(np.uint64)), (tag, j)
        assert np.array_equal(host["pod_flags"][j].view(np.uint32), pf[j]), (tag, j)
        assert np.array_equal(host["cpu_value"][j].view(np.uint64), wv[j]), (tag, j)
        assert np.array_equal(host["cpu_flags"][j].view(np.uint32), wf[j]), (tag, j)
        assert np.array_equal(host["cpu_pod"][j], wa[j]), (tag, j)
    assert np.array_equal(host["pod_count"], pods[0][1]) and np.array_equal(host["cpu_count"], wn), tag
    mv, mn, mf = oracle.seg_max(mem, mem_offs, gaps)
    assert np.array_equal(host["mem_value"].view(np.uint64), mv.view(np.uint64)), tag
    assert np.array_equal(host["mem_count"], mn), tag
    assert np.array_equal(host["mem_flags"].view(np.uint32), mf.astype(np.uint32)), tag
    return host


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_rows_equal_the_single_launches(gpu, mode, gaps):
    from krr_amd import _native

    x, pod_offs, groups, _, mem, mem_offs = make_fleet(53, gaps)
    assert int(np.diff(pod_offs).max()) == 5000
    for ps in SETS:
        plist = params_of(ps, mode)
        shared = 0 if ps == (66, 96) and mode != "ref_index" else 1
        assert _native.multi_plan(5000, plist).shared == shared, (mode, ps)
        host = check_rows(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist, (mode, gaps, ps))
        # the rows differ somewhere (else one answer copied P times would pass), a later pod
        # wins somewhere and an object is without pods
        assert (host["cpu_value"][0].view(np.uint64) != host["cpu_value"][-1].view(np.uint64)).any()
        assert (host["cpu_pod"] > 0).any() and (host["cpu_pod"] == -1).any()


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_planned_by_the_pod_length(gpu, mode, gaps):
    """5 pods x 2,000 slots: {80, 99} shares one pass at the pod length and would not at the
    length of the object's concatenated series."""
    from krr_amd import _native

    plist = params_of((80, 99), mode)
    assert _native.multi_plan(2000, plist).shared == 1 and _native.multi_plan(10000, plist).shared == 0
    fleet = fleet_of([2000] * 30, [5] * 6, 59, gaps)
    x, pod_offs, groups, obj_offs, mem, mem_offs = fleet
    assert int(np.diff(pod_offs).max()) == 2000 and int(np.diff(obj_offs).max()) == 10000
    check_rows(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist, (mode, gaps))


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_fallback_with_a_long_pod(gpu, mode, gaps):
    from krr_amd import _native

    plist = params_of((50, 99), mode)
    assert _native.multi_plan(70000, plist).shared == 0
    x, pod_offs, groups, _, mem, mem_offs = make_fleet(61, gaps, extra_pod_len=70000)
    check_rows(gpu, x, pod_offs, groups, mem, mem_offs, gaps, plist, (mode, gaps))


@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_different_winners_per_row(gpu, mode):
    """Pod A steady (high p66, modest p96), pod B spiky (low p66, high p96): the request's
    winner is A, the limit's B, each row carrying that pod's own value."""
    x, pod_offs, groups, _, mem, mem_offs = fleet_of([50, 100, 100, 7], [1, 2, 1], 67, False)
    x[50:150] = 0.5
    x[150:240] = 0.1
    x[240:250] = 2.0
    host = check_rows(gpu, x, pod_offs, groups, mem, mem_offs, False, params_of((66, 96), mode), mode)
    assert host["cpu_pod"][0][1] == 0 and host["cpu_pod"][1][1] == 1
    assert host["cpu_value"][0][1] == host["pod_value"][0][1] == 0.5
    assert host["cpu_value"][1][1] == host["pod_value"][1][2] == 2.0
    assert host["pod_value"][0][2] == 0.1 and host["pod_value"][1][1] == 0.5


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_a_wide_group(gpu, mode, gaps):
    """One object of 130 pods of one to three slots: the fold's lanes stride, four rows."""
    rng = np.random.default_rng(71)
    lens = rng.integers(1, 4, 130).tolist()
    x, pod_offs, groups, _, mem, mem_offs = fleet_of(lens + [5, 9], [130, 0, 2], 73, gaps)
    x[pod_offs[100]:pod_offs[101]] = 9.0  # the hottest pod sits in the lanes' second stride
    host = check_rows(gpu, x, pod_offs, groups, mem, mem_offs, gaps, params_of((50, 90, 99, 100), mode), (mode, gaps))
    assert (host["cpu_pod"][:, 0] == 100).all() and (host["cpu_value"][:, 0] == 9.0).all()


def test_degenerate_fleets(gpu):
    plist = params_of((66, 96), "sorted_lower")
    none, zero = np.zeros(0), np.zeros(1, dtype=np.int64)
    # every object without pods: all rows EMPTY, NaN, -1; the memory is still answered
    _, _, _, _, mem, mem_offs = fleet_of([], [0, 0, 0], 79, False)
    host = check_rows(gpu, none, zero, np.zeros(4, dtype=np.int64), mem, mem_offs, False, plist, "no pods")
    assert host["cpu_flags"].shape == (2, 3) and (host["cpu_flags"] == 4).all() and (host["cpu_pod"] == -1).all()
    assert np.isnan(host["cpu_value"]).all() and (host["cpu_count"] == 0).all() and (host["mem_count"] > 0).any()
    # no object: nothing is written
    host = run_multi(gpu, none, zero, zero, none, zero, False, plist, slack=4)
    assert host["cpu_value"].shape == (2, 4) and untouched(host)
    # one percentile: krr_simple_run_pods
    x, pod_offs, groups, _, mem, mem_offs = make_fleet(83, True)
    for mode in MODES:
        check_rows(gpu, x, pod_offs, groups, mem, mem_offs, True, params_of((96,), mode), ("one", mode))


def test_argument_errors(gpu):
    from krr_amd import _native

    x, pod_offs, groups, _, mem, mem_offs = make_fleet(89, False, pods_per_object=np.array([2, 0, 3]))
    bad_groups = groups.copy()
    bad_groups[-1] -= 1  # ends short of the pod segments
    for plist, g in (([], groups), (params_of((50, 90, 95, 99, 100), "linear"), groups),
                     (params_of((95,), "linear") + params_of((99,), "sorted_lower"), groups),
                     (params_of((66, 96), "sorted_lower"), bad_groups)):
        with pytest.raises(_native.NativeError) as e:
            run_multi(gpu, x, pod_offs, g, mem, mem_offs, False, plist, n_rows=5)
        assert e.value.code == _native.KRR_E_INVALID and str(e.value).strip()
        assert untouched(run_multi.last)  # nothing was launched


def packed(x, pod_offs, groups, obj_offs, mem, mem_offs, gaps):
    from krr_amd.core.packing import PackedFleet, PackedSeries

    cpu = PackedSeries(x, obj_offs, int(np.diff(obj_offs).max()), gaps)
    cpu.pod_offsets, cpu.pod_groups = pod_offs, groups
    return PackedFleet(cpu, PackedSeries(mem, mem_offs, int(np.diff(mem_offs).max()), gaps))


@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_chunked_runs_equal_the_whole(gpu, mode):
    from krr_amd.core.engine import SimpleEngine

    x, pod_offs, groups, obj_offs, mem, mem_offs = make_fleet(97, True)
    fleet = packed(x, pod_offs, groups, obj_offs, mem, mem_offs, True)
    plist = params_of((66, 96), mode)
    whole = SimpleEngine(0).run_packed_multi(fleet, plist, aggregation="pods_max", return_pods=True)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 8 * (x.size + mem.size) // 5
    assert len(eng._chunk_bounds(fleet)) >= 3
    parts = eng.run_packed_multi(fleet, plist, aggregation="pods_max", return_pods=True)
    assert len(whole) == len(parts) == 2
    for j, (a, b) in enumerate(zip(whole, parts)):
        for k in ("cpu_value", "cpu_count", "cpu_flags", "mem_value", "mem_count", "mem_flags"):
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), (j, k)
        for k in ("pod_value", "pod_count", "pod_flags", "cpu_pod"):
            assert np.array_equal(bits(a.pods[k]), bits(b.pods[k])), (j, k)
        assert a.pods["pod_count"].size == pod_offs.size - 1 and a.pods["cpu_pod"].size == groups.size - 1
        # and the whole run is the native call's row
        host = run_multi(gpu, x, pod_offs, groups, mem, mem_offs, True, plist)
        assert np.array_equal(bits(a.cpu_value), bits(host["cpu_value"][j]))
        assert np.array_equal(a.pods["cpu_pod"], host["cpu_pod"][j])
        assert np.array_equal(bits(a.pods["pod_value"]), bits(host["pod_value"][j]))
    assert (whole[0].pods["cpu_pod"] != whole[1].pods["cpu_pod"]).any()
    with pytest.raises(ValueError, match="unknown cpu aggregation"):
        eng.run_packed_multi(fleet, plist, aggregation="pods_mean")


# ---------------------------------------------------------------------------------------------
# strategy level
# ---------------------------------------------------------------------------------------------

PAIRS = [("66", "96"), ("95", "99")]


def golden_check(fixture, mode, pair):
    """Request and limit of SimpleLimitStrategy(cpu_aggregation="pods_max") against Python max()
    over the pods of the flat SimpleStrategy's own per-pod proposal at that percentile (the
    reference pins that proposal); memory against the flat strategy's.  Shared with the CPU
    stand-in test (test_pods_limit_standin.py)."""
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.strategies.simple import PercentileMode, SimpleStrategy, SimpleStrategySettings
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    cases = load(fixture)
    kept, left_out, multi = split_cases(cases)
    n_cases, n_out, n_multi = COUNTS[fixture]
    assert len(cases) == n_cases and left_out == n_out and multi >= n_multi
    pm = PercentileMode(mode)
    flats = [SimpleStrategy(SimpleStrategySettings(cpu_percentile=p, percentile_mode=pm)) for p in pair]
    limit = SimpleLimitStrategy(SimpleLimitStrategySettings(cpu_request=pair[0], cpu_limit=pair[1],
                                                            percentile_mode=pm, cpu_aggregation="pods_max"))
    flat_limit = SimpleLimitStrategy(SimpleLimitStrategySettings(cpu_request=pair[0], cpu_limit=pair[1],
                                                                 percentile_mode=pm))
    # a NaN among the MEMORY samples makes max() raise in either aggregation (simple.py:29):
    # those histories run one by one, the others as one batch
    mem_nan = [any(Decimal(s).is_nan() for v in c["mem"].values() for s in v) for c in kept]
    for c in (c for c, bad in zip(kept, mem_nan) if bad):
        try:
            flats[0].run_batch([hist(c)], [obj(c["name"])])
        except decimal.InvalidOperation:
            with pytest.raises(decimal.InvalidOperation):
                limit.run_batch([hist(c)], [obj(c["name"])])
    kept = [c for c, bad in zip(kept, mem_nan) if not bad]
    hs, objs = [hist(c) for c in kept], [obj(c["name"]) for c in kept]
    got, flat, flat_lim = limit.run_batch(hs, objs), flats[0].run_batch(hs, objs), flat_limit.run_batch(hs, objs)
    singles = [{ResourceType.CPU: {pod: samples}, ResourceType.Memory: {}}
               for h in hs for pod, samples in h[ResourceType.CPU].items() if samples]
    per_pod = [iter(f.run_batch(singles, [obj("pod")] * len(singles))) for f in flats]
    differs = 0
    for c, h, r, f, fl in zip(kept, hs, got, flat, flat_lim):
        cpu = r[ResourceType.CPU]
        for which, (mine, it) in enumerate(zip((cpu.request, cpu.limit), per_pod)):
            own = [next(it)[ResourceType.CPU].request for samples in h[ResourceType.CPU].values() if samples]
            want = max(own) if own else Decimal("NaN")
            if mode == "linear":  # defined on the float64 values
                assert float(mine) == float(want) or (mine.is_nan() and want.is_nan()), (c["name"], which, mine, want)
            else:
                assert same_decimal(mine, want), (c["name"], which, mine, want)
        if mode != "ref_index" and not cpu.request.is_nan() and not cpu.limit.is_nan():
            assert cpu.limit >= cpu.request, c["name"]
        assert same_decimal(r[ResourceType.Memory].request, f[ResourceType.Memory].request), c["name"]
        assert same_decimal(r[ResourceType.Memory].limit, f[ResourceType.Memory].limit), c["name"]
        differs += not (same_decimal(cpu.request, fl[ResourceType.CPU].request) and
                        same_decimal(cpu.limit, fl[ResourceType.CPU].limit))
    assert differs > 0  # the two aggregations are different rules on these fixtures


@pytest.mark.parametrize("pair", PAIRS, ids="-".join)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fixture", list(COUNTS))
def test_strategy_equals_max_of_per_pod_proposals(fixture, mode, pair):
    golden_check(fixture, mode, pair)


def runner_check(mode):
    """BatchedRunner over the pods_max strategy rounds run_batch's results; on three_objects()
    the hot second pod of object 0 lifts both CPU values above the flat strategy's."""
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import PercentileMode
    from krr_amd.strategies.simple_limit import SimpleLimitStrategy, SimpleLimitStrategySettings

    pm = PercentileMode(mode)
    strat = SimpleLimitStrategy(SimpleLimitStrategySettings(percentile_mode=pm, cpu_aggregation="pods_max"))
    flat = SimpleLimitStrategy(SimpleLimitStrategySettings(percentile_mode=pm))
    hs = three_objects()
    objs = [obj(f"o{i}") for i in range(3)]
    runner = BatchedRunner(strat, 5, 10)
    res = strat.run_batch(hs, objs)
    want = [format_result(r, 5, 10) for r in res]
    for g, a, w in zip(runner.recommend(objs, hs), runner.allocations(objs, hs), want):
        for rt in (ResourceType.CPU, ResourceType.Memory):
            assert str(g[rt].request) == str(w[rt].request) and str(g[rt].limit) == str(w[rt].limit)
            assert str(a.requests[rt]) == str(w[rt].request) and str(a.limits[rt]) == str(w[rt].limit)
    f0 = flat.run_batch(hs, objs)
    if mode != "ref_index":  # (REF_INDEX picks by position: neither rule bounds the other)
        assert res[0][ResourceType.CPU].request > f0[0][ResourceType.CPU].request
        assert res[0][ResourceType.CPU].limit > f0[0][ResourceType.CPU].limit
    for rt in (ResourceType.CPU, ResourceType.Memory):  # one pod: the flat rule
        assert same_decimal(res[1][rt].request, f0[1][rt].request) and same_decimal(res[1][rt].limit, f0[1][rt].limit)
    one = strat.run(hs[0], objs[0])
    assert same_decimal(one[ResourceType.CPU].limit, res[0][ResourceType.CPU].limit)
    if mode != "ref_index":
        assert all(r[ResourceType.CPU].limit >= r[ResourceType.CPU].request for r in res)


@pytest.mark.parametrize("mode", MODES)
def test_runner_and_three_objects(mode):
    runner_check(mode)

"""cpu_aggregation = "pods_max" on the MI355X: krr_simple_run_pods bit for bit against
oracle.percentile over the pod CSR, the numpy fold of those pod results (test_gpu_group_max.fold)
and oracle.seg_max; then the strategy, the records path and the runner against the Python max()
of the flat strategy's own per-pod proposals."""
import decimal
import json
import os
from decimal import Decimal

import numpy as np
import pytest

from test_gpu_group_max import fold

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["ref_index", "sorted_lower", "linear"]
POD_LENS = [1, 2, 63, 64, 65, 1440, 5000]


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


def params_of(p, mode):
    from krr_amd.core.engine import percentile_params

    return percentile_params(Decimal(str(p)), mode)


def oracle_pods(x, offs, prm, gaps):
    from oracle import oracle

    max_n = int(np.diff(offs).max()) if offs.size > 1 else 0
    tab = None
    if prm.mode != 2 and prm.rule.needs_table(max_n):
        tab = prm.rule.table(max(max_n, 1))
    return oracle.percentile(x, offs, prm.mode, prm.p_num, prm.p_den, prm.q, gaps, k_table=tab)


def make_fleet(seed, gaps, pods_per_object=None, extra_pod_len=0):
    """About 40 objects with 0..7 pods of lengths from POD_LENS (every count and every length
    occurs); gapped: 10 % of the slots absent and some pods without one present sample.
    ``extra_pod_len``: one more object with a single pod of that many slots.  Values are
    rounded (ties) and positive (the sign of a zero LINEAR result is unspecified)."""
    rng = np.random.default_rng(seed)
    if pods_per_object is None:
        pods_per_object = np.concatenate([np.arange(8), rng.integers(0, 8, 32)])
    pod_lens, per_object = [], []
    for k in pods_per_object:
        lens = rng.choice(POD_LENS, int(k))
        pod_lens.extend(lens.tolist())
        per_object.append(int(k))
    if len(pod_lens) >= len(POD_LENS):
        pod_lens[:len(POD_LENS)] = POD_LENS  # every length occurs, among the first objects' pods
    if extra_pod_len:
        pod_lens.append(extra_pod_len)
        per_object.append(1)
    pod_offs = np.concatenate([[0], np.cumsum(pod_lens)]).astype(np.int64)
    groups = np.concatenate([[0], np.cumsum(per_object)]).astype(np.int64)
    x = np.round(rng.gamma(2.0, 0.05, int(pod_offs[-1])), 3) + 0.001
    if gaps:
        x[rng.random(x.size) < 0.1] = np.nan
        for j in rng.choice(len(pod_lens) - 1, 6, replace=False):  # pods with no present sample
            x[pod_offs[j]:pod_offs[j + 1]] = np.nan
    obj_offs = pod_offs[groups]
    mem_lens = rng.integers(0, 3000, len(per_object))
    mem_offs = np.concatenate([[0], np.cumsum(mem_lens)]).astype(np.int64)
    mem = np.floor(rng.normal(2e8, 2e7, int(mem_offs[-1])))
    if gaps:
        mem[rng.random(mem.size) < 0.1] = np.nan
    return x, pod_offs, groups, obj_offs, mem, mem_offs


def run_pods(gpu, x, pod_offs, groups, mem, mem_offs, gaps, prm, records=True):
    import torch

    ctx, dev = gpu
    S, n_pods = groups.size - 1, pod_offs.size - 1
    xd = torch.from_numpy(x).to(dev)
    pcs = ctx.series(xd, torch.from_numpy(pod_offs).to(dev), max(int(np.diff(pod_offs).max(initial=0)), 1), gaps)
    ms = ctx.series(torch.from_numpy(mem).to(dev), torch.from_numpy(mem_offs).to(dev),
                    max(int(np.diff(mem_offs).max(initial=0)), 1), gaps)
    out = {}
    for k, dt, n, fill in (("cpu_value", torch.float64, S, -777.0), ("cpu_count", torch.int64, S, -7),
                           ("cpu_flags", torch.int32, S, -1), ("cpu_pod", torch.int64, S, -99),
                           ("mem_value", torch.float64, S, -777.0), ("mem_count", torch.int64, S, -7),
                           ("mem_flags", torch.int32, S, -1), ("pod_value", torch.float64, n_pods, -777.0),
                           ("pod_count", torch.int64, n_pods, -7), ("pod_flags", torch.int32, n_pods, -1)):
        out[k] = torch.full((n,), fill, dtype=dt, device=dev)
    rec = torch.full((S, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) if records else None
    ctx.simple_run_pods(pcs, torch.from_numpy(groups).to(dev), ms, prm, out, records=rec)
    # the pod-level outputs are krr_segmented_percentile's over the pod series
    sv = torch.full((n_pods,), -777.0, dtype=torch.float64, device=dev)
    sn = torch.full((n_pods,), -7, dtype=torch.int64, device=dev)
    sf = torch.full((n_pods,), -1, dtype=torch.int32, device=dev)
    ctx.segmented_percentile(pcs, prm, sv, sn, sf)
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in out.items()}
    assert np.array_equal(host["pod_value"].view(np.uint64), sv.cpu().numpy().view(np.uint64))
    assert np.array_equal(host["pod_count"], sn.cpu().numpy()) and np.array_equal(host["pod_flags"], sf.cpu().numpy())
    return host, (rec.cpu().numpy() if records else None)


def check_against_references(host, rec, x, pod_offs, groups, mem, mem_offs, gaps, prm, tag):
    from oracle import oracle

    pv, pn, pf = oracle_pods(x, pod_offs, prm, gaps)
    assert np.array_equal(host["pod_value"].view(np.uint64), pv.view(np.uint64)), tag
    assert np.array_equal(host["pod_count"], pn), tag
    assert np.array_equal(host["pod_flags"].view(np.uint32), pf.astype(np.uint32)), tag
    wv, wn, wf, wa = fold(groups, pv[None], pn, pf.astype(np.uint32)[None])
    assert np.array_equal(host["cpu_value"].view(np.uint64), wv[0]), tag
    assert np.array_equal(host["cpu_count"], wn), tag
    assert np.array_equal(host["cpu_flags"].view(np.uint32), wf[0]), tag
    assert np.array_equal(host["cpu_pod"], wa[0]), tag
    mv, mn, mf = oracle.seg_max(mem, mem_offs, gaps)
    assert np.array_equal(host["mem_value"].view(np.uint64), mv.view(np.uint64)), tag
    assert np.array_equal(host["mem_count"], mn), tag
    assert np.array_equal(host["mem_flags"].view(np.uint32), mf.astype(np.uint32)), tag
    if rec is not None:
        assert np.array_equal(rec[:, 0].view(np.uint64), wv[0]), tag
        assert np.array_equal(rec[:, 1].view(np.uint64), mv.view(np.uint64)), tag
        assert np.array_equal(rec[:, 2], wn | (wf[0].astype(np.int64) << 48)), tag
        assert np.array_equal(rec[:, 3], mn | (mf.astype(np.int64) << 48)), tag
    return wv, wa


@pytest.mark.parametrize("p", [50, 99])
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_run_pods_matches_oracle_fold_and_max(gpu, mode, gaps, p):
    x, pod_offs, groups, _, mem, mem_offs = make_fleet(31, gaps)
    prm = params_of(p, mode)
    host, rec = run_pods(gpu, x, pod_offs, groups, mem, mem_offs, gaps, prm)
    _, wa = check_against_references(host, rec, x, pod_offs, groups, mem, mem_offs, gaps, prm, (mode, gaps, p))
    # the fold is not the flat percentile, and a later pod wins somewhere
    assert (wa[0] > 0).any() and (wa[0] == -1).any()


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_run_pods_window_select(gpu, mode, gaps):
    """One 50,400-slot pod at p50: the launch is planned by that length (window select, the
    long-segment kernel), the short pods with it; its misses go through the fallback pass, whose
    launch gets the pod count."""
    from krr_amd import _native

    prm = params_of(50, mode)
    assert _native.select_plan(50_400, prm).hselect == 1 and _native.select_plan(50_400, prm).fused_hselect == 1
    x, pod_offs, groups, _, mem, mem_offs = make_fleet(37, gaps, extra_pod_len=50_400)
    host, rec = run_pods(gpu, x, pod_offs, groups, mem, mem_offs, gaps, prm)
    check_against_references(host, rec, x, pod_offs, groups, mem, mem_offs, gaps, prm, (mode, gaps))
    assert gpu[0].wselect_fallbacks() >= 0  # any count: the results are exact either way


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_one_pod_per_object_equals_the_flat_run(gpu, mode, gaps):
    import torch

    ctx, dev = gpu
    x, pod_offs, groups, obj_offs, mem, mem_offs = make_fleet(41, gaps, pods_per_object=np.ones(40, dtype=np.int64))
    assert np.array_equal(obj_offs, pod_offs)
    prm = params_of(99, mode)
    host, rec = run_pods(gpu, x, pod_offs, groups, mem, mem_offs, gaps, prm)
    S = groups.size - 1
    cs = ctx.series(torch.from_numpy(x).to(dev), torch.from_numpy(obj_offs).to(dev), int(np.diff(obj_offs).max()), gaps)
    ms = ctx.series(torch.from_numpy(mem).to(dev), torch.from_numpy(mem_offs).to(dev),
                    int(np.diff(mem_offs).max()), gaps)
    out = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
           (("cpu_value", torch.float64), ("cpu_count", torch.int64), ("cpu_flags", torch.int32),
            ("mem_value", torch.float64), ("mem_count", torch.int64), ("mem_flags", torch.int32))}
    flat_rec = torch.zeros((S, 4), dtype=torch.int64, device=dev)
    ctx.simple_run(cs, ms, prm, out, records=flat_rec)
    torch.cuda.synchronize()
    for k, t in out.items():
        a, b = host[k], t.cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b), k
    assert np.array_equal(rec, flat_rec.cpu().numpy())
    assert np.array_equal(host["cpu_pod"], np.where(host["cpu_flags"] & 4, -1, 0))


def test_argument_checks(gpu):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    x, pod_offs, groups, _, mem, mem_offs = make_fleet(43, False, pods_per_object=np.array([2, 0, 3]))
    prm = params_of(99, "linear")
    bad = groups.copy()
    bad[-1] -= 1  # does not span the pod segments
    with pytest.raises(_native.NativeError) as e:
        run_pods(gpu, x, pod_offs, bad, mem, mem_offs, False, prm)
    assert e.value.code == _native.KRR_E_INVALID
    with pytest.raises(_native.NativeError) as e:  # one object more than the memory series holds
        run_pods(gpu, x, pod_offs, groups, mem[:mem_offs[-2]], mem_offs[:-1], False, prm)
    assert e.value.code == _native.KRR_E_INVALID
    # a fleet without one pod: every object EMPTY, memory as ever
    g0 = np.zeros(4, dtype=np.int64)
    host, rec = run_pods(gpu, np.zeros(0), np.zeros(1, dtype=np.int64), g0, mem, mem_offs, False, prm)
    assert (host["cpu_flags"] == 4).all() and (host["cpu_pod"] == -1).all() and np.isnan(host["cpu_value"]).all()
    check_against_references(host, rec, np.zeros(0), np.zeros(1, dtype=np.int64), g0, mem, mem_offs, False, prm, "no pods")


# ---------------------------------------------------------------------------------------------
# strategy level
# ---------------------------------------------------------------------------------------------

def load(name):
    with open(os.path.join(HERE, "golden", name)) as fh:
        return json.load(fh)["cases"]


def hist(case):
    from krr_amd.core.models.allocations import ResourceType

    return {ResourceType.CPU: {k: [Decimal(s) for s in v] for k, v in case["cpu"].items() if v},
            ResourceType.Memory: {k: [Decimal(s) for s in v] for k, v in case["mem"].items() if v}}


def obj(name):
    from krr_amd.api.models import K8sObjectData, ResourceAllocations

    return K8sObjectData(cluster=None, name=name, container="c", pods=["p"], namespace="ns", kind="Deployment",
                         allocations=ResourceAllocations(requests={}, limits={}))


def split_cases(cases):
    """(the cases without a NaN among their CPU samples, how many were left out, how many of the
    kept ones have two or more pods with samples) — found by scanning the inputs."""
    kept = [c for c in cases if not any(Decimal(s).is_nan() for v in c["cpu"].values() for s in v)]
    multi = sum(1 for c in kept if sum(1 for v in c["cpu"].values() if v) >= 2)
    return kept, len(cases) - len(kept), multi


# fixture: (cases, left out for a NaN CPU sample, multi-pod cases kept) as counted on this tree
COUNTS = {"simple_strategy.json": (65, 2, 39), "simple_strategy_exact.json": (35, 1, 18)}


def same_decimal(a, b):
    return a.is_nan() == b.is_nan() and str(a) == str(b)


@pytest.mark.parametrize("mode", ["ref_index", "sorted_lower"])
@pytest.mark.parametrize("fixture", list(COUNTS))
def test_strategy_equals_max_of_per_pod_proposals(fixture, mode):
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.strategies.simple import PercentileMode, SimpleStrategy, SimpleStrategySettings

    cases = load(fixture)
    kept, left_out, multi = split_cases(cases)
    n_cases, n_out, n_multi = COUNTS[fixture]
    assert len(cases) == n_cases and left_out == n_out and multi >= n_multi
    kw = dict(percentile_mode=PercentileMode(mode))
    concat = SimpleStrategy(SimpleStrategySettings(**kw))
    pods_max = SimpleStrategy(SimpleStrategySettings(cpu_aggregation="pods_max", **kw))
    # a NaN among the MEMORY samples makes max() raise in either aggregation (simple.py:29): those
    # histories run one by one, the others as one batch
    mem_nan = [any(Decimal(s).is_nan() for v in c["mem"].values() for s in v) for c in kept]

    def run(strat):
        batch = [c for c, bad in zip(kept, mem_nan) if not bad]
        res = iter(strat.run_batch([hist(c) for c in batch], [obj(c["name"]) for c in batch]))
        out = []
        for c, bad in zip(kept, mem_nan):
            if not bad:
                out.append(next(res))
                continue
            try:
                out.append(strat.run_batch([hist(c)], [obj(c["name"])])[0])
            except decimal.InvalidOperation:
                out.append(decimal.InvalidOperation)
        return out

    hs = [hist(c) for c in kept]
    got, flat = run(pods_max), run(concat)
    differs = 0
    for c, h, r, f in zip(kept, hs, got, flat):
        if f is decimal.InvalidOperation or r is decimal.InvalidOperation:
            assert r is f, c["name"]
            continue
        per_pod = [concat.settings.calculate_cpu_proposal({pod: samples})
                   for pod, samples in h[ResourceType.CPU].items() if samples]
        want = max(per_pod) if per_pod else Decimal("NaN")
        cpu = r[ResourceType.CPU].request
        assert same_decimal(cpu, want), (c["name"], cpu, want)
        assert r[ResourceType.CPU].limit is None
        assert same_decimal(r[ResourceType.Memory].request, f[ResourceType.Memory].request), c["name"]
        assert same_decimal(r[ResourceType.Memory].limit, f[ResourceType.Memory].limit), c["name"]
        differs += not same_decimal(cpu, f[ResourceType.CPU].request)
    assert differs > 0  # the two aggregations are different rules on these fixtures


def three_objects():
    rng = np.random.default_rng(3)

    def pod(n, scale):
        return [Decimal(repr(round(float(v), 4))) for v in rng.gamma(2.0, scale, n)]

    from krr_amd.core.models.allocations import ResourceType

    hs = []
    for pods in ([(300, 0.01), (200, 0.2), (250, 0.01)], [(120, 0.05)], [(80, 0.3), (500, 0.02)]):
        cpu = {f"p{i}": pod(n, s) for i, (n, s) in enumerate(pods)}
        mem = {f"p{i}": [Decimal(int(v)) for v in rng.normal(2e8, 2e7, n)] for i, (n, s) in enumerate(pods)}
        hs.append({ResourceType.CPU: cpu, ResourceType.Memory: mem})
    return hs


@pytest.mark.parametrize("mode", MODES)
def test_records_path_and_runner(mode):
    from krr_amd.core.distributed import raw_from_records
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import PercentileMode, SimpleStrategy, SimpleStrategySettings

    strat = SimpleStrategy(SimpleStrategySettings(cpu_aggregation="pods_max", percentile_mode=PercentileMode(mode)))
    hs = three_objects()
    fleet = strat.pack(hs)
    raw = strat.settings.run_fleet(fleet)
    rec = raw_from_records(strat.settings.run_fleet_records(fleet))
    for k in ("cpu_value", "mem_value"):
        assert np.array_equal(getattr(raw, k).view(np.uint64), getattr(rec, k).view(np.uint64)), k
    for k in ("cpu_count", "cpu_flags", "mem_count", "mem_flags"):
        assert np.array_equal(getattr(raw, k), getattr(rec, k)), k
    # the hot second pod of object 0 decides, not the flat percentile
    flat = SimpleStrategy(SimpleStrategySettings(percentile_mode=PercentileMode(mode))).settings.run_fleet(fleet)
    assert raw.cpu_value[0] > flat.cpu_value[0] and raw.cpu_value[1] == flat.cpu_value[1]
    objs = [obj(f"o{i}") for i in range(3)]
    got = BatchedRunner(strat, 5, 10).recommend(objs, hs)
    want = [format_result(r, 5, 10) for r in strat.run_batch(hs, objs)]
    for g, w in zip(got, want):
        for res in (ResourceType.CPU, ResourceType.Memory):
            assert str(g[res].request) == str(w[res].request) and str(g[res].limit) == str(w[res].limit)


def test_fleet_without_pod_boundaries_is_refused():
    from krr_amd.core.packing import PackedFleet, PackedSeries
    from krr_amd.strategies.simple import SimpleStrategySettings

    offs = np.array([0, 3], dtype=np.int64)
    fleet = PackedFleet(PackedSeries(np.array([1.0, 2.0, 3.0]), offs, 3), PackedSeries(np.array([1.0, 2.0, 3.0]), offs, 3))
    with pytest.raises(ValueError, match="device packer"):
        SimpleStrategySettings(cpu_aggregation="pods_max").run_fleet(fleet)
    assert SimpleStrategySettings().run_fleet(fleet).cpu_count[0] == 3  # concat needs none


def test_chunked_runs_equal_the_whole(monkeypatch):
    """A fleet run as several chunks (each with its own rebased pod offsets and groups) gives the
    whole run's results, pod-level outputs, records and — for HistoryData outside Prometheus'
    strings, located per pod and per chunk — Decimals."""
    from krr_amd.core.distributed import raw_from_records
    from krr_amd.core.engine import SimpleEngine
    from krr_amd.core.models.allocations import ResourceType
    from krr_amd.core.packing import PackedFleet, PackedSeries
    from krr_amd.strategies.simple import PercentileMode, SimpleStrategy, SimpleStrategySettings

    x, pod_offs, groups, obj_offs, mem, mem_offs = make_fleet(47, True)
    cpu = PackedSeries(x, obj_offs, int(np.diff(obj_offs).max()), True)
    cpu.pod_offsets, cpu.pod_groups = pod_offs, groups
    fleet = PackedFleet(cpu, PackedSeries(mem, mem_offs, int(np.diff(mem_offs).max()), True))
    prm = params_of(99, "linear")
    whole = SimpleEngine(0).run_packed(fleet, prm, aggregation="pods_max", return_pods=True)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 8 * (x.size + mem.size) // 5
    assert len(eng._chunk_bounds(fleet)) >= 3
    parts = eng.run_packed(fleet, prm, aggregation="pods_max", return_pods=True)
    rec = raw_from_records(eng.run_packed_records(fleet, prm, aggregation="pods_max"))
    for other in (parts, rec):
        for k in ("cpu_value", "mem_value"):
            assert np.array_equal(getattr(whole, k).view(np.uint64), getattr(other, k).view(np.uint64)), k
        for k in ("cpu_count", "cpu_flags", "mem_count", "mem_flags"):
            assert np.array_equal(getattr(whole, k), getattr(other, k)), k
    assert np.array_equal(whole.pods["pod_value"].view(np.uint64), parts.pods["pod_value"].view(np.uint64))
    for k in ("pod_count", "pod_flags", "cpu_pod"):
        assert np.array_equal(whole.pods[k], parts.pods[k]), k
    assert whole.pods["pod_count"].size == pod_offs.size - 1 and (whole.pods["cpu_pod"] > 0).any()

    kept, _, _ = split_cases(load("simple_strategy_exact.json"))
    cases = [c for c in kept if not any(Decimal(s).is_nan() for v in c["mem"].values() for s in v)]
    hs, objs = [hist(c) for c in cases], [obj(c["name"]) for c in cases]
    for mode in ("ref_index", "sorted_lower"):
        strat = SimpleStrategy(SimpleStrategySettings(cpu_aggregation="pods_max", percentile_mode=PercentileMode(mode)))
        one = strat.run_batch(hs, objs)
        with monkeypatch.context() as m:
            m.setattr(SimpleEngine, "chunk_bytes", 64)
            assert len(SimpleEngine(0)._chunk_bounds(strat.pack(hs))) >= 4
            many = strat.run_batch(hs, objs)
        for c, a, b in zip(cases, one, many):
            for res in (ResourceType.CPU, ResourceType.Memory):
                assert same_decimal(a[res].request, b[res].request), (mode, c["name"])

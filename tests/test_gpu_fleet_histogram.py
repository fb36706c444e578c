"""krr_amd.api.batch.FleetBatch.histogram on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) through the real engine
against the plain restatement (tests/_whist_ref.py), bit for bit: host-packed, chunked, per pod
and resident in HBM with gaps; two time slices merged into the whole; the bracket against the
exact weighted percentile; then examples/vpa_strategy.py through the BatchedRunner."""
from decimal import Decimal

import numpy as np
import pytest

from _whist_ref import EMPTY, QNAN, SKETCH_RANGE, bracket, whist_one
from _wquantile_ref import fraction_of
from krr_amd.api import HistogramBins, default_bins  # noqa: F401  (the feature: absent, nothing here runs)
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
nan = np.nan
PERCENTILES = ("50", "90", "95", "99.9", "100")


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, r):
    return np.array([float(x) for samples in h[r].values() for x in samples])


def _geom(bins):
    return bins.mantissa_bits, bins.min_exponent, bins.octaves


def _hold(hist, series_list, table, base=None):
    """Every series: row, total, extremes, count and flags equal the restatement's; then every
    percentile's bin, bracket and flags."""
    geom = _geom(hist.bins)
    assert hist.n_objects == len(series_list) and tuple(hist.tensor().shape) == (len(series_list), hist.bins.width)
    rows = hist.tensor().cpu().numpy().view(np.uint64)
    ups, fl = hist.percentiles(PERCENTILES, return_flags=True)
    for s, x in enumerate(series_list):
        row, W, mn, mx = whist_one(x, table, geom, 0 if base is None else int(base[s]))
        present = int(np.count_nonzero(~np.isnan(x)))
        assert np.array_equal(rows[s], row) and np.array_equal(hist.of(s), row), s
        assert int(hist.wsum[s]) == W and hist.total[s] == W / 2 ** 32 and hist.count[s] == present, s
        assert int(hist.wmin[s:s + 1].view(np.uint64)[0]) == mn and int(hist.wmax[s:s + 1].view(np.uint64)[0]) == mx, s
        assert hist.flags[s] == (EMPTY if present == 0 else 0), s
        for j, p in enumerate(PERCENTILES):
            b, lo, hi, f = bracket(row, mn, mx, geom, *fraction_of(p))
            glo, ghi = hist.bracket(p)
            assert hist.answer_bins(p)[s] == b and fl[j][s] == f | hist.flags[s], (s, p)
            assert int(glo[s:s + 1].view(np.uint64)[0]) == lo and int(ghi[s:s + 1].view(np.uint64)[0]) == hi, (s, p)
            assert int(ups[j][s:s + 1].view(np.uint64)[0]) == hi, (s, p)


def _same(a, b):
    assert np.array_equal(a.tensor().cpu().numpy(), b.tensor().cpu().numpy())
    for k in ("count", "flags", "wsum"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("wmin", "wmax"):
        assert np.array_equal(getattr(a, k).view(np.uint64), getattr(b, k).view(np.uint64)), k


def test_host_packed_fleet_pods_and_chunks(histories):
    from krr_amd.api import FleetBatch, FleetHistogram, decay_weights
    from krr_amd.core.engine import SimpleEngine

    batch = FleetBatch(histories, device=0)
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    tables = {"decay": decay_weights(6, 130), "short": np.array([0, 9, 2], np.uint64)}
    narrow = {CPU: HistogramBins(3, -4, 2), MEM: HistogramBins(2, 28, 1)}  # the lumped bins in use
    for r in (CPU, MEM):
        series = [_flat(h, r) for h in histories]
        for table in tables.values():
            for bins in (None, narrow[r]):
                h = batch.histogram(r, table, bins)
                assert isinstance(h, FleetHistogram) and h.bins == (bins or default_bins(r))
                _hold(h, series, table)
                assert batch.histogram(r, table, bins) is h  # cached
        unit = batch.histogram(r)
        _hold(unit, series, np.array([1], np.uint64))
        assert np.array_equal(unit.wsum, unit.count.astype(np.uint64))
        assert len(list(eng._series_parts(small.series(r)))) >= 5
        _same(small.histogram(r, tables["decay"]), batch.histogram(r, tables["decay"]))  # chunking changes no bit
        lumped = batch.histogram(r, tables["decay"], narrow[r]).percentiles(["50", "100"], return_flags=True)[1]
        assert (lumped & SKETCH_RANGE).any()
    pods = batch.per_pod(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    _hold(pods.histogram(CPU, tables["decay"]), kept, tables["decay"])
    with pytest.raises(ValueError):
        batch.histogram(CPU, tables["decay"], age_base=-1)
    with pytest.raises(ValueError):
        batch.histogram(CPU, tables["decay"], age_base=np.zeros(N + 1, np.int64))
    with pytest.raises(ValueError):
        batch.histogram(CPU, tables["decay"], bins=(4, -10, 20))
    with pytest.raises(ValueError):
        batch.histogram(CPU, np.array([0.5]))


def test_gapped_fleet_resident_in_hbm():
    import torch

    from krr_amd.api import FleetBatch, decay_weights
    from krr_amd.core.packing import PackedFleet, PackedSeries

    rng = np.random.default_rng(51)
    lens = rng.integers(1, 3001, 14)
    lens[[2, 9]] = 0
    segs = []
    for s, n in enumerate(lens.tolist()):
        x = rng.gamma(2.0, 0.05, n) if s % 2 else np.floor(rng.normal(2e8, 2e7, n))
        x[rng.random(n) < 0.2] = nan
        segs.append(x)
    segs[5][:] = nan
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = torch.device("cuda:0")
    ps = PackedSeries(torch.from_numpy(np.concatenate(segs)).to(dev), torch.from_numpy(offs).to(dev), int(lens.max()), True)
    batch = FleetBatch.from_fleet(PackedFleet(ps, ps), device=0)
    bins = HistogramBins(4, -10, 40)  # CPU-like and memory-like series in one row layout
    for table in (decay_weights(300, 3000), decay_weights(20, 3000)):
        _hold(batch.histogram(MEM, table, bins), segs, table)
    base = rng.integers(0, 500, 14)
    _hold(batch.histogram(MEM, decay_weights(300, 3000), bins, age_base=base), segs, decay_weights(300, 3000), base)
    h7 = batch.histogram(MEM, decay_weights(300, 3000), bins, age_base=7)
    _hold(h7, segs, decay_weights(300, 3000), np.full(14, 7))


def test_merge_of_two_time_slices_is_the_whole(histories):
    from krr_amd.api import FleetBatch, decay_weights

    table = decay_weights(6, 130)
    cut = [{r: {p: x[:len(x) // 2] for p, x in h[r].items()} for r in (CPU, MEM)} for h in histories]
    rest = [{r: {p: x[len(x) // 2:] for p, x in h[r].items()} for r in (CPU, MEM)} for h in histories]
    whole, older, newer = (FleetBatch(hh, device=0).per_pod(CPU) for hh in (histories, cut, rest))
    # per pod: a pod's series cut in two (pods without samples are dropped by the packer alike)
    pods = [x for h in histories for x in h[CPU].values() if len(x)]
    keep_old = np.array([len(x) // 2 > 0 for x in pods])
    after = np.array([len(x) - len(x) // 2 for x in pods])
    want = whole.histogram(CPU, table)
    new = newer.histogram(CPU, table)
    assert new.n_objects == len(pods) and older.n_objects == int(keep_old.sum())
    old = older.histogram(CPU, table, age_base=after[keep_old])
    # pods of one sample have no older half: their row of the whole is the newer slice's alone
    rows_old = np.zeros((len(pods), want.bins.width), np.int64)
    rows_old[keep_old] = old.tensor().cpu().numpy()
    assert np.array_equal(rows_old + new.tensor().cpu().numpy(), want.tensor().cpu().numpy())
    # object by object (one segment per object, no pod dropped): FleetHistogram.merge itself
    series = [_flat(h, MEM) for h in histories]
    after = np.array([sum(len(x) - len(x) // 2 for x in h[MEM].values()) for h in histories])
    after[0] = series[0].size  # object 0 has no older slice at all
    # an object's flat series is its pods one after the other: cut the FLAT series where the rest begins
    cut = [{MEM: {"a": [Decimal(repr(float(v))) for v in x[:x.size - a]]}, CPU: {}} for x, a in zip(series, after)]
    rest = [{MEM: {"a": [Decimal(repr(float(v))) for v in x[x.size - a:]]}, CPU: {}} for x, a in zip(series, after)]
    want = FleetBatch(histories, device=0).histogram(MEM, table)
    old = FleetBatch(cut, device=0).histogram(MEM, table, age_base=after)
    new = FleetBatch(rest, device=0).histogram(MEM, table)
    for merged in (old.merge(new), new.merge(old)):
        _same(merged, want)
        assert np.array_equal(merged.percentiles(PERCENTILES).view(np.uint64), want.percentiles(PERCENTILES).view(np.uint64))
    # KRR_FLAG_EMPTY stays only where both slices were empty
    assert (want.flags == EMPTY).sum() == 2 and old.flags[0] == EMPTY and (old.flags == EMPTY).sum() >= 3
    with pytest.raises(ValueError):
        old.merge(FleetBatch(rest, device=0).histogram(MEM, table, HistogramBins(3, 20, 20)))
    with pytest.raises(ValueError):
        old.merge(FleetBatch(rest[:5], device=0).histogram(MEM, table))


def test_bracket_encloses_the_exact_weighted_percentile(histories):
    from krr_amd.api import FleetBatch, decay_weights

    batch = FleetBatch(histories, device=0)
    table = decay_weights(6, 130)
    for r in (CPU, MEM):
        h = batch.histogram(r, table)
        m = h.bins.mantissa_bits
        for p in PERCENTILES:
            v = batch.weighted_percentile(r, p, table)
            lo, hi = h.bracket(p)
            has = ~np.isnan(v)
            assert has.sum() == N - 2 and np.isnan(lo[~has]).all() and np.isnan(hi[~has]).all()
            assert np.array_equal(h.answer_bins(p)[has], h.bins.bin_of(v[has]))
            assert (lo[has] <= v[has]).all() and (v[has] <= hi[has]).all()
            assert (hi[has] <= v[has] * (1 + 2.0 ** -m)).all()  # default bins hold every sample of this fleet
            assert np.array_equal(h.percentile(p).view(np.uint64), hi.view(np.uint64))
        assert np.array_equal(h.percentile("100").view(np.uint64), h.wmax.view(np.uint64))
        assert np.array_equal(h.total, batch.weight_sums(r, table))


def test_vpa_strategy_through_the_batched_runner(histories, monkeypatch):
    """recommend() over the fleet equals the strategy's own per-object run(), from exactly one
    histogram launch over every pod; the request is the p90 bucket end of the restatement x 1.15."""
    from examples.vpa_strategy import VpaSettings, VpaStrategy
    from krr_amd import _native
    from krr_amd.api import decay_weights
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import format_result
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.utils.prom_decimal import prom_decimal

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    calls = []
    real = _native.Context.segmented_whist
    monkeypatch.setattr(_native.Context, "segmented_whist",
                        lambda self, series, *a, **k: (calls.append(series.n_segments), real(self, series, *a, **k))[1])
    strategy = VpaStrategy(VpaSettings(half_life_slots=6, memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    runner = BatchedRunner(strategy)
    got = runner.recommend(objects, histories)
    n_pods = sum(1 for h in histories for x in h[CPU].values() if len(x))
    assert calls == [n_pods]  # one launch over every pod of the fleet, three percentiles read from it
    raw = strategy.run_batch(histories, objects)
    table = decay_weights(6, max(len(x) for h in histories for x in h[CPU].values()))
    geom = _geom(default_bins(CPU))
    for o, (h, obj) in enumerate(zip(histories, objects)):
        one = strategy.run(h, obj)
        want = format_result(one, runner.cpu_min_value, runner.memory_min_value)
        for r in (CPU, MEM):
            for field in ("request", "limit"):
                a, b = getattr(got[o][r], field), getattr(want[r], field)
                assert (a is None and b is None) or (a.is_nan() and b.is_nan()) or (a == b and str(a) == str(b)), (o, r)
        pods = [x for x in h[CPU].values() if len(x)]
        if not pods:
            assert o in (3, 11) and raw[o][CPU].request.is_nan() and raw[o][CPU].limit.is_nan()
            continue
        ends = {}
        for p in (90, 95):
            per_pod = []
            for x in pods:
                row, W, mn, mx = whist_one([float(s) for s in x], table, geom)
                hi = bracket(row, mn, mx, geom, p, 1)[2]
                per_pod.append(float(np.array([hi], np.uint64).view(np.float64)[0]))
            ends[p] = prom_decimal(max(per_pod))
        assert raw[o][CPU].request == ends[90] * Decimal("1.15") == one[CPU].request, o
        assert raw[o][CPU].limit == ends[95] * Decimal("1.15") and raw[o][CPU].limit >= raw[o][CPU].request, o
        assert raw[o][MEM].request == max(s for x in h[MEM].values() for s in x) * Decimal("1.1")
    assert QNAN  # the restatement's NaN is the kernels' (imported for the reader)

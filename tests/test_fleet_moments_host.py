"""krr_amd.api.batch.FleetBatch.moments / FleetMoments and examples/trend_strategy.py without a
device, as tests/test_fleet_batch_host.py does it: ``SimpleEngine._moments_part`` is stood in by
an exact-then-rounded restatement (tests/_moments_ref.py: exact integer sums of the float64
inputs, one rational division, ONE rounding to float64), so that everything above a launch —
packing once, caching, chunking, pod views, the accessors, ``concat`` and the example strategy —
runs here.  The kernel itself: tests/test_gpu_moments.py and tests/test_gpu_fleet_moments.py."""
from decimal import Decimal

import numpy as np
import pytest

from _moments_ref import FIELDS, exact_moments, ratios, rounded
from krr_amd.core.models.allocations import ResourceType
from test_fleet_batch_host import N, _histories

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1


def np_moments(vals, offs, gaps=False, trend=True) -> dict:
    """krr_segmented_moments restated: numpy arrays per output name."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs)
    S = offs.size - 1
    out = {k: np.full(S, np.nan) for k in (FIELDS if trend else ("mean", "m2"))}
    out["count"], out["flags"] = np.zeros(S, np.int64), np.zeros(S, np.int32)
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        n = int(np.count_nonzero(~np.isnan(x))) if gaps else x.size
        out["count"][s] = n
        if n == 0:
            out["flags"][s] = EMPTY
        elif not gaps and np.isnan(x).any():
            out["flags"][s] = NAN
        else:
            r = rounded(exact_moments(x))
            for k in out:
                if k in r:
                    out[k][s] = r[k]
    return out


def moments_of(x, trend=True):
    """A FleetMoments of one series (NaN = absent slot) from the stand-in."""
    from krr_amd.api import FleetMoments

    x = np.asarray(x, dtype=np.float64)
    r = np_moments(x, np.array([0, x.size]), gaps=True, trend=trend)
    return FleetMoments(r["count"], r["mean"], r["m2"], r.get("tmean"), r.get("t2"), r.get("cxt"),
                        r["flags"].view(np.uint32), np.array([x.size], dtype=np.int64))


@pytest.fixture
def standin(monkeypatch):
    """The launchers stood in; returns the call log: ("moments", segments of the chunk, trend)."""
    import torch

    from _standin import k_table_for
    from krr_amd.core.engine import SimpleEngine
    from oracle import oracle

    calls = []

    def moments_part(self, ctx, part, trend):
        calls.append(("moments", part.n_segments, trend))
        return {k: torch.from_numpy(v) for k, v in np_moments(part.values, part.offsets, part.gaps_are_nan, trend).items()}

    def percentiles_part(self, ctx, part, params_list):
        rows = [oracle.percentile(part.values, part.offsets, p.mode, p.p_num, p.p_den, p.q, part.gaps_are_nan,
                                  k_table=k_table_for(part, p)) for p in params_list]
        return {"value": torch.from_numpy(np.stack([r[0] for r in rows])), "count": torch.from_numpy(rows[0][1]),
                "flags": torch.from_numpy(np.stack([r[2] for r in rows]).astype(np.int32))}

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_moments_part", moments_part)
    monkeypatch.setattr(SimpleEngine, "_percentiles_part", percentiles_part)
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return np.array([float(x) for samples in h[resource].values() for x in samples])


# --- FleetBatch.moments -------------------------------------------------------------------------
def test_packs_once_caches_and_trend_serves_no_trend(standin, histories, monkeypatch):
    from krr_amd.api import FleetBatch, FleetMoments, batch as batch_mod

    packed = []
    real = batch_mod.pack_resource
    monkeypatch.setattr(batch_mod, "pack_resource", lambda hs, r: (packed.append(r), real(hs, r))[1])
    b = FleetBatch(histories)
    mo = b.moments(CPU)
    assert isinstance(mo, FleetMoments) and mo.has_trend
    assert b.moments(CPU) is mo and b.moments(CPU, trend=False) is mo  # the trend result serves both
    assert packed == [CPU] and standin == [("moments", N, True)]
    for o, h in enumerate(histories):
        x = _flat(h, CPU)
        assert mo.count[o] == x.size == mo.slots[o]
        if x.size == 0:
            assert mo.flags[o] == EMPTY and all(np.isnan(getattr(mo, k)[o]) for k in FIELDS)
        else:
            assert mo.flags[o] == 0 and mo.mean[o] == pytest.approx(x.mean(), rel=1e-12)
            assert mo.variance()[o] == pytest.approx(x.var(), rel=1e-9)
    # the other way round: a no-trend result does not serve a trend request
    c = FleetBatch(histories)
    light = c.moments(MEM, trend=False)
    assert not light.has_trend and light.tmean is None and c.moments(MEM, trend=False) is light
    full = c.moments(MEM)
    assert full.has_trend and c.moments(MEM, trend=False) is full
    assert standin[1:] == [("moments", N, False), ("moments", N, True)]
    assert np.array_equal(light.mean, full.mean, equal_nan=True) and np.array_equal(light.m2, full.m2, equal_nan=True)


def test_chunks_concatenate_in_object_order(standin, histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    whole = FleetBatch(histories, engine=SimpleEngine(0))
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    parts = FleetBatch(histories, engine=small)
    for r in (CPU, MEM):
        a, c = whole.moments(r), parts.moments(r)
        for k in FIELDS + ("count", "flags", "slots"):
            assert np.array_equal(getattr(a, k), getattr(c, k), equal_nan=True), k
    chunked = [n for _, n, _ in standin if n < N]
    assert len(chunked) > 4 and sum(chunked) == 2 * N  # whole segments, every object once per resource


def test_per_pod(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    with pytest.raises(ValueError, match="pod boundaries"):
        b.per_pod(MEM).moments(MEM)  # the packers attach them to the CPU series only
    pods = b.per_pod(CPU)
    mo = pods.moments(CPU)
    kept = [np.array([float(v) for v in x]) for h in histories for x in h[CPU].values() if len(x)]
    assert mo.count.tolist() == [x.size for x in kept] == mo.slots.tolist()
    assert np.allclose(mo.mean, [x.mean() for x in kept], rtol=1e-12, atol=0)
    assert np.allclose(mo.std(), [x.std() for x in kept], rtol=1e-9, atol=0)
    assert standin == [("moments", len(kept), True)]


def test_no_device_raises(histories, monkeypatch):
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    b = FleetBatch(histories, engine=SimpleEngine(0))
    with pytest.raises(_native.NativeUnavailable):
        b.moments(CPU)
    with pytest.raises(_native.NativeUnavailable):
        b.moments(MEM, trend=False)


# --- FleetMoments -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 17, 120])
def test_accessors_against_numpy(n):
    """Well-conditioned data (kappa = sqrt(Sxx / M2) <= 100): rtol 1e-10 is above n kappa u ~ 1e-12
    for both sides and far below any error in a formula."""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.float64)
    x = 10.0 + 0.05 * i + rng.normal(0, 1.0, n)
    assert np.sqrt((x * x).sum() / ((x - x.mean()) ** 2).sum()) <= 100
    mo = moments_of(x)
    slope, intercept = np.polyfit(i, x, 1)
    rel = dict(rel=1e-10)
    assert mo.variance()[0] == pytest.approx(np.var(x), **rel) and mo.std()[0] == pytest.approx(np.std(x), **rel)
    assert mo.variance(ddof=1)[0] == pytest.approx(np.var(x, ddof=1), **rel)
    assert mo.std(ddof=1)[0] == pytest.approx(np.std(x, ddof=1), **rel)
    assert mo.slope[0] == pytest.approx(slope, **rel) and mo.intercept[0] == pytest.approx(intercept, **rel)
    want_r2 = 1.0 if n == 2 else np.corrcoef(i, x)[0, 1] ** 2
    assert mo.r2[0] == pytest.approx(want_r2, **rel) and mo.r2[0] <= 1.0
    assert mo.value_at(5)[0] == pytest.approx(intercept + slope * 5, **rel)
    assert mo.value_at(np.array([2.5]))[0] == pytest.approx(intercept + slope * 2.5, **rel)
    assert mo.forecast(10)[0] == pytest.approx(intercept + slope * (n - 1 + 10), **rel)
    assert mo.forecast(0)[0] == pytest.approx(mo.value_at(mo.slots - 1)[0], rel=1e-15)


def test_accessors_with_gaps_use_the_slot_index():
    """On the gapped layout the regressor is the slot, not the sample number."""
    rng = np.random.default_rng(8)
    x = 3.0 + 0.25 * np.arange(90) + rng.normal(0, 0.5, 90)
    x[rng.random(90) < 0.3] = np.nan
    keep = ~np.isnan(x)
    mo = moments_of(x)
    slope, intercept = np.polyfit(np.arange(90)[keep], x[keep], 1)
    assert mo.slope[0] == pytest.approx(slope, rel=1e-10) and mo.intercept[0] == pytest.approx(intercept, rel=1e-10)
    assert mo.forecast(5)[0] == pytest.approx(intercept + slope * 94, rel=1e-10) and mo.slots[0] == 90


def test_nan_rules():
    one, two, const, empty = moments_of([4.0]), moments_of([4.0, 6.0]), moments_of([2.5] * 9), moments_of([np.nan] * 3)
    assert one.variance()[0] == 0.0 and np.isnan(one.variance(ddof=1)[0]) and np.isnan(one.std(ddof=1)[0])
    assert two.variance(ddof=1)[0] == 2.0 and np.isnan(two.variance(ddof=2)[0])
    assert one.t2[0] == 0.0 and np.isnan(one.slope[0]) and np.isnan(one.intercept[0]) and np.isnan(one.r2[0])
    assert np.isnan(one.value_at(3)[0]) and np.isnan(one.forecast(1)[0])
    assert const.slope[0] == 0.0 and const.intercept[0] == 2.5 and np.isnan(const.r2[0])  # m2 = 0: no r2
    assert const.forecast(100)[0] == 2.5
    assert empty.flags[0] == EMPTY and empty.count[0] == 0 and empty.slots[0] == 3
    for v in (empty.variance(), empty.std(), empty.slope, empty.intercept, empty.r2, empty.value_at(0),
              empty.forecast(1)):
        assert np.isnan(v[0])
    lone_gap = moments_of([np.nan, np.nan, 7.0, np.nan])
    assert lone_gap.tmean[0] == 2.0 and lone_gap.mean[0] == 7.0 and np.isnan(lone_gap.slope[0])


def test_trend_accessors_raise_without_trend():
    mo = moments_of([1.0, 2.0, 4.0], trend=False)
    assert mo.variance()[0] == pytest.approx(14 / 9) and mo.std(ddof=1)[0] == pytest.approx(np.std([1, 2, 4], ddof=1))
    for use in (lambda: mo.slope, lambda: mo.intercept, lambda: mo.r2, lambda: mo.value_at(1), lambda: mo.forecast(1)):
        with pytest.raises(ValueError, match="trend"):
            use()
    assert not mo.concat(moments_of([3.0, 5.0])).has_trend  # no trend on one side: none in the result


def _within_bounds(mo, x):
    e = exact_moments(x)
    r = ratios({k: getattr(mo, k)[0] for k in FIELDS}, e)
    assert mo.count[0] == e["n"] and mo.slots[0] == x.size
    assert all(v <= 1.0 for v in r.values()), r


CONCAT_DATA = {
    "memory": lambda rng, n: np.floor(rng.normal(2e8, 2e7, n)),
    "cpu": lambda rng, n: rng.gamma(2.0, 0.05, n),
    "ramp": lambda rng, n: 5e7 + 1e4 * np.arange(n) + rng.normal(0, 1e6, n),
    "cond1e9": lambda rng, n: 1e9 + rng.random(n),
}


@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gaps"])
@pytest.mark.parametrize("kind", sorted(CONCAT_DATA))
def test_concat_splits_lie_within_the_bounds(kind, gaps):
    """moments(x[:k]).concat(moments(x[k:])) against the exact moments of x, held to the kernel's
    own bounds (n >= 40 present samples, so that n u covers the handful of roundings of two rounded
    inputs and one merge)."""
    rng = np.random.default_rng(12)
    n = 200
    x = CONCAT_DATA[kind](rng, n)
    if gaps:
        x[rng.random(n) < 0.2] = np.nan
        x[[0, n - 1]] = 1.0 + x[~np.isnan(x)][0]  # k = 1 and k = n - 1 split off one PRESENT sample
    for k in (0, 1, n // 2, n - 1, n):
        a, b = moments_of(x[:k]), moments_of(x[k:])
        mo = a.concat(b)
        _within_bounds(mo, x)
        assert mo.flags[0] == 0
        if k in (0, n):  # an empty side is the identity
            whole = moments_of(x)
            assert all(getattr(mo, f)[0] == getattr(whole, f)[0] for f in FIELDS)


def test_concat_folds_day_by_day():
    rng = np.random.default_rng(13)
    days = [np.floor(rng.normal(2e8 + 1e6 * d, 2e7, 96)) for d in range(3)]
    days[1][rng.random(96) < 0.25] = np.nan
    fold = moments_of(days[0]).concat(moments_of(days[1])).concat(moments_of(days[2]))
    _within_bounds(fold, np.concatenate(days))
    assert fold.slots[0] == 3 * 96
    other = moments_of(days[0]).concat(moments_of(days[1]).concat(moments_of(days[2])))  # the other bracketing
    _within_bounds(other, np.concatenate(days))


def test_concat_flags_and_shapes():
    from krr_amd.api import FleetMoments

    def two(first, second):  # a two-object result
        a, b = moments_of(first), moments_of(second)
        return FleetMoments(*(np.concatenate([getattr(a, f), getattr(b, f)]) for f in
                              ("count", "mean", "m2", "tmean", "t2", "cxt", "flags", "slots")))

    nan = np.nan
    left, right = two([nan, nan], [1.0, 2.0]), two([nan], [nan, nan, 5.0])
    got = left.concat(right)
    assert got.flags.tolist() == [EMPTY, 0] and got.count.tolist() == [0, 3] and got.slots.tolist() == [3, 5]
    assert got.tmean[1] == pytest.approx((0 + 1 + 4) / 3) and got.mean[1] == pytest.approx(8 / 3)
    assert all(np.isnan(getattr(got, f)[0]) for f in FIELDS)
    flagged = two([1.0], [1.0])
    flagged.flags[1] = NAN
    flagged.mean[1] = flagged.m2[1] = nan
    got = flagged.concat(left)
    assert got.flags.tolist() == [0, NAN] and got.mean[0] == 1.0 and np.isnan(got.mean[1])
    with pytest.raises(ValueError, match="same objects"):
        left.concat(moments_of([1.0]))


# --- examples/trend_strategy.py -----------------------------------------------------------------
def trend_request(history, sigmas, horizon):
    """The strategy's CPU definition per object, from numpy alone (None: no sample)."""
    best = None
    for samples in history[CPU].values():
        x = np.array([float(v) for v in samples])
        if x.size == 0:
            continue
        slope = np.polyfit(np.arange(x.size), x, 1)[0] if x.size >= 2 else 0.0
        v = x.mean() + sigmas * x.std() + max(slope, 0.0) * horizon
        best = v if best is None else max(best, v)
    return best


@pytest.mark.parametrize("horizon", [0.0, 30.0])
def test_trend_strategy_equals_numpy_per_object(standin, histories, horizon):
    from examples.trend_strategy import TrendHeadroomSettings, TrendHeadroomStrategy

    strategy = TrendHeadroomStrategy(TrendHeadroomSettings(cpu_sigmas=2.5, horizon_slots=horizon,
                                                           memory_percentile=Decimal(90),
                                                           memory_buffer_percentage=Decimal(10)))
    got = strategy.run_batch(histories)
    assert len(got) == N and standin == [("moments", standin[0][1], horizon > 0)]  # one launch over all pods
    slopes_up = 0
    for o, h in enumerate(histories):
        want = trend_request(h, 2.5, horizon)
        cpu, mem = got[o][CPU], got[o][MEM]
        assert cpu.limit is None
        if want is None:
            assert o in (3, 11) and cpu.request.is_nan() and mem.request.is_nan() and mem.limit.is_nan()
            continue
        assert mem.limit == mem.request
        assert float(cpu.request) == pytest.approx(want, rel=1e-9)
        m = sorted(x for samples in h[MEM].values() for x in samples)
        assert mem.request == m[int((len(m) - 1) * Decimal(90) / 100)] * Decimal("1.1")
        slopes_up += want > trend_request(h, 2.5, 0.0)
    assert (slopes_up > 3) == (horizon > 0)
    first = strategy.run(histories[0], None)
    assert first[CPU].request == got[0][CPU].request and first[MEM].request == got[0][MEM].request


def test_exports():
    import krr_amd.api as api

    assert "FleetMoments" in api.__all__ and api.FleetMoments is api.batch.FleetMoments

"""krr_amd.api.batch.FleetBatch.exceedance / FleetExceedance / allocation_thresholds and
examples/sustained_strategy.py without a device, as tests/test_fleet_moments_host.py does it:
``SimpleEngine._exceed_part`` is stood in by the plain restatement (tests/_exceed_ref.py: exact
integers, the excess an exact rational sum rounded ONCE to float64), so that everything above a
launch — threshold forms, caching, chunking with the thresholds sliced alongside, groups of four
rows, pod views, the accessors, ``concat`` and the example strategy — runs here.  The kernel
itself: tests/test_gpu_exceed.py and tests/test_gpu_fleet_exceed.py."""
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from _exceed_ref import INT_FIELDS, exceed_one, np_exceed
from krr_amd.core.models.allocations import ResourceType
from test_fleet_batch_host import N, _histories

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1
ROWS = INT_FIELDS + ("excess",)
nan = np.nan


def exceedance_of(x, taus):
    """A FleetExceedance of one series (NaN = absent slot) and R thresholds from the restatement."""
    from krr_amd.api import FleetExceedance

    x = np.asarray(x, dtype=np.float64)
    thr = np.asarray(taus, dtype=np.float64).reshape(-1, 1)
    r = np_exceed(x, np.array([0, x.size]), thr, gaps=True)
    return FleetExceedance(r["above"], r["excess"], r["longest"], r["head"], r["tail"], r["last"], thr, r["count"],
                           r["flags"].view(np.uint32), np.array([x.size], dtype=np.int64))


@pytest.fixture
def standin(monkeypatch):
    """The launchers stood in; returns the call log: ("exceed", segments of the chunk, rows, the
    thresholds the chunk was given)."""
    import torch

    from _standin import k_table_for
    from krr_amd.core.engine import SimpleEngine
    from oracle import oracle

    calls = []

    def exceed_part(self, ctx, part, thresholds):
        calls.append(("exceed", part.n_segments, thresholds.shape[0], np.array(thresholds)))
        assert thresholds.shape[1] == part.n_segments
        return {k: torch.from_numpy(v) for k, v in
                np_exceed(part.values, part.offsets, thresholds, part.gaps_are_nan).items()}

    def percentiles_part(self, ctx, part, params_list):
        rows = [oracle.percentile(part.values, part.offsets, p.mode, p.p_num, p.p_den, p.q, part.gaps_are_nan,
                                  k_table=k_table_for(part, p)) for p in params_list]
        return {"value": torch.from_numpy(np.stack([r[0] for r in rows])), "count": torch.from_numpy(rows[0][1]),
                "flags": torch.from_numpy(np.stack([r[2] for r in rows]).astype(np.int32))}

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_exceed_part", exceed_part)
    monkeypatch.setattr(SimpleEngine, "_resident", lambda self, part: part)  # the one upload for several groups
    monkeypatch.setattr(SimpleEngine, "_percentiles_part", percentiles_part)
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return np.array([float(x) for samples in h[resource].values() for x in samples])


def _check_rows(ex, histories, resource, thr):
    """Every object and row of ``ex`` against the restatement of the object's flattened samples."""
    for o, h in enumerate(histories):
        x = _flat(h, resource)
        assert ex.count[o] == x.size == ex.slots[o]
        for r in range(thr.shape[0]):
            e = exceed_one(x, thr[r, o])
            assert [getattr(ex, k)[r, o] for k in INT_FIELDS] == [e[k] for k in INT_FIELDS], (o, r)
            assert ex.excess[r, o] == float(e["excess"])  # the stand-in rounds the exact sum once
        assert ex.flags[o] == (EMPTY if x.size == 0 else 0)


# --- FleetBatch.exceedance ----------------------------------------------------------------------
def test_threshold_forms_and_caching(standin, histories, monkeypatch):
    from krr_amd.api import FleetBatch, FleetExceedance, batch as batch_mod

    packed = []
    real = batch_mod.pack_resource
    monkeypatch.setattr(batch_mod, "pack_resource", lambda hs, r: (packed.append(r), real(hs, r))[1])
    b = FleetBatch(histories)
    row = np.linspace(0.02, 0.2, N)
    ex = b.exceedance(CPU, row)
    assert isinstance(ex, FleetExceedance) and ex.above.shape == (1, N) and ex.thresholds.shape == (1, N)
    assert ex.count.shape == ex.flags.shape == ex.slots.shape == (N,) and ex.flags.dtype == np.uint32
    _check_rows(ex, histories, CPU, row[None, :])
    assert b.exceedance(CPU, row.copy()) is ex and b.exceedance(CPU, row[None, :]) is ex  # the same bytes
    assert b.exceedance(CPU, list(row)) is ex and b.exceedance(CPU, [Decimal(repr(float(t))) for t in row]) is ex
    assert packed == [CPU] and [c[:3] for c in standin] == [("exceed", N, 1)]
    # a sequence per object: None and Decimal('NaN') are "no request set"
    mixed = [None if o % 3 == 0 else Decimal("NaN") if o % 3 == 1 else Decimal("0.1") for o in range(N)]
    got = b.exceedance(CPU, mixed)
    want = np.array([nan if o % 3 != 2 else 0.1 for o in range(N)])
    assert np.array_equal(got.thresholds, want[None, :], equal_nan=True) and got is not ex
    assert (got.above[0, np.isnan(want)] == 0).all() and (got.last[0, np.isnan(want)] == -1).all()
    _check_rows(got, histories, CPU, want[None, :])
    # [R, S]: the result's rows, and another resource packs once more
    two = np.stack([np.full(N, 1.9e8), np.full(N, 2.2e8)])
    m = b.exceedance(MEM, two)
    assert m.above.shape == (2, N) and (m.above[0] >= m.above[1]).all() and packed == [CPU, MEM]
    _check_rows(m, histories, MEM, two)
    assert b.exceedance(MEM, two[::-1]) is not m  # other bytes
    assert len(standin) == 4


@pytest.mark.parametrize("bad", [np.zeros(N - 1), np.zeros((2, N + 1)), np.zeros((N, 1)), np.zeros((1, 1, N)),
                                 np.zeros((0, N)), [0.1] * (N + 2), [[0.1] * N]],
                         ids=["short", "wide", "transposed", "3d", "no_rows", "long_list", "nested_list"])
def test_wrong_threshold_shapes_raise(standin, histories, bad):
    from krr_amd.api import FleetBatch

    with pytest.raises(ValueError, match="thresholds"):
        FleetBatch(histories).exceedance(CPU, bad)
    assert standin == []


def test_chunks_slice_the_thresholds_with_the_segments(standin, histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    rng = np.random.default_rng(3)
    thr = {CPU: rng.uniform(0.03, 0.2, (3, N)), MEM: rng.normal(2e8, 2e7, (3, N))}
    whole = FleetBatch(histories, engine=SimpleEngine(0))
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    parts = FleetBatch(histories, engine=small)
    for r in (CPU, MEM):
        a, c = whole.exceedance(r, thr[r]), parts.exceedance(r, thr[r])
        for k in ROWS + ("thresholds", "count", "flags", "slots"):
            assert np.array_equal(getattr(a, k), getattr(c, k), equal_nan=True), k
        _check_rows(c, histories, r, thr[r])  # every object met ITS thresholds
    chunked = [c for c in standin if c[1] < N]
    assert len(chunked) > 8 and sum(c[1] for c in chunked) == 2 * N  # whole segments, every object once per resource
    for r, calls in ((CPU, chunked[:len(chunked) // 2]), (MEM, chunked[len(chunked) // 2:])):
        assert np.array_equal(np.concatenate([c[3] for c in calls], axis=1), thr[r])  # consecutive column ranges


def test_more_than_four_thresholds_run_in_groups(standin, histories):
    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    assert _native.KRR_MAX_THRESHOLDS == 4
    thr = np.linspace(0.01, 0.3, 9)[:, None] * np.linspace(0.5, 1.5, N)[None, :]
    ex = FleetBatch(histories).exceedance(CPU, thr)
    assert ex.above.shape == (9, N) and [c[:3] for c in standin] == [("exceed", N, 4), ("exceed", N, 4), ("exceed", N, 1)]
    assert np.array_equal(np.concatenate([c[3] for c in standin], axis=0), thr)
    _check_rows(ex, histories, CPU, thr)
    del standin[:]
    small = SimpleEngine(0)
    small.chunk_bytes = 1024
    ex2 = FleetBatch(histories, engine=small).exceedance(CPU, thr[:6])
    assert [c[2] for c in standin] == [4, 2] * (len(standin) // 2) and len(standin) > 2  # per chunk: 4 rows, then 2
    for k in ROWS:
        assert np.array_equal(getattr(ex2, k), getattr(ex, k)[:6]), k


def test_per_pod_with_repeated_thresholds(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    pods = b.per_pod(CPU)
    thr = np.linspace(0.05, 0.15, N)
    per_pod = np.repeat(thr, np.diff(pods.pod_groups))
    ex = pods.exceedance(CPU, per_pod)
    kept = [(o, np.array([float(v) for v in x])) for o, h in enumerate(histories) for x in h[CPU].values() if len(x)]
    assert ex.above.shape == (1, len(kept)) and standin[0][:3] == ("exceed", len(kept), 1)
    for j, (o, x) in enumerate(kept):
        e = exceed_one(x, thr[o])
        assert ex.thresholds[0, j] == thr[o]
        assert [getattr(ex, k)[0, j] for k in INT_FIELDS] == [e[k] for k in INT_FIELDS], j
    with pytest.raises(ValueError, match="thresholds"):
        pods.exceedance(CPU, thr)  # one per object is not one per pod


def test_no_device_raises(histories, monkeypatch):
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeUnavailable):
        FleetBatch(histories, engine=SimpleEngine(0)).exceedance(CPU, np.zeros(N))


# --- FleetExceedance ----------------------------------------------------------------------------
def test_accessors():
    x = [1.0, 5.0, 6.0, nan, 1.0, 7.0, nan, nan]
    ex = exceedance_of(x, [2.0, 6.5, 9.0, nan])
    assert ex.count[0] == 5 and ex.slots[0] == 8
    assert ex.above[:, 0].tolist() == [3, 1, 0, 0] and ex.longest[:, 0].tolist() == [2, 1, 0, 0]
    assert ex.head[:, 0].tolist() == [0, 0, 0, 0] and ex.tail[:, 0].tolist() == [1, 1, 0, 0]
    assert ex.last[:, 0].tolist() == [5, 5, -1, -1]
    assert np.array_equal(ex.share[:, 0], [3 / 5, 1 / 5, 0.0, 0.0])
    assert np.array_equal(ex.mean_excess[:, 0], [(3.0 + 4.0 + 5.0) / 3, 0.5, nan, nan], equal_nan=True)
    assert ex.since_last[:, 0].tolist() == [2, 2, -1, -1]
    empty = exceedance_of([nan, nan], [1.0, nan])
    assert empty.flags[0] == EMPTY and np.isnan(empty.share).all() and np.isnan(empty.mean_excess).all()
    assert empty.since_last[:, 0].tolist() == [-1, -1] and empty.excess.tolist() == [[0.0], [0.0]]
    full = exceedance_of([3.0, 4.0], [1.0])
    assert full.share[0, 0] == 1.0 and full.head[0, 0] == full.tail[0, 0] == full.longest[0, 0] == 2
    assert full.since_last[0, 0] == 0 and full.mean_excess[0, 0] == 2.5


def test_allocation_thresholds():
    from types import SimpleNamespace as NS

    from krr_amd.api import allocation_thresholds
    from krr_amd.core.models.allocations import ResourceAllocations

    def obj(req_cpu, lim_cpu, req_mem, lim_mem):
        return NS(allocations=ResourceAllocations(requests={CPU: req_cpu, MEM: req_mem}, limits={CPU: lim_cpu, MEM: lim_mem}))

    objects = [obj("100m", "1", "128Mi", None), obj(None, None, None, "1Gi"), obj(Decimal("NaN"), Decimal("0.5"), Decimal("NaN"), Decimal("NaN"))]
    assert objects[2].allocations.requests[CPU] == "?" == objects[2].allocations.limits[MEM]  # the model's NaN
    assert np.array_equal(allocation_thresholds(objects, CPU), [0.1, nan, nan], equal_nan=True)
    assert np.array_equal(allocation_thresholds(objects, CPU, "limits"), [1.0, nan, 0.5], equal_nan=True)
    assert np.array_equal(allocation_thresholds(objects, MEM, which="requests"), [128.0 * 2 ** 20, nan, nan], equal_nan=True)
    assert np.array_equal(allocation_thresholds(objects, MEM, "limits"), [nan, 2.0 ** 30, nan], equal_nan=True)
    assert allocation_thresholds([], CPU).shape == (0,) and allocation_thresholds(objects, CPU).dtype == np.float64
    with pytest.raises(ValueError, match="requests"):
        allocation_thresholds(objects, CPU, "request")


def _concat_equals_whole(x, taus, k):
    """exceedance(x[:k]).concat(exceedance(x[k:])) against the restatement of x: integers exactly,
    excess within the two sides' summed bounds of the exact sum."""
    a, b = exceedance_of(x[:k], taus), exceedance_of(x[k:], taus)
    got = a.concat(b)
    assert got.slots[0] == len(x) and np.array_equal(got.thresholds, a.thresholds, equal_nan=True)
    for r, tau in enumerate(taus):
        e = exceed_one(x, tau)
        assert got.count[0] == e["count"]
        assert [int(getattr(got, f)[r, 0]) for f in INT_FIELDS] == [e[f] for f in INT_FIELDS], (k, r, tau)
        if isinstance(e["excess"], Fraction):
            bound = exceed_one(x[:k], tau)["bound"] + exceed_one(x[k:], tau)["bound"]
            assert abs(Fraction(float(got.excess[r, 0])) - e["excess"]) <= bound, (k, r, tau)
    assert got.flags[0] == (EMPTY if got.count[0] == 0 else 0)
    return got


def test_concat_cut_at_every_position():
    """A small series with runs at both ends, a run around a hole, an interrupted run and trailing
    gaps, cut everywhere: inside runs, at gaps, and with an empty side."""
    x = np.array([5.0, 5.0, 1.0, nan, 5.0, nan, nan, 5.0, 5.0, 1.0, 5.0, nan, 1.0, nan, 5.0, 5.0, 5.0, nan])
    taus = [2.0, 0.5, 5.0, nan]
    whole = exceedance_of(x, taus)
    assert whole.count[0] == 12  # six of the 18 slots are absent
    assert whole.longest[:, 0].tolist() == [3, 12, 0, 0] and whole.head[:, 0].tolist() == [2, 12, 0, 0]
    for k in range(x.size + 1):
        got = _concat_equals_whole(x, taus, k)
        assert np.array_equal(got.since_last, whole.since_last)
    for gaps_only in ([nan] * 4, []):
        g = exceedance_of(gaps_only, taus)  # an empty side is the identity for the runs; slots still add
        for got, shift in ((whole.concat(g), 0), (g.concat(whole), len(gaps_only))):
            for f in ("above", "longest", "head", "tail", "excess"):
                assert np.array_equal(getattr(got, f), getattr(whole, f)), f
            assert np.array_equal(got.last, np.where(whole.last >= 0, whole.last + shift, -1))
            assert got.slots[0] == x.size + len(gaps_only) and got.flags[0] == 0
    both = exceedance_of([nan], taus).concat(exceedance_of([nan, nan], taus))
    assert both.flags[0] == EMPTY and both.slots[0] == 3 and (both.last == -1).all()


@pytest.mark.parametrize("kind", ["cpu", "memory"])
@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gaps"])
def test_concat_random_cuts(kind, gaps):
    rng = np.random.default_rng(17)
    n = 400
    x = rng.gamma(2.0, 0.05, n) if kind == "cpu" else np.floor(rng.normal(2e8, 2e7, n))
    p = np.sort(x)
    taus = [p[n // 2], p[int(n * 0.9)], p[int(n * 0.99)], p[0] - 1.0]
    if gaps:
        x[rng.random(n) < 0.2] = nan
    for k in [0, 1, n - 1, n] + rng.integers(2, n - 1, 12).tolist():
        _concat_equals_whole(x, taus, k)


def test_concat_folds_day_by_day():
    rng = np.random.default_rng(19)
    days = [rng.gamma(2.0, 0.05, 96) for _ in range(3)]
    days[1][rng.random(96) < 0.25] = nan
    taus, x = [0.1, 0.05], np.concatenate(days)
    for fold in (exceedance_of(days[0], taus).concat(exceedance_of(days[1], taus)).concat(exceedance_of(days[2], taus)),
                 exceedance_of(days[0], taus).concat(exceedance_of(days[1], taus).concat(exceedance_of(days[2], taus)))):
        for r, tau in enumerate(taus):
            e = exceed_one(x, tau)
            assert [int(getattr(fold, f)[r, 0]) for f in INT_FIELDS] == [e[f] for f in INT_FIELDS]
        assert fold.slots[0] == 3 * 96


def test_concat_refuses_other_thresholds_and_merges_flags():
    from krr_amd.api import FleetExceedance

    a = exceedance_of([1.0, 3.0], [2.0, nan])
    assert a.concat(exceedance_of([3.0], [2.0, nan])).above[:, 0].tolist() == [2, 0]  # NaN equals NaN
    for other in ([2.5, nan], [2.0, 1.0], [2.0], [nan, 2.0], [-2.0, nan]):
        with pytest.raises(ValueError, match="thresholds"):
            a.concat(exceedance_of([3.0], other))
    with pytest.raises(ValueError, match="thresholds"):
        exceedance_of([1.0], [0.0]).concat(exceedance_of([1.0], [-0.0]))  # bitwise: 0.0 is not -0.0

    def two(first, second, taus):  # a two-object result
        p, q = exceedance_of(first, taus), exceedance_of(second, taus)
        cat = lambda f: np.concatenate([getattr(p, f), getattr(q, f)], axis=-1)  # noqa: E731
        return FleetExceedance(*(cat(f) for f in ("above", "excess", "longest", "head", "tail", "last", "thresholds",
                                                   "count", "flags", "slots")))

    left, right = two([nan, nan], [3.0, 1.0], [2.0]), two([nan], [nan, 3.0, 3.0], [2.0])
    got = left.concat(right)
    assert got.flags.tolist() == [EMPTY, 0] and got.count.tolist() == [0, 4] and got.slots.tolist() == [3, 5]
    assert got.above[0].tolist() == [0, 3] and got.longest[0].tolist() == [0, 2] and got.last[0].tolist() == [-1, 4]
    flagged = two([3.0], [3.0], [2.0])
    flagged.flags[1], flagged.excess[0, 1] = NAN, nan
    got = flagged.concat(two([3.0], [3.0], [2.0]))
    assert got.flags.tolist() == [0, NAN] and got.excess[0, 0] == 2.0 and np.isnan(got.excess[0, 1])
    with pytest.raises(ValueError, match="same objects"):
        left.concat(exceedance_of([1.0], [2.0]))


# --- examples/sustained_strategy.py -------------------------------------------------------------
def sustained_request(history, percentiles, max_share, max_sustained):
    """The strategy's CPU definition per object by a plain loop (None: no sample)."""
    x = [v for samples in history[CPU].values() for v in samples]
    if not x:
        return None
    ordered = sorted(x)
    cands = [ordered[int((len(x) - 1) * Decimal(p) / 100)] for p in percentiles]
    for c in cands:
        above = [v > c for v in x]
        run = longest = 0
        for a in above:
            run = run + 1 if a else 0
            longest = max(longest, run)
        if sum(above) / len(x) <= max_share and longest <= max_sustained:
            return c
    return cands[-1]


@pytest.mark.parametrize("max_share,max_sustained", [(0.3, 5), (0.3, 1), (0.08, 3), (1.0, 0), (0.0, 100)])
def test_sustained_strategy_equals_a_python_loop(standin, histories, max_share, max_sustained):
    from examples.sustained_strategy import SustainedSettings, SustainedStrategy

    strategy = SustainedStrategy(SustainedSettings(max_share=max_share, max_sustained_slots=max_sustained,
                                                   memory_percentile=Decimal(90), memory_buffer_percentage=Decimal(10)))
    got = strategy.run_batch(histories)
    assert len(got) == N and [c[:3] for c in standin] == [("exceed", N, 4)]  # one launch, four thresholds
    picks = set()
    for o, h in enumerate(histories):
        want = sustained_request(h, (50, 75, 90, 95), max_share, max_sustained)
        cpu, mem = got[o][CPU], got[o][MEM]
        assert cpu.limit is None
        if want is None:
            assert o in (3, 11) and cpu.request.is_nan() and mem.request.is_nan() and mem.limit.is_nan()
            continue
        assert cpu.request == want, o
        ordered = sorted(v for samples in h[CPU].values() for v in samples)
        picks.add(tuple(ordered[int((len(ordered) - 1) * Decimal(p) / 100)] for p in (50, 75, 90, 95)).index(want))
        m = sorted(x for samples in h[MEM].values() for x in samples)
        assert mem.request == m[int((len(m) - 1) * Decimal(90) / 100)] * Decimal("1.1") and mem.limit == mem.request
    if (max_share, max_sustained) == (0.3, 1):
        assert len(picks) >= 3  # the run length decides, not the share alone
    for o in (0, 3, 7):
        first = strategy.run(histories[o], None)
        assert (first[CPU].request == got[o][CPU].request or (first[CPU].request.is_nan() and got[o][CPU].request.is_nan()))
        assert first[MEM].request == got[o][MEM].request or first[MEM].request.is_nan()


def test_exports():
    import krr_amd.api as api
    from krr_amd import _native

    assert {"FleetExceedance", "allocation_thresholds"} <= set(api.__all__)
    assert api.FleetExceedance is api.batch.FleetExceedance and "krr_segmented_exceed" in _native.EXPORTED_SYMBOLS

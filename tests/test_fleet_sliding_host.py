"""krr_amd.api.batch.FleetBatch.sliding / sustained_peak / FleetSliding without a device, as
tests/test_fleet_rollup_host.py does it: ``SimpleEngine._slide_part`` is stood in by the plain
restatement (tests/_slide_ref.py; sum and mean the exact value rounded ONCE to float64), so that
everything above a launch — validation, the ``stats=`` selection, caching, chunking, the
accessors, ``as_batch`` — runs here, and the restatement itself is checked against a brute-force
double loop.  The kernel: tests/test_gpu_slide.py and tests/test_gpu_fleet_sliding.py."""
from fractions import Fraction

import numpy as np
import pytest

from _slide_ref import SCALE, brute_slide, np_peak, np_slide, slide_one, sum_within_bound
from krr_amd.core.models.allocations import ResourceType
from test_fleet_batch_host import N, _histories

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1
ALL = ("mean", "sum", "max", "min", "wcount")
nan, inf = np.nan, float("inf")


def np_sliding(vals, offs, window, min_count, gaps, want=ALL) -> dict:
    """What a launch returns, from the restatement: per-slot arrays for ``want``, peak and slot."""
    vals, offs = np.asarray(vals, dtype=np.float64), np.asarray(offs, dtype=np.int64)
    r = np_slide(vals, offs, window, min_count, gaps, means=True)
    S = offs.size - 1
    peak, slot = np.full(S, nan), np.full(S, -1, np.int64)
    for s in range(S):
        a, b = offs[s], offs[s + 1]
        peak[s], slot[s] = np_peak(r["mean"][a:b], r["emitted"][a:b])
    out = {k: (r[k].astype(np.int32) if k == "wcount" else r[k]) for k in want}
    out.update(peak=peak, peak_slot=slot, count=r["count"], flags=r["flags"].astype(np.int32))
    return out


def sliding_of(series, window, min_count=None, gaps=True, want=ALL):
    """A hand-built FleetSliding of a few series (NaN = absent slot) from the restatement."""
    from krr_amd.api import FleetSliding

    series = [np.asarray(x, dtype=np.float64) for x in series]
    offs = np.concatenate([[0], np.cumsum([x.size for x in series])]).astype(np.int64)
    mc = window if min_count is None else min_count
    r = np_sliding(np.concatenate(series) if series else np.zeros(0), offs, window, mc, gaps, want)
    return FleetSliding(CPU, window, mc, offs, r["count"], r["flags"], r["peak"], r["peak_slot"],
                        {k: r[k] for k in want})


@pytest.fixture
def standin(monkeypatch):
    """The launcher stood in; returns the call log: (segments of the chunk, window, min_count, want)."""
    import torch

    from krr_amd.core.engine import SimpleEngine

    calls = []

    def slide_part(self, ctx, part, window, min_count, want):
        calls.append((part.n_segments, window, min_count, tuple(want)))
        r = np_sliding(part.values, part.offsets, window, min_count, part.gaps_are_nan, want)
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items()}

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_slide_part", slide_part)
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return np.array([float(x) for samples in h[resource].values() for x in samples])


# --- the restatement against a brute-force loop -------------------------------------------------
X = [1.5, nan, -0.0, 0.0, 3.0, nan, nan, -2.0, 0.25, 7.0, nan, inf, 1.0, -inf, 2.0, 0.1, 0.2, 0.3]


@pytest.mark.parametrize("gaps", [True, False])
def test_np_slide_against_brute_force(gaps):
    offs = np.array([0, len(X)])
    for W in (1, 2, 3, 4, 7, len(X), len(X) + 5):
        for mc in sorted({1, -(-W // 2), W}):
            r, brute = np_slide(X, offs, W, mc, gaps, means=True), brute_slide(X, W, mc, gaps)
            for i, b in enumerate(brute):
                assert r["wcount"][i] == b["count"] and r["emitted"][i] == b["emitted"], (W, mc, i)
                t = b["total"]
                if t is None:
                    assert r["exact"][i] is None and np.isnan([r["min"][i], r["max"][i], r["mean"][i]]).all()
                elif isinstance(t, Fraction):
                    assert Fraction(r["exact"][i], SCALE) == t
                    assert r["mean"][i] == float(t / b["count"]) and r["sum"][i] == float(t)
                    assert Fraction(r["mag"][i], SCALE) == sum(abs(Fraction(v)) for v in X[max(0, i - W + 1):i + 1]
                                                                if v == v and abs(v) != inf)
                else:
                    assert np.array_equal(r["exact"][i], t, equal_nan=True)
                    assert np.array_equal(r["mean"][i], t, equal_nan=True)
                for k in ("min", "max"):
                    assert np.array_equal(r[k][i], b[k], equal_nan=True), (W, mc, i, k)
                    assert r[k][i] != 0 or not np.signbit(r[k][i])  # a zero extremum is +0.0


def test_bound_check_in_integers():
    x = [0.1, 0.2, 0.3]
    w = slide_one(x, 3, False)
    e, mag = w["total"][2], w["mag"][2]
    assert sum_within_bound(0.1 + 0.2 + 0.3, e, mag, 3) and sum_within_bound(0.3 + 0.2 + 0.1, e, mag, 3)
    assert not sum_within_bound(0.6000000000000003, e, mag, 3) and not sum_within_bound(nan, e, mag, 3)
    assert sum_within_bound(0.1, w["total"][0], w["mag"][0], 1) and not sum_within_bound(0.1000000000000001, w["total"][0], w["mag"][0], 1)


def test_np_peak_rules():
    assert np_peak([1.0, 3.0, 3.0, 2.0], [True] * 4) == (3.0, 1)
    assert np_peak([5.0, 3.0], [False, True]) == (3.0, 1)
    p, at = np_peak([1.0, nan, 9.0, nan], [True] * 4)
    assert np.isnan(p) and at == 1
    p, at = np_peak([nan, 2.0], [False, False])
    assert np.isnan(p) and at == -1
    p, at = np_peak([-0.0, 0.0], [True, True])
    assert p == 0 and not np.signbit(p) and at == 0
    assert np_peak([1.0, inf, inf], [True] * 3) == (inf, 1)


# --- validation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, -3, 2.0, "5", None, True])
def test_bad_window_raises(standin, histories, window):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    with pytest.raises(ValueError, match="window"):
        b.sliding(CPU, window)
    with pytest.raises(ValueError, match="window"):
        b.sustained_peak(CPU, window)
    assert standin == []


def test_window_above_the_cap_points_to_rollup(standin, histories):
    from krr_amd import _native
    from krr_amd.api import FleetBatch

    cap = _native.KRR_SLIDE_MAX_WINDOW
    assert cap >= 1440
    with pytest.raises(ValueError, match=r"(?s)KRR_SLIDE_MAX_WINDOW.*rollup"):
        FleetBatch(histories).sliding(CPU, cap + 1)
    FleetBatch(histories).sliding(CPU, cap, min_count=1)
    assert len(standin) == 1


@pytest.mark.parametrize("min_count", [0, -1, 6, 2.0, "3", True])
def test_bad_min_count_raises(standin, histories, min_count):
    from krr_amd.api import FleetBatch

    with pytest.raises(ValueError, match="min_count"):
        FleetBatch(histories).sliding(CPU, 5, min_count)
    assert standin == []


def test_bad_stats_raise(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    for stats in (("median",), ("mean", "p95"), "count"):
        with pytest.raises(ValueError, match="stats="):
            b.sliding(CPU, 5, stats=stats)
    assert standin == []
    sl = b.sliding(CPU, 5, stats=("mean", "wcount"))
    assert sl.stats == ("mean", "wcount")
    for call in (lambda: sl.of(0, "max"), lambda: sl.dense("sum"), lambda: sl.tensor("min"), lambda: sl.as_batch("max")):
        with pytest.raises(ValueError, match="stats="):
            call()
    for call in (lambda: sl.of(0, "median"), lambda: sl.as_batch("wcount")):
        with pytest.raises(ValueError, match="stat"):
            call()
    with pytest.raises(IndexError):
        sl.of(N, "mean")


def test_no_device_raises(histories, monkeypatch):
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeUnavailable):
        FleetBatch(histories, engine=SimpleEngine(0)).sliding(CPU, 5)


# --- FleetBatch.sliding above the launch --------------------------------------------------------
def test_stats_selection_reaches_the_launch_and_is_cached(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    sl = b.sliding(CPU, 4)
    assert standin == [(N, 4, 4, ("mean",))] and sl.window == 4 and sl.min_count == 4  # min_count=None: the window
    assert b.sliding(CPU, 4) is sl and b.sliding(CPU, 4, 4, stats="mean") is sl and len(standin) == 1
    assert b.sliding(CPU, 4, 2) is not sl and standin[-1] == (N, 4, 2, ("mean",))
    al = b.sliding(CPU, 4, stats=("wcount", "min", "sum", "mean", "max"))  # any order: the kernel's
    assert standin[-1] == (N, 4, 4, ALL) and al.stats == ALL
    pk = b.sustained_peak(CPU, 4)
    assert standin[-1] == (N, 4, 4, ()) and len(standin) == 4
    assert np.array_equal(pk, sl.peak, equal_nan=True) and np.array_equal(pk, al.peak, equal_nan=True)
    p2, at = b.sustained_peak(CPU, 4, return_slot=True)
    assert len(standin) == 4 and p2 is pk and np.array_equal(at, sl.peak_slot)


def test_chunks_give_the_result_of_one_chunk(standin, histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    whole = FleetBatch(histories, engine=SimpleEngine(0)).sliding(CPU, 4, 2, stats=ALL)
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    del standin[:]
    parts = FleetBatch(histories, engine=small).sliding(CPU, 4, 2, stats=ALL)
    assert len(standin) > 4 and sum(c[0] for c in standin) == N
    assert np.array_equal(parts.offsets, whole.offsets) and parts.offsets[0] == 0
    for k in ALL:
        assert np.array_equal(parts._flat(k), whole._flat(k), equal_nan=True), k
    for k in ("count", "flags", "slots", "peak_slot"):
        assert np.array_equal(getattr(parts, k), getattr(whole, k)), k
    assert np.array_equal(parts.peak, whole.peak, equal_nan=True)
    for o, h in enumerate(histories):
        x = _flat(h, CPU)
        assert whole.slots[o] == x.size and whole.flags[o] == (EMPTY if x.size == 0 else 0)
        brute = brute_slide(x, 4, 2, False)
        assert whole.of(o, "wcount").tolist() == [b["count"] for b in brute]
        assert np.array_equal(whole.of(o, "sum"), [float(b["total"]) if b["emitted"] else nan for b in brute],
                              equal_nan=True)
        means = [float(b["total"] / b["count"]) if b["emitted"] else nan for b in brute]
        assert np.array_equal(whole.of(o, "mean"), means, equal_nan=True)
        live = [m for m in means if m == m]
        assert (whole.peak[o] == max(live) and means[whole.peak_slot[o]] == max(live)) if live else \
            (np.isnan(whole.peak[o]) and whole.peak_slot[o] == -1)


def test_per_pod_view_slides_per_pod(standin, histories):
    from krr_amd.api import FleetBatch

    pods = FleetBatch(histories).per_pod(CPU)
    sl = pods.sliding(CPU, 3, 1, stats=("max",))
    j = 0
    for h in histories:
        for samples in h[CPU].values():
            if not len(samples):
                continue  # a pod without samples has no segment in the pod view
            x = np.array([float(v) for v in samples])
            assert sl.of(j, "max").tolist() == [b["max"] for b in brute_slide(x, 3, 1, False)]
            j += 1
    assert j == sl.n_objects == pods.n_objects


# --- FleetSliding on hand-built results ---------------------------------------------------------
SERIES = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [], [nan, nan, 9.0], [4.0, nan, nan, nan, nan, 6.0, 2.0, 8.0, 1.0, 3.0, 5.0]]


def test_of_and_flat_arrays():
    sl = sliding_of(SERIES, 3, 2)
    assert sl.offsets.tolist() == [0, 7, 7, 10, 21] and sl.slots.tolist() == [7, 0, 3, 11]
    assert sl.count.tolist() == [7, 0, 1, 7] and sl.flags.tolist() == [0, EMPTY, 0, 0]
    assert np.array_equal(sl.of(0, "mean"), [nan, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0], equal_nan=True)
    assert np.array_equal(sl.of(0, "sum"), [nan, 3.0, 6.0, 9.0, 12.0, 15.0, 18.0], equal_nan=True)
    assert sl.of(0, "wcount").tolist() == [1, 2, 3, 3, 3, 3, 3]
    assert sl.of(1).size == 0
    assert np.isnan(sl.of(2, "mean")).all() and sl.of(2, "wcount").tolist() == [0, 0, 1]
    assert np.array_equal(sl.of(3, "max"), [nan, nan, nan, nan, nan, nan, 6.0, 8.0, 8.0, 8.0, 5.0], equal_nan=True)
    assert np.array_equal(sl.of(3, "min"), [nan, nan, nan, nan, nan, nan, 2.0, 2.0, 1.0, 1.0, 1.0], equal_nan=True)
    assert sl.peak.tolist()[0] == 6.0 and sl.peak_slot.tolist() == [6, -1, -1, 7]
    assert sl.peak[3] == 16.0 / 3 and np.isnan(sl.peak[1]) and np.isnan(sl.peak[2])
    full = sliding_of(SERIES, 3)  # min_count=None: full windows only
    assert full.min_count == 3 and np.isnan(full.of(0, "mean")[:2]).all() and full.of(0, "mean")[2] == 2.0


def test_dense_is_right_justified():
    sl = sliding_of(SERIES, 3, 1, want=("max", "wcount"))
    d = sl.dense("max")
    assert d.shape == (4, 11)
    assert np.array_equal(d[0], [nan] * 4 + [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], equal_nan=True)
    assert np.isnan(d[1]).all() and np.array_equal(d[2], [nan] * 10 + [9.0], equal_nan=True)
    assert np.array_equal(sl.dense("wcount")[3], [1, 1, 1, 0, 0, 1, 2, 3, 3, 3, 3])
    assert sliding_of([], 3, 1).dense("max").shape == (0, 0)


def test_as_batch_is_a_gapped_series_over_the_same_offsets():
    sl = sliding_of(SERIES, 3, 2)
    for stat in ("mean", "sum", "max", "min"):
        b = sl.as_batch(stat)
        assert sl.as_batch(stat) is b and b.n_objects == 4
        ps = b.series(CPU)
        assert ps.gaps_are_nan and np.array_equal(ps.offsets, sl.offsets) and ps.max_len == 11
        assert np.array_equal(np.asarray(ps.values), sl._flat(stat), equal_nan=True), stat
    with pytest.raises(KeyError):
        sl.as_batch("mean").series(MEM)


def test_as_batch_refuses_a_nan_object():
    sl = sliding_of([[1.0, nan, 3.0, 4.0]], 2, 1, gaps=False)
    assert sl.flags.tolist() == [NAN] and np.isnan(sl.peak[0]) and sl.peak_slot[0] == 1
    assert np.array_equal(sl.of(0, "mean"), [1.0, nan, nan, 3.5], equal_nan=True)
    with pytest.raises(ValueError, match="NaN"):
        sl.as_batch("mean")


def test_a_burst_across_the_rollup_grid(standin, histories):
    """The reason the feature exists, on the host: five slots at 10 that straddle the 5-slot grid."""
    x = np.zeros(20)
    x[3:8] = 10.0
    sl = sliding_of([x], 5, gaps=False)
    assert sl.peak[0] == 10.0 and sl.peak_slot[0] == 7
    grid = x.reshape(4, 5).mean(axis=1)
    assert grid.max() == 6.0 < sl.peak[0]


def test_inconsistent_hand_built_sliding_raises():
    from krr_amd.api import FleetSliding

    z = np.zeros(3)
    with pytest.raises(ValueError, match="same slots"):
        FleetSliding(CPU, 2, 1, [0, 4], [4], [0], [1.0], [0], {"mean": z})
    with pytest.raises(ValueError, match="stat"):
        FleetSliding(CPU, 2, 1, [0, 3], [3], [0], [1.0], [0], {"median": z})


def test_exports():
    import krr_amd.api as api
    from krr_amd import _native

    assert "FleetSliding" in api.__all__ and api.FleetSliding is api.batch.FleetSliding
    assert "krr_segmented_slide" in _native.EXPORTED_SYMBOLS
    assert "concat" not in dir(api.FleetSliding) and "cannot be merged" in api.FleetSliding.__doc__
    assert "on this window grid" in api.FleetRollup.peak.__doc__

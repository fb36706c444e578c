"""krr_amd.api.batch.FleetBatch.rollup / FleetRollup / FleetProfile without a device, as
tests/test_fleet_exceed_host.py does it: ``SimpleEngine._rollup_part`` is stood in by the plain
restatement (tests/_rollup_ref.py; the sum an exact rational rounded ONCE to float64), so that
everything above a launch — validation, caching, chunking with the window offsets rebased, the
accessors, ``dense``, ``fold`` — runs here, and the restatement itself is checked against a
brute-force loop.  The kernel: tests/test_gpu_rollup.py and tests/test_gpu_fleet_rollup.py."""
from fractions import Fraction

import numpy as np
import pytest

from _rollup_ref import END, START, brute_window_of, np_rollup, rollup_one, window_bounds
from krr_amd.core.models.allocations import ResourceType
from test_fleet_batch_host import N, _histories

CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN = 4, 1
ALIGNS = {"start": START, "end": END}
nan = np.nan


def rollup_of(series, window, align, gaps=True):
    """A hand-built FleetRollup of a few series (NaN = absent slot) from the restatement."""
    from krr_amd.api import FleetRollup

    series = [np.asarray(x, dtype=np.float64) for x in series]
    offs = np.concatenate([[0], np.cumsum([x.size for x in series])]).astype(np.int64)
    r = np_rollup(np.concatenate(series) if series else np.zeros(0), offs, window, ALIGNS[align], gaps)
    return FleetRollup(CPU, window, align, r["offsets"], np.diff(offs), r["count"], r["flags"],
                       r["wcount"].astype(np.int32), r["min"], r["max"], r["sum"])


@pytest.fixture
def standin(monkeypatch):
    """The launcher stood in; returns the call log: (segments of the chunk, window, align)."""
    import torch

    from krr_amd.core.engine import SimpleEngine

    calls = []

    def rollup_part(self, ctx, part, window, align):
        calls.append((part.n_segments, window, align))
        r = np_rollup(part.values, part.offsets, window, align, part.gaps_are_nan)
        out = {"wcount": torch.from_numpy(r["wcount"].astype(np.int32)), "count": torch.from_numpy(r["count"]),
               "flags": torch.from_numpy(r["flags"].astype(np.int32))}
        out.update({k: torch.from_numpy(r[k]) for k in ("min", "max", "sum")})
        return out, r["offsets"]

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_rollup_part", rollup_part)
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return np.array([float(x) for samples in h[resource].values() for x in samples])


# --- the restatement against a brute-force loop -------------------------------------------------
@pytest.mark.parametrize("align", list(ALIGNS))
def test_window_bounds_against_a_walk(align):
    for L in range(0, 14):
        for W in range(1, 16):
            b = window_bounds(L, W, ALIGNS[align])
            assert len(b) == -(-L // W)
            owner = [brute_window_of(i, L, W, ALIGNS[align]) for i in range(L)]
            for w, (lo, hi) in enumerate(b):
                assert owner[lo:hi] == [w] * (hi - lo) and 0 < hi - lo <= W, (L, W, w)
            assert sum(hi - lo for lo, hi in b) == L
            full = [hi - lo == W for lo, hi in b]
            assert all(full[1:] if align == "end" else full[:-1])  # only the first / the last may be partial


def test_rollup_one_against_brute_force():
    x = [1.5, nan, -0.0, 0.0, 3.0, nan, nan, -2.0, 0.25, 7.0, nan]
    for gaps in (True, False):
        for align in ALIGNS.values():
            for W in (1, 2, 3, 4, 11, 12):
                wins = rollup_one(x, W, align, gaps)
                for w, e in enumerate(wins):
                    xs = [v for i, v in enumerate(x) if brute_window_of(i, len(x), W, align) == w]
                    pres = [v for v in xs if v == v]
                    if not gaps and len(pres) != len(xs):
                        assert e["nan"] and e["count"] == len(xs) and np.isnan([e["min"], e["max"], e["exact"]]).all()
                        continue
                    assert e["count"] == len(pres) and not e["nan"]
                    assert e["exact"] == sum((Fraction(v) for v in pres), Fraction(0))
                    if pres:
                        assert e["min"] == min(pres) and e["max"] == max(pres)
                        for k in ("min", "max"):  # a zero extremum is +0.0
                            assert e[k] != 0 or np.signbit(e[k]) == False  # noqa: E712
                    else:
                        assert np.isnan(e["min"]) and np.isnan(e["max"]) and e["exact"] == 0
                    m = len(pres)
                    u = Fraction(1, 2 ** 53)
                    want = (m - 1) * u / (1 - (m - 1) * u) * sum(abs(Fraction(v)) for v in pres) if m > 1 else 0
                    assert e["bound"] == want


def test_np_rollup_flags_and_capacity():
    vals = np.array([1.0, nan, 2.0, 3.0, 4.0, 5.0])
    offs = np.array([0, 0, 2, 6])
    r = np_rollup(vals, offs, 2, END, gaps=False)
    assert r["offsets"].tolist() == [0, 0, 1, 3] and r["flags"].tolist() == [EMPTY, NAN, 0]
    assert r["wcount"].tolist() == [2, 2, 2] and np.isnan(r["sum"][0]) and r["sum"][1:].tolist() == [5.0, 9.0]
    g = np_rollup(vals, offs, 2, END, gaps=True, win_offsets=[0, 0, 1, 2])
    assert g["flags"].tolist() == [EMPTY, 0, 2] and g["written"].tolist() == [True, False]


# --- validation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, -3, 2.0, "5", None, True, 2 ** 31])
def test_bad_window_raises(standin, histories, window):
    from krr_amd.api import FleetBatch

    with pytest.raises(ValueError, match="window"):
        FleetBatch(histories).rollup(CPU, window)
    assert standin == []


def test_bad_align_stat_and_period_raise(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    with pytest.raises(ValueError, match="align"):
        b.rollup(CPU, 5, align="middle")
    ru = b.rollup(CPU, 5)
    for call in (lambda: ru.of(0, "median"), lambda: ru.dense("p95"), lambda: ru.as_batch("wcount"),
                 lambda: ru.as_batch("count"), lambda: ru.peak("nope")):
        with pytest.raises(ValueError, match="stat"):
            call()
    for period in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="period"):
            ru.fold(period)
    with pytest.raises(IndexError):
        ru.of(N, "mean")


def test_no_device_raises(histories, monkeypatch):
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeUnavailable):
        FleetBatch(histories, engine=SimpleEngine(0)).rollup(CPU, 5)


# --- FleetBatch.rollup above the launch ---------------------------------------------------------
@pytest.mark.parametrize("align", list(ALIGNS))
def test_rollup_caches_and_chunks_rebase_the_offsets(standin, histories, align):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    whole = FleetBatch(histories, engine=SimpleEngine(0))
    ru = whole.rollup(CPU, 4, align)
    assert whole.rollup(CPU, 4, align) is ru and len(standin) == 1  # cached per (resource, window, align)
    assert whole.rollup(CPU, 4, "start" if align == "end" else "end") is not ru and len(standin) == 2
    assert whole.rollup(CPU, 3, align) is not ru and len(standin) == 3
    assert ru.window == 4 and ru.align == align and ru.n_objects == N
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    del standin[:]
    parts = FleetBatch(histories, engine=small).rollup(CPU, 4, align)
    assert len(standin) > 4 and sum(c[0] for c in standin) == N
    assert np.array_equal(parts.offsets, ru.offsets) and parts.offsets[0] == 0
    for k in ("wcount", "min", "max", "sum", "mean"):
        assert np.array_equal(getattr(parts, k), getattr(ru, k), equal_nan=True), k
    for k in ("count", "flags", "slots", "n_windows"):
        assert np.array_equal(getattr(parts, k), getattr(ru, k)), k
    for o, h in enumerate(histories):
        x = _flat(h, CPU)
        wins = rollup_one(x, 4, ALIGNS[align], False)
        assert ru.n_windows[o] == len(wins) == -(-x.size // 4) and ru.slots[o] == x.size
        assert ru.of(o, "wcount").tolist() == [e["count"] for e in wins]
        assert ru.of(o, "sum").tolist() == [float(e["exact"]) for e in wins]
        assert ru.of(o, "mean").tolist() == [float(e["exact"]) / e["count"] for e in wins]
        assert ru.flags[o] == (EMPTY if x.size == 0 else 0)


def test_per_pod_view_rolls_up_per_pod(standin, histories):
    from krr_amd.api import FleetBatch

    pods = FleetBatch(histories).per_pod(CPU)
    ru = pods.rollup(CPU, 3, "start")
    j = 0
    for h in histories:
        for samples in h[CPU].values():
            if not len(samples):
                continue  # a pod without samples has no segment in the pod view
            x = np.array([float(v) for v in samples])
            assert ru.of(j, "max").tolist() == [e["max"] for e in rollup_one(x, 3, START, False)]
            j += 1
    assert j == ru.n_objects == pods.n_objects


# --- FleetRollup on hand-built results ----------------------------------------------------------
SERIES = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [], [nan, nan, 9.0], [4.0, nan, nan, nan, nan, 6.0, 2.0, 8.0, 1.0, 3.0, 5.0]]


def test_of_and_flat_arrays():
    ru = rollup_of(SERIES, 3, "end")
    assert ru.offsets.tolist() == [0, 3, 3, 4, 8] and ru.n_windows.tolist() == [3, 0, 1, 4]
    assert ru.slots.tolist() == [7, 0, 3, 11] and ru.count.tolist() == [7, 0, 1, 7]
    assert ru.flags.tolist() == [0, EMPTY, 0, 0]
    assert ru.of(0, "sum").tolist() == [1.0, 9.0, 18.0] and ru.of(0, "wcount").tolist() == [1, 3, 3]
    assert ru.of(0, "mean").tolist() == [1.0, 3.0, 6.0]
    assert ru.of(1, "mean").size == 0
    assert ru.of(2, "min").tolist() == [9.0]
    assert np.array_equal(ru.of(3, "mean"), [4.0, nan, (8.0 + 6.0 + 2.0) / 3, 3.0], equal_nan=True)
    assert np.array_equal(ru.of(3, "max"), [4.0, nan, 8.0, 5.0], equal_nan=True)
    assert ru.of(3, "sum").tolist() == [4.0, 0.0, 16.0, 9.0] and ru.of(3, "wcount").tolist() == [1, 0, 3, 3]
    st = rollup_of(SERIES, 3, "start")
    assert st.of(0, "sum").tolist() == [6.0, 15.0, 7.0] and st.of(0, "wcount").tolist() == [3, 3, 1]
    assert st.mean.size == st.offsets[-1] == 8


def test_dense_is_justified_by_align():
    end, start = rollup_of(SERIES, 3, "end"), rollup_of(SERIES, 3, "start")
    d = end.dense("sum")
    assert d.shape == (4, 4)
    assert np.array_equal(d, [[nan, 1.0, 9.0, 18.0], [nan] * 4, [nan, nan, nan, 9.0], [4.0, 0.0, 16.0, 9.0]], equal_nan=True)
    d = start.dense("sum")
    assert np.array_equal(d[0], [6.0, 15.0, 7.0, nan], equal_nan=True)
    assert np.array_equal(d[2], [9.0, nan, nan, nan], equal_nan=True)
    assert np.array_equal(end.dense("wcount")[3], [1, 0, 3, 3])
    assert np.array_equal(end.dense()[0], [nan, 1.0, 3.0, 6.0], equal_nan=True)  # mean by default
    assert rollup_of([], 3, "end").dense("max").shape == (0, 0)


def _np_fold(ru, period):
    """``fold`` restated with loops: window j of an object with nw windows goes to column j % period
    ("start") or to the column counted back from period - 1 ("end")."""
    S = ru.n_objects
    cnt = np.zeros((S, period), np.int64)
    mn, mx, sm = np.full((S, period), nan), np.full((S, period), nan), np.zeros((S, period))
    for s in range(S):
        nw = int(ru.n_windows[s])
        for j in range(nw):
            c = j % period if ru.align == "start" else period - 1 - (nw - 1 - j) % period
            n = int(ru.of(s, "wcount")[j])
            if n == 0:
                continue
            lo, hi = ru.of(s, "min")[j], ru.of(s, "max")[j]
            mn[s, c] = lo if cnt[s, c] == 0 else min(mn[s, c], lo)
            mx[s, c] = hi if cnt[s, c] == 0 else max(mx[s, c], hi)
            sm[s, c] += ru.of(s, "sum")[j]
            cnt[s, c] += n
    return cnt, mn, mx, sm


@pytest.mark.parametrize("align", list(ALIGNS))
@pytest.mark.parametrize("window,period", [(1, 1), (1, 4), (2, 3), (3, 2), (2, 24), (5, 1)])
def test_fold_against_loops(align, window, period):
    rng = np.random.default_rng(23)
    series = [np.floor(rng.normal(200, 20, n)) for n in (0, 1, 5, 24, 25, 47, 96)]  # integers: sums are exact
    for x in series:
        x[rng.random(x.size) < 0.3] = nan
    series.append(np.full(9, nan))
    ru = rollup_of(series, window, align)
    p = ru.fold(period)
    cnt, mn, mx, sm = _np_fold(ru, period)
    assert p.count.shape == (len(series), period) and p.count.dtype == np.int64
    assert np.array_equal(p.count, cnt) and np.array_equal(p.sum, sm)
    assert np.array_equal(p.min, mn, equal_nan=True) and np.array_equal(p.max, mx, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(p.mean, np.where(cnt > 0, sm / np.where(cnt > 0, cnt, 1), nan), equal_nan=True)
    assert p.count.sum() == ru.count.sum()


def test_fold_puts_the_last_window_last_for_end_and_the_first_first_for_start():
    x = [np.arange(1.0, 8.0), np.arange(10.0, 13.0)]  # 7 and 3 windows of one slot
    e = rollup_of(x, 1, "end").fold(4)
    assert e.max[:, 3].tolist() == [7.0, 12.0] and e.count[0].tolist() == [1, 2, 2, 2] and e.count[1].tolist() == [0, 1, 1, 1]
    assert e.min[0].tolist() == [4.0, 1.0, 2.0, 3.0] and np.isnan(e.min[1, 0]) and e.sum[1, 0] == 0
    s = rollup_of(x, 1, "start").fold(4)
    assert s.min[:, 0].tolist() == [1.0, 10.0] and s.count[0].tolist() == [2, 2, 2, 1] and s.count[1].tolist() == [1, 1, 1, 0]


def test_fold_propagates_a_nan_window():
    ru = rollup_of([[1.0, nan, 3.0, 4.0]], 1, "start", gaps=False)
    assert ru.flags.tolist() == [NAN]
    p = ru.fold(2)
    assert p.count.tolist() == [[2, 2]] and p.sum[0, 0] == 4.0 and np.isnan([p.sum[0, 1], p.min[0, 1], p.max[0, 1]]).all()
    with pytest.raises(ValueError, match="NaN"):
        ru.as_batch("mean")


def test_as_batch_is_a_gapped_series_over_the_window_offsets():
    ru = rollup_of(SERIES, 3, "end")
    for stat in ("min", "max", "sum", "mean"):
        b = ru.as_batch(stat)
        assert ru.as_batch(stat) is b and b.n_objects == 4
        ps = b.series(CPU)
        assert ps.gaps_are_nan and np.array_equal(ps.offsets, ru.offsets) and ps.max_len == 4
        want = getattr(ru, stat).copy()
        want[ru.wcount == 0] = nan  # an empty window is an absent slot, for the sum too
        assert np.array_equal(np.asarray(ps.values), want, equal_nan=True), stat
    with pytest.raises(KeyError):
        ru.as_batch("mean").series(MEM)


def test_inconsistent_hand_built_rollup_raises():
    from krr_amd.api import FleetRollup

    z = np.zeros(3)
    with pytest.raises(ValueError, match="same windows"):
        FleetRollup(CPU, 2, "end", [0, 2], [4], [4], [0], np.zeros(3, np.int32), z, z, z)
    with pytest.raises(ValueError, match="align"):
        FleetRollup(CPU, 2, "centre", [0, 3], [6], [6], [0], np.zeros(3, np.int32), z, z, z)


def test_exports():
    import krr_amd.api as api
    from krr_amd import _native

    assert {"FleetRollup", "FleetProfile"} <= set(api.__all__)
    assert "krr_segmented_rollup" in _native.EXPORTED_SYMBOLS
    assert (_native.KRR_ROLLUP_START, _native.KRR_ROLLUP_END) == (0, 1)
    assert "concat" not in dir(api.FleetRollup) and "concat" in api.FleetRollup.__doc__  # out of scope, and said so

"""The weighted percentile without a device: the restatement (tests/_wquantile_ref.py) against
numpy's weighted ``inverted_cdf`` and the unit-weight identity, the weight tables
(``decay_weights`` / ``window_weights``), and everything ``FleetBatch.weighted_percentile`` does
above a launch — validation, caching, chunking, pod views, ``to_decimal`` and
examples/recency_strategy.py — with ``SimpleEngine._wquantile_part`` stood in by the restatement,
as tests/test_fleet_exceed_host.py stands in ``_exceed_part``.  The kernel itself:
tests/test_gpu_wquantile.py and tests/test_gpu_fleet_wquantile.py."""
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from _wquantile_ref import EMPTY, QNAN, bits, fraction_of, np_wquantile, okey, weights_of, wquantile_one
from krr_amd.api import decay_weights, window_weights  # noqa: F401  (the feature: absent, nothing here runs)
from krr_amd.core.models.allocations import ResourceType
from test_fleet_batch_host import N, _histories, _np_stats

CPU, MEM = ResourceType.CPU, ResourceType.Memory


def _value(b: int) -> float:
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


# --- the restatement ----------------------------------------------------------------------------
def test_okey_orders_like_the_floats():
    xs = [-math.inf, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, 1e300, math.inf]
    keys = [okey(bits(v)) for v in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)  # -0.0 before +0.0


@pytest.mark.parametrize("kind", ["gamma", "integers"])
def test_restatement_equals_numpy_inverted_cdf(kind):
    """Away from knife edges (numpy's float CDF may round either way there): the target W q is kept
    at least 1e-9 W from every cumulative weight."""
    rng = np.random.default_rng(11)
    checked = 0
    for _ in range(300):
        n = int(rng.integers(1, 200))
        x = rng.gamma(2.0, 0.05, n) if kind == "gamma" else np.floor(rng.normal(50, 5, n))  # integers: many ties
        table = rng.integers(0, 1000, int(rng.integers(1, 250))).astype(np.uint64)
        w = np.array(weights_of(n, table), dtype=np.float64)
        if w.sum() == 0:
            continue
        p = Decimal(int(rng.integers(1, 10000))) / 100
        cdf = np.cumsum(w[np.argsort(x, kind="stable")]) / w.sum()
        if np.abs(cdf - float(p) / 100).min() < 1e-9:
            continue
        b, W = wquantile_one(x, table, *fraction_of(p))
        assert W == int(w.sum())
        assert _value(b) == np.quantile(x, float(p) / 100, weights=w, method="inverted_cdf")
        checked += 1
    assert checked > 250


def test_unit_weights_are_the_ceil_rank():
    rng = np.random.default_rng(12)
    for n in (1, 2, 3, 10, 99, 100, 101):
        x = rng.gamma(2.0, 0.05, n)
        for p in ("0.000000001", "1", "33.3", "50", "99", "99.999", "100"):
            num, den = fraction_of(p)
            b, W = wquantile_one(x, [1], num, den)
            k = -(-n * num // (100 * den)) - 1  # ceil(n p / 100) - 1
            assert W == n and _value(b) == np.sort(x)[k], (n, p)


def test_rule_details():
    # the knife edge: C * den == W * num takes the LOWER sample (>=, not >)
    x = np.arange(100, dtype=np.float64)
    assert _value(wquantile_one(x, [1], 50, 1)[0]) == 49.0
    assert _value(wquantile_one(x, [1], 5000001, 100000)[0]) == 50.0
    # age: the last slot is age 0; a table shorter than the series repeats its last entry
    assert _value(wquantile_one([1.0, 2.0, 3.0], [0, 0, 5], 50, 1)[0]) == 1.0
    assert _value(wquantile_one([1.0, 2.0, 3.0], [5, 0], 50, 1)[0]) == 3.0
    assert wquantile_one([1.0, 2.0, 3.0, 4.0], [0, 7], 100, 1) == (bits(3.0), 21)
    # a zero-weight sample is never the answer; equal keys count together; -0.0 before +0.0
    assert _value(wquantile_one([9.0, 1.0], [1, 0], 1, 10**9)[0]) == 1.0
    assert wquantile_one([0.0, -0.0], [1], 50, 1)[0] == bits(-0.0) and wquantile_one([-0.0, 0.0], [1], 51, 1)[0] == bits(0.0)
    assert wquantile_one([np.nan, 2.0, np.nan], [3], 50, 1) == (bits(2.0), 3)  # NaN: an absent slot
    assert wquantile_one([], [1], 50, 1) == (QNAN, 0) and wquantile_one([1.0, 2.0], [0], 50, 1) == (QNAN, 0)
    r = np_wquantile([1.0, np.nan, 3.0, 5.0], [0, 3, 3, 4], [1], 50, 1, gaps=False)  # a NaN sample, empty, one sample
    assert r["flags"].tolist() == [1, 4, 0] and r["wsum"].tolist() == [0, 0, 1] and r["count"].tolist() == [3, 0, 1]


def test_sorted_once_equals_the_plain_loop():
    """``Sorted`` (what the GPU tests ask, many questions per series) against ``wquantile_one``."""
    from _wquantile_ref import Sorted

    rng = np.random.default_rng(13)
    for i in range(120):
        n = int(rng.integers(0, 300))
        x = rng.gamma(2.0, 0.05, n) if i % 3 else np.floor(rng.normal(0, 3, n))  # ties and both zeros' neighbours
        if i % 4 == 0:
            x[rng.random(n) < 0.3] = np.nan
        if i % 5 == 0 and n > 4:
            x[:4] = [0.0, -0.0, np.inf, -np.inf]
        s = Sorted(x)
        for table in ([1], [0], [3, 0, 2], rng.integers(0, 2 ** 32 + 1, 40).astype(np.uint64), np.arange(400, dtype=np.uint64)):
            for p in ("0.000000001", "50", "99", "100", str(rng.integers(1, 10000) / 100)):
                assert s.answer(table, *fraction_of(p)) == wquantile_one(x, table, *fraction_of(p)), (i, p)


# --- the tables ---------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2, 3, 7, 60, 64, 700, 1440])
def test_decay_weights(h):
    from krr_amd.api import decay_weights

    n = 34 * h + 5
    w = decay_weights(h, n)
    assert w.dtype == np.uint64 and w.shape == (n,)
    assert [int(w[k * h]) for k in range(34)] == [2 ** (32 - k) if k <= 32 else 0 for k in range(34)]  # exact powers
    assert (np.diff(w.astype(np.int64)) <= 0).all()  # never increases
    assert w[32 * h] == 1 and (w[32 * h + 1:] == 0).all()  # the zero tail
    for a in sorted({1, h - 1, h + 1, 5 * h // 2, 31 * h + 1} & set(range(1, n))):
        v, e = int(w[a]), 32 * h - a  # floor(2^(e / h)) exactly: v^h <= 2^e < (v + 1)^h
        assert v ** h <= 2 ** e < (v + 1) ** h, a
    assert np.array_equal(decay_weights(h, 10), w[:10]) and decay_weights(np.int64(h), 3).dtype == np.uint64


def test_window_weights_and_bad_table_arguments():
    from krr_amd.api import decay_weights, window_weights

    w = window_weights(3, 7)
    assert w.dtype == np.uint64 and w.tolist() == [1, 1, 1, 0, 0, 0, 0]
    assert window_weights(0, 1).tolist() == [0]
    for bad in ((3, 3), (4, 3), (-1, 3), (1.0, 3), (1, 0), (1, 2.5), (True, 3)):
        with pytest.raises(ValueError):
            window_weights(*bad)
    for bad in ((0, 5), (-2, 5), (1.5, 5), (3, 0), (3, -1), (3, 2.0), (True, 3)):
        with pytest.raises(ValueError):
            decay_weights(*bad)


# --- FleetBatch.weighted_percentile -------------------------------------------------------------
@pytest.fixture
def standin(monkeypatch):
    """The launcher stood in; returns the call log: ("wq", segments of the chunk, table, p_num, p_den)."""
    import torch

    from krr_amd.core.engine import SimpleEngine

    calls = []

    def wquantile_part(self, ctx, part, table, p_num, p_den):
        tab = table.numpy().view(np.uint64)
        calls.append(("wq", part.n_segments, tab.copy(), p_num, p_den))
        r = np_wquantile(part.values, part.offsets, tab, p_num, p_den, part.gaps_are_nan)
        r["wsum"] = r["wsum"].view(np.int64)
        r["passes"] = np.ones(part.n_segments, np.int32)
        return {k: torch.from_numpy(v) for k, v in r.items()}

    def upload(self, tab):
        calls.append(("upload", tab.size))
        return torch.from_numpy(tab.view(np.int64))

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_wquantile_part", wquantile_part)
    monkeypatch.setattr(SimpleEngine, "_upload_table", upload)
    monkeypatch.setattr(SimpleEngine, "_stats_part", lambda self, ctx, part: _np_stats(part))
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return np.array([float(x) for samples in h[resource].values() for x in samples])


def _check(values, histories, resource, table, p):
    num, den = fraction_of(p)
    for o, h in enumerate(histories):
        b, W = wquantile_one(_flat(h, resource), table, num, den)
        got = int(values[o:o + 1].view(np.uint64)[0])
        assert (np.isnan(values[o]) and W == 0) or got == b, o


def test_values_caching_and_flags(standin, histories):
    from krr_amd.api import FleetBatch, decay_weights, window_weights

    b = FleetBatch(histories)
    table = decay_weights(8, 120)
    v = b.weighted_percentile(CPU, "95", table)
    assert v.dtype == np.float64 and v.shape == (N,) and np.isnan(v[[3, 11]]).all() and not np.isnan(np.delete(v, [3, 11])).any()
    _check(v, histories, CPU, table, "95")
    assert [c[0] for c in standin] == ["upload", "wq"] and standin[1][1] == N and standin[1][3:] == (95, 1)
    # the same percentile and the same bytes: no launch
    for again in (b.weighted_percentile(CPU, 95, table.copy()), b.weighted_percentile(CPU, Decimal("95.0"), list(table)),
                  b.weighted_percentile(CPU, "95", table.astype(np.int64))):
        assert np.array_equal(again, v, equal_nan=True)
    assert len(standin) == 2
    v2, f2 = b.weighted_percentile(CPU, "95", table, return_flags=True)
    assert f2.dtype == np.uint32 and f2[[3, 11]].tolist() == [EMPTY, EMPTY] and np.array_equal(v2, v, equal_nan=True)
    # another percentile, another table, another resource: one launch each; the fraction is exact
    b.weighted_percentile(CPU, "99.5", table)
    assert standin[-1][3:] == (199, 2)
    win = window_weights(5, 200)
    vw = b.weighted_percentile(MEM, 50, win)
    for o, h in enumerate(histories):
        x = _flat(h, MEM)[-5:]  # the unit-weight answer of the last five samples
        assert (x.size == 0 and np.isnan(vw[o])) or vw[o] == np.sort(x)[-(-x.size // 2) - 1], o
    assert len([c for c in standin if c[0] == "wq"]) == 3
    # weight_sums: from the cache when the table was used, else one launch
    n_calls = len(standin)
    ws = b.weight_sums(CPU, table)
    assert len(standin) == n_calls and ws.dtype == np.float64
    for o, h in enumerate(histories):
        assert ws[o] == sum(weights_of(_flat(h, CPU).size, table)) / 2 ** 32
    assert np.array_equal(b.weight_sums(MEM, [1]), [float(_flat(h, MEM).size) / 2 ** 32 for h in histories])
    assert len(standin) == n_calls + 2
    # no weight at all: NaN without a flag
    z, zf = b.weighted_percentile(CPU, 50, np.zeros(3, np.uint64), return_flags=True)
    assert np.isnan(z).all() and zf[0] == 0 and zf[3] == EMPTY


@pytest.mark.parametrize("bad", [np.array([], np.uint64), np.ones((2, 2), np.uint64), np.array([1.0, 2.0]),
                                 np.array([1, -1]), np.array([2 ** 32 + 1], np.uint64), np.array([True, False]),
                                 np.uint64(3), [0.5]],
                         ids=["empty", "2d", "float", "negative", "above_2^32", "bool", "scalar", "float_list"])
def test_bad_weights_raise(standin, histories, bad):
    from krr_amd.api import FleetBatch

    with pytest.raises(ValueError, match="weights"):
        FleetBatch(histories).weighted_percentile(CPU, 50, bad)
    assert standin == []


@pytest.mark.parametrize("bad", [0, -1, "100.0001", 101, "nan", "inf", "x", "0.00000000000000001", Fraction(1, 3)])
def test_bad_percentiles_raise(standin, histories, bad):
    from krr_amd.api import FleetBatch

    with pytest.raises(ValueError, match="percentile"):
        FleetBatch(histories).weighted_percentile(CPU, bad, [1])
    assert standin == []


def test_largest_weight_and_finest_percentile_pass(standin, histories):
    from krr_amd.api import FleetBatch

    v = FleetBatch(histories).weighted_percentile(CPU, "0.000000000000001", np.array([2 ** 32, 0], np.uint64))
    assert standin[-1][3:] == (1, 10 ** 15)
    for o, h in enumerate(histories):
        x = _flat(h, CPU)
        assert (x.size == 0 and np.isnan(v[o])) or v[o] == x[-1]  # only the last sample has weight


def test_chunks_share_one_upload(standin, histories):
    from krr_amd.api import FleetBatch, decay_weights
    from krr_amd.core.engine import SimpleEngine

    table = decay_weights(5, 64)
    whole = FleetBatch(histories, engine=SimpleEngine(0)).weighted_percentile(MEM, 90, table)
    del standin[:]
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    parts = FleetBatch(histories, engine=small)
    got = parts.weighted_percentile(MEM, 90, table)
    assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))
    _check(got, histories, MEM, table, 90)
    launches = [c for c in standin if c[0] == "wq"]
    assert [c[0] for c in standin].count("upload") == 1 and len(launches) > 4 and sum(c[1] for c in launches) == N
    assert all(np.array_equal(c[2], table) for c in launches)
    r = small.wquantile_series(parts.series(MEM), table, 90)
    assert set(r) == {"value", "wsum", "passes", "count", "flags"} and r["wsum"].dtype == np.uint64
    assert r["flags"].dtype == np.uint32 and r["passes"].dtype == np.int32 and r["count"].dtype == np.int64


def test_per_pod_and_to_decimal(standin, histories):
    from krr_amd.api import FleetBatch, decay_weights

    b = FleetBatch(histories)
    pods = b.per_pod(CPU)
    table = decay_weights(4, 40)
    v, f = pods.weighted_percentile(CPU, 90, table, return_flags=True)
    kept = [np.array([float(s) for s in x]) for h in histories for x in h[CPU].values() if len(x)]
    assert v.shape == (len(kept),) and standin[-1][1] == len(kept)
    for j, x in enumerate(kept):
        assert int(v[j:j + 1].view(np.uint64)[0]) == wquantile_one(x, table, 90, 1)[0], j
    dec = b.to_decimal(v, f)
    own = {s for h in histories for x in h[CPU].values() for s in x}
    assert all(d in own for d in dec)  # a sample's own bits: the Decimal the history holds
    ov, of = b.weighted_percentile(CPU, 90, table, return_flags=True)
    od = b.to_decimal(ov, of)
    assert od[3].is_nan() and od[11].is_nan() and sum(d.is_nan() for d in od) == 2


def test_no_device_raises(histories, monkeypatch):
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeUnavailable):
        FleetBatch(histories, engine=SimpleEngine(0)).weighted_percentile(CPU, 50, [1])


# --- examples/recency_strategy.py ---------------------------------------------------------------
@pytest.mark.parametrize("half_life", [1, 6, 1440])
def test_recency_strategy_equals_a_python_loop(standin, histories, half_life, monkeypatch):
    import torch

    from _standin import k_table_for
    from examples.recency_strategy import RecencySettings, RecencyStrategy
    from krr_amd.api import decay_weights
    from krr_amd.core.engine import SimpleEngine
    from oracle import oracle

    def percentiles_part(self, ctx, part, params_list):
        rows = [oracle.percentile(part.values, part.offsets, p.mode, p.p_num, p.p_den, p.q, part.gaps_are_nan,
                                  k_table=k_table_for(part, p)) for p in params_list]
        return {"value": torch.from_numpy(np.stack([r[0] for r in rows])), "count": torch.from_numpy(rows[0][1]),
                "flags": torch.from_numpy(np.stack([r[2] for r in rows]).astype(np.int32))}

    monkeypatch.setattr(SimpleEngine, "_percentiles_part", percentiles_part)
    strategy = RecencyStrategy(RecencySettings(half_life_slots=half_life, memory_buffer_percentage=Decimal(10)))
    got = strategy.run_batch(histories)
    assert len(got) == N and [c[0] for c in standin].count("wq") == 1  # every pod of the fleet in one launch
    longest = max(len(x) for h in histories for x in h[CPU].values())
    table = decay_weights(half_life, longest)
    for o, h in enumerate(histories):
        cpu, mem = got[o][CPU], got[o][MEM]
        pods = [x for x in h[CPU].values() if len(x)]
        if not pods:
            assert o in (3, 11) and cpu.request.is_nan() and cpu.limit.is_nan() and mem.request.is_nan()
            continue
        per_pod = []
        for x in pods:
            b, W = wquantile_one([float(s) for s in x], table, 95, 1)
            assert W > 0
            per_pod.append(next(s for s in x if bits(float(s)) == b))
        flat = sorted(s for x in pods for s in x)
        p99 = flat[int((len(flat) - 1) * Decimal(99) / 100)]
        assert cpu.request == max(per_pod), o
        assert cpu.limit == max(p99, cpu.request), o
        m = max(s for x in h[MEM].values() for s in x)
        assert mem.request == m * Decimal("1.1") and mem.limit == mem.request
    one = strategy.run(histories[0], None)
    assert one[CPU].request == got[0][CPU].request and one[CPU].limit == got[0][CPU].limit


def test_exports():
    import krr_amd.api as api
    from krr_amd import _native

    assert {"decay_weights", "window_weights"} <= set(api.__all__)
    assert api.decay_weights is api.batch.decay_weights and "krr_segmented_wquantile" in _native.EXPORTED_SYMBOLS
    assert hasattr(api.FleetBatch, "weighted_percentile") and hasattr(api.FleetBatch, "weight_sums")

"""krr_amd.api.batch.FleetBatch without a device: the engine's two per-chunk launchers
(``SimpleEngine._stats_part`` / ``_percentiles_part``) stood in by numpy and the CPU oracle, in
the spirit of tests/_standin.py, so that everything above a launch — packing once, caching,
chunking and the concatenation of chunk results, the mean, the Decimal conversion — runs here.
The kernels themselves: tests/test_gpu_stats.py and tests/test_gpu_fleet_batch.py."""
import decimal
import os
import re
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from krr_amd.core.models.allocations import ResourceType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU, MEM = ResourceType.CPU, ResourceType.Memory
EMPTY, NAN, CAP = 4, 1, 2
N = 20


def _histories():
    """20 objects of 0-3 pods with 1-40 samples per pod; objects 3 and 11 have no sample at all
    (no pod / one pod without data)."""
    from krr_amd.utils.prom_decimal import prom_decimal

    rng = np.random.default_rng(5)
    out = []
    for o in range(N):
        pods = {} if o == 3 else {f"o{o}-p{p}": int(rng.integers(1, 41)) for p in range(int(rng.integers(1, 4)))}
        if o == 11:
            pods = {"o11-p0": 0}
        out.append({
            CPU: {p: [prom_decimal(float(round(v, 4))) for v in rng.gamma(2.0, 0.05, n)] for p, n in pods.items()},
            MEM: {p: [prom_decimal(float(int(v))) for v in rng.normal(2e8, 2e7, n)] for p, n in pods.items()},
        })
    return out


def _np_stats(ps):
    import torch

    vals, offs = np.asarray(ps.values), np.asarray(ps.offsets)
    S = offs.size - 1
    out = {"min": np.full(S, np.nan), "max": np.full(S, np.nan), "sum": np.zeros(S),
           "count": np.zeros(S, np.int64), "flags": np.zeros(S, np.int32)}
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        out["count"][s] = x.size
        if x.size == 0:
            out["flags"][s] = EMPTY
        elif np.isnan(x).any():
            out["flags"][s], out["sum"][s] = NAN, np.nan
        else:
            out["min"][s], out["max"][s], out["sum"][s] = x.min(), x.max(), x.sum()
    return {k: torch.from_numpy(v) for k, v in out.items()}


@pytest.fixture
def standin(monkeypatch):
    """The launchers stood in; returns the call log: ("stats" | "pct", segments of the chunk)."""
    import torch

    from krr_amd.core.engine import SimpleEngine
    from oracle import oracle
    from _standin import k_table_for

    calls = []

    def stats_part(self, ctx, part):
        calls.append(("stats", part.n_segments))
        return _np_stats(part)

    def percentiles_part(self, ctx, part, params_list):
        calls.append(("pct", part.n_segments))
        rows = [oracle.percentile(part.values, part.offsets, p.mode, p.p_num, p.p_den, p.q, part.gaps_are_nan,
                                  k_table=k_table_for(part, p)) for p in params_list]
        return {"value": torch.from_numpy(np.stack([r[0] for r in rows])), "count": torch.from_numpy(rows[0][1]),
                "flags": torch.from_numpy(np.stack([r[2] for r in rows]).astype(np.int32))}

    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)
    monkeypatch.setattr(SimpleEngine, "_stats_part", stats_part)
    monkeypatch.setattr(SimpleEngine, "_percentiles_part", percentiles_part)
    return calls


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _flat(h, resource):
    return [x for samples in h[resource].values() for x in samples]


def test_packs_each_resource_once_and_caches_results(standin, histories, monkeypatch):
    from krr_amd.api import FleetBatch, batch as batch_mod

    packed = []
    real = batch_mod.pack_resource
    monkeypatch.setattr(batch_mod, "pack_resource", lambda hs, r: (packed.append(r), real(hs, r))[1])
    b = FleetBatch(histories)
    assert b.n_objects == N and packed == []
    st = b.stats(CPU)
    assert b.stats(CPU) is st and packed == [CPU]
    v = b.percentile(CPU, "95", mode="sorted_lower")
    assert packed == [CPU]  # the same packed series serves the percentile
    b.stats(MEM)
    b.percentile(MEM, 50, mode="linear")
    assert packed == [CPU, MEM]
    assert standin == [("stats", N), ("pct", N), ("stats", N), ("pct", N)]
    # asking again launches nothing; a new percentile of a set launches only the missing ones
    assert np.array_equal(b.percentile(CPU, "95", mode="sorted_lower"), v, equal_nan=True)
    vs = b.percentiles(CPU, ["50", "95", "99"], mode="sorted_lower")
    assert len(standin) == 5 and vs.shape == (3, N) and np.array_equal(vs[1], v, equal_nan=True)
    b.percentile(CPU, "95", mode="linear")  # another mode is another result
    assert len(standin) == 6


def test_values_against_python(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    for r in (CPU, MEM):
        st = b.stats(r)
        v, f = b.percentile(r, "90", mode="sorted_lower", return_flags=True)
        got_min, got_max, got_p = b.to_decimal(st.min, st.flags), b.to_decimal(st.max, st.flags), b.to_decimal(v, f)
        for o, h in enumerate(histories):
            x = _flat(h, r)
            assert st.count[o] == len(x)
            if not x:
                assert st.flags[o] == EMPTY and got_min[o].is_nan() and got_max[o].is_nan() and got_p[o].is_nan()
                continue
            assert (got_min[o], got_max[o]) == (min(x), max(x))
            assert got_p[o] == sorted(x)[int((len(x) - 1) * Decimal(90) / 100)]
            assert st.sum[o] == pytest.approx(float(sum(x)), rel=1e-12)
    assert np.array_equal(b.counts(MEM, "90", mode="sorted_lower"), b.stats(MEM).count)


def test_chunks_concatenate_in_object_order(standin, histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    whole = FleetBatch(histories, engine=SimpleEngine(0))
    small = SimpleEngine(0)
    small.chunk_bytes = 256  # 32 samples per chunk: the 20 objects run as many chunks
    parts = FleetBatch(histories, engine=small)
    for r in (CPU, MEM):
        a, c = whole.stats(r), parts.stats(r)
        for k in ("count", "min", "max", "sum", "flags"):
            assert np.array_equal(getattr(a, k), getattr(c, k), equal_nan=True), k
        va, fa = whole.percentiles(r, ["50", "99"], mode="linear", return_flags=True)
        vc, fc = parts.percentiles(r, ["50", "99"], mode="linear", return_flags=True)
        assert np.array_equal(va, vc, equal_nan=True) and np.array_equal(fa, fc)
    for kind in ("stats", "pct"):
        chunked = [n for k, n in standin if k == kind and n < N]
        assert len(chunked) > 4 and sum(chunked) == 2 * N  # whole segments, every object once per resource


def test_more_percentiles_than_one_launch_takes(standin, histories):
    """The grouping by KRR_MAX_PERCENTILES lives in the launcher that is stood in here; the engine
    entry hands it the whole list and returns one row per entry."""
    from krr_amd.api import FleetBatch

    ps = ["10", "25", "50", "75", "90", "99"]
    vs = FleetBatch(histories).percentiles(CPU, ps, mode="sorted_lower")
    assert vs.shape == (len(ps), N)
    ok = ~np.isnan(vs[0])
    assert (np.diff(vs[:, ok], axis=0) >= 0).all()


def test_mean_with_empties(standin, histories):
    from krr_amd.api import FleetBatch

    st = FleetBatch(histories).stats(CPU)
    mean = st.mean
    assert np.isnan(mean[[3, 11]]).all() and (st.count[[3, 11]] == 0).all() and (st.sum[[3, 11]] == 0).all()
    ok = st.count > 0
    assert ok.sum() == N - 2 and np.array_equal(mean[ok], st.sum[ok] / st.count[ok])


def test_to_decimal_rules():
    from krr_amd.api import FleetBatch

    values = np.array([0.1, np.nan, np.nan, 2e8, np.inf, -0.0])
    flags = np.array([0, EMPTY, NAN, 0, 0, 0], dtype=np.uint32)
    got = FleetBatch.to_decimal(values, flags)
    assert got[0] == Decimal("0.1") and str(got[0]) == "0.1"          # the float's shortest string
    assert got[1].is_nan() and got[2].is_nan()
    assert str(got[3]) == "200000000" and got[4] == Decimal("Infinity") and str(got[5]) == "-0"
    assert [str(d) for d in FleetBatch.to_decimal(values[[0, 3]])] == ["0.1", "200000000"]
    # cpu_from_raw's rule: sorted() over two or more Decimals with a NaN among them signals
    with pytest.raises(decimal.InvalidOperation):
        FleetBatch.to_decimal(values, flags, counts=np.array([5, 0, 2, 5, 5, 5]), mode="sorted_lower")
    assert FleetBatch.to_decimal(values, flags, counts=np.array([5, 0, 1, 5, 5, 5]), mode="sorted_lower")[2].is_nan()
    with pytest.raises(RuntimeError, match="KRR_FLAG_CAPACITY"):
        FleetBatch.to_decimal(values, np.array([0, 0, 0, CAP, 0, 0], dtype=np.uint32))


def test_nan_and_capacity_flags_of_percentiles(standin, monkeypatch):
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    h = [{CPU: {"p": [Decimal("1"), Decimal("NaN"), Decimal("3")]}, MEM: {}}, {CPU: {"p": [Decimal("2")]}, MEM: {}}]
    v, f = FleetBatch(h).percentile(CPU, "50", mode="sorted_lower", return_flags=True)
    assert f[0] & NAN and np.isnan(v[0]) and v[1] == 2.0 and f[1] == 0
    real = SimpleEngine._percentiles_part

    def capacity(self, ctx, part, params_list):
        out = real(self, ctx, part, params_list)
        out["flags"][0, 1] |= CAP
        return out

    monkeypatch.setattr(SimpleEngine, "_percentiles_part", capacity)
    with pytest.raises(RuntimeError, match="object 1.*KRR_FLAG_CAPACITY"):
        FleetBatch(h).percentile(CPU, "50", mode="sorted_lower")
    with pytest.raises(ValueError, match="unknown percentile mode"):
        FleetBatch(h).percentile(CPU, "50", mode="nearest")


def test_per_pod(standin, histories):
    from krr_amd.api import FleetBatch

    b = FleetBatch(histories)
    with pytest.raises(ValueError, match="pod boundaries"):
        b.per_pod(MEM)  # the packers attach them to the CPU series only
    pods = b.per_pod(CPU)
    assert b.per_pod(CPU) is pods
    kept = [[x for x in h[CPU].values() if len(x)] for h in histories]
    assert np.array_equal(np.diff(pods.pod_groups), [len(k) for k in kept]) and pods.n_objects == sum(map(len, kept))
    mx = pods.to_decimal(pods.stats(CPU).max)
    assert mx == [max(x) for k in kept for x in k]
    with pytest.raises(KeyError):
        pods.stats(MEM)


def test_from_fleet(standin, histories):
    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import pack_histories

    a, b = FleetBatch(histories), FleetBatch.from_fleet(pack_histories(histories))
    assert b.n_objects == N
    assert np.array_equal(a.stats(MEM).max, b.stats(MEM).max, equal_nan=True)
    assert np.array_equal(a.per_pod(CPU).pod_groups, b.per_pod(CPU).pod_groups)


def test_exact_mask(histories):
    from krr_amd.api import FleetBatch

    assert FleetBatch(histories).exact_mask(CPU) is None
    odd = [dict(h) for h in histories[:4]]
    odd[2] = {CPU: {"p": [Decimal("0.10"), Decimal("0.2")]}, MEM: {"p": [Decimal("5")]}}
    b = FleetBatch(odd)
    assert b.exact_mask(CPU).tolist() == [False, False, True, False] and b.exact_mask(MEM) is None


def test_no_device_raises(histories, monkeypatch):
    """No CPU path: without a HIP device every computing call raises, as every other entry."""
    import torch

    from krr_amd import _native
    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    b = FleetBatch(histories, engine=SimpleEngine(0))
    with pytest.raises(_native.NativeUnavailable):
        b.stats(CPU)
    with pytest.raises(_native.NativeUnavailable):
        b.percentile(MEM, "95", mode="linear")


def test_header_declares_and_library_exports_segmented_stats():
    import __graft_entry__ as g

    g.build()
    from krr_amd import _native

    header = open(os.path.join(ROOT, "include", "krr_amd.h")).read()
    assert re.search(r"^int\s+krr_segmented_stats\(krr_ctx\* ctx, const krr_series\* series, double\* out_min, "
                     r"double\* out_max,\s+double\* out_sum, int64_t\* out_count, uint32_t\* out_flags, "
                     r"void\* stream\);", header, flags=re.M)
    assert "krr_segmented_stats" in _native.EXPORTED_SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    assert any(line.split()[-1] == "krr_segmented_stats" and " T " in line for line in nm.splitlines())
    lib = _native.load_library()
    assert lib.krr_segmented_stats(None, None, None, None, None, None, None, None) == -1
    assert re.search(r"#define KRR_ABI_VERSION 3\b", header) and lib.krr_abi_version() == 3

"""krr_amd.api.batch.FleetBatch.overlay on the MI355X: the 20-object fleet of
tests/test_fleet_batch_host.py (0-3 pods, two objects without samples) host-packed, in chunks and
resident in HBM, and a dense-grid fleet of a few dozen objects whose pods start late or stop early,
through the real engine against the plain restatement (tests/_overlay_ref.py) — bit for bit: the
sum of a slot has one order.  Then what is built on the slots: ``as_batch`` with a percentile,
a further ``rollup``, ``peak``, ``dense``, the cache, and examples/balanced_strategy.py."""
from decimal import Decimal

import numpy as np
import pytest

from _overlay_ref import EMPTY, END, START, overlay_one
from krr_amd.core.models.allocations import ResourceAllocations, ResourceType
from test_fleet_batch_host import N, _histories

pytestmark = pytest.mark.gpu

CPU, MEM = ResourceType.CPU, ResourceType.Memory
ALIGNS = {"start": START, "end": END}
nan = np.nan


@pytest.fixture(scope="module")
def histories():
    return _histories()


def _pods(h, r):
    return [np.array([float(x) for x in samples]) for samples in h[r].values() if len(samples)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _hold(ov, objects, gaps):
    """Every object's slots against the restatement, bit for bit; returns per object the
    restatement's (active, sum, max, min) arrays."""
    assert ov.n_objects == len(objects) and ov.offsets[0] == 0
    out = []
    for s, pods in enumerate(objects):
        slots = overlay_one(pods, ALIGNS[ov.align], gaps)
        a = np.array([e[0] for e in slots], dtype=np.int64)
        sm, mx, mn = (np.array([e[k] for e in slots], dtype=np.float64) for k in (1, 2, 3))
        assert ov.slots[s] == len(slots) == max((len(p) for p in pods), default=0) and ov.pods[s] == len(pods), s
        assert ov.count[s] == a.sum() and ov.flags[s] == (EMPTY if a.sum() == 0 else 0), s
        assert ov.of(s, "active").tolist() == a.tolist(), s
        for k, want in (("sum", sm), ("max", mx), ("min", mn)):
            assert np.array_equal(_bits(ov.of(s, k)), _bits(want)), (s, k)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(a > 0, sm / np.where(a > 0, a, 1), nan)
        assert np.array_equal(ov.of(s, "mean"), mean, equal_nan=True), s
        out.append((a, sm, mx, mn))
    return out


def _resident(ps, dev):
    import torch

    from krr_amd.core.packing import PackedSeries

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    out = PackedSeries(up(ps.values, np.float64), up(ps.offsets, np.int64), int(ps.max_len), ps.gaps_are_nan)
    if ps.pod_offsets is not None:
        out.pod_offsets, out.pod_groups = up(ps.pod_offsets, np.int64), up(ps.pod_groups, np.int64)
    return out


def _dense_fleet(seed=11, S=30, slots=300):
    """A dense-grid series of S objects of 1-6 pods on 300 slots (object 4 without pods): pods
    start late, stop early or have holes, and one pod has no sample at all."""
    from krr_amd.core.packing import pack_dense_grid

    rng = np.random.default_rng(seed)
    start, step = 1_700_000_000.0, 60.0
    per_object, grids = [], []
    for o in range(S):
        k = 0 if o == 4 else int(rng.integers(1, 7))
        pods, gs = [], []
        for p in range(k):
            lo = int(rng.integers(0, 120)) if rng.random() < 0.5 else 0
            hi = int(rng.integers(180, slots)) if rng.random() < 0.5 else slots
            idx = np.arange(lo, hi)
            idx = idx[rng.random(idx.size) >= 0.1]  # scrapes missed
            if o == 7 and p == 0:
                idx = idx[:0]
            vs = rng.gamma(2.0, 0.05, idx.size)
            pods.append((start + step * idx, vs))
            g = np.full(slots, nan)
            g[idx] = vs
            gs.append(g)
        per_object.append(pods)
        grids.append(gs)
    return pack_dense_grid(per_object, start, step, slots), grids


@pytest.mark.parametrize("align", list(ALIGNS))
def test_host_packed_fleet_whole_in_chunks_and_resident(histories, align):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.engine import SimpleEngine
    from krr_amd.core.packing import PackedFleet, pack_resource

    objects = [_pods(h, CPU) for h in histories]
    ov = FleetBatch(histories, device=0).overlay(CPU, align)
    _hold(ov, objects, gaps=False)
    assert ov.flags[3] == ov.flags[11] == EMPTY and ov.tensor("sum").is_cuda and ov.tensor("mean").is_cuda
    eng = SimpleEngine(0)
    eng.chunk_bytes = 256  # 32 samples per chunk
    small = FleetBatch(histories, engine=eng)
    assert len(list(eng._series_parts(small.series(CPU)))) >= 5
    dev = torch.device("cuda:0")
    cpu = _resident(pack_resource(histories, CPU), dev)
    res = FleetBatch.from_fleet(PackedFleet(cpu, _resident(pack_resource(histories, MEM), dev)), device=0)
    for other in (small.overlay(CPU, align), res.overlay(CPU, align)):  # one order of additions: the same bits
        for k in ("sum", "max", "min", "mean"):
            assert np.array_equal(_bits(getattr(other, k)), _bits(getattr(ov, k))), k
        for k in ("active", "offsets", "slots", "pods", "count", "flags"):
            assert np.array_equal(getattr(other, k), getattr(ov, k)), k
    with pytest.raises(ValueError, match="pod boundaries"):
        res.overlay(MEM)  # pack_resource attaches the pod boundaries to the CPU series only


@pytest.mark.parametrize("align", list(ALIGNS))
def test_dense_grid_fleet_and_what_is_built_on_the_slots(align):
    import torch

    from krr_amd.api import FleetBatch
    from krr_amd.core.packing import PackedFleet, PackedSeries

    ps, grids = _dense_fleet()
    dev = torch.device("cuda:0")
    batch = FleetBatch.from_fleet(PackedFleet(_resident(ps, dev), _resident(ps, dev)), device=0)
    ov = batch.overlay(CPU, align)
    ref = _hold(ov, grids, gaps=True)
    S = len(grids)
    for s, gs in enumerate(grids):  # on the grid a slot is a point in time: active is the replica count
        up = np.sum([~np.isnan(g) for g in gs], axis=0) if gs else np.zeros(0, dtype=np.int64)
        assert ov.of(s, "active").tolist() == np.asarray(up).tolist(), s
    assert (ov.active == 0).any() and ov.active.max() >= 5 and ov.slots.tolist() == [0 if s == 4 else 300 for s in range(S)]
    both = batch.overlay(CPU, "start" if align == "end" else "end")  # every pod has the same slots: no shift
    assert np.array_equal(_bits(both.sum), _bits(ov.sum)) and np.array_equal(both.active, ov.active)
    # a percentile of the workload's total: the kernel on the restatement's series, uploaded as a gapped series
    series = [np.where(a > 0, sm, nan) for a, sm, _, _ in ref]
    offs = np.concatenate([[0], np.cumsum([x.size for x in series])]).astype(np.int64)
    ref_ps = PackedSeries(np.concatenate(series), offs, 300, True)
    want_b = FleetBatch.from_fleet(PackedFleet(ref_ps, ref_ps), device=0)
    total = ov.as_batch("sum")
    assert ov.as_batch("sum") is total and total.series(CPU).values.is_cuda and total.series(CPU).gaps_are_nan
    for p, mode in (("95", "linear"), ("50", "linear"), ("99", "sorted_lower"), ("90", "ref_index")):
        got, gf = total.percentile(CPU, p, mode=mode, return_flags=True)
        want, wf = want_b.percentile(CPU, p, mode=mode, return_flags=True)
        assert np.array_equal(gf, wf) and np.array_equal(_bits(got), _bits(want)), (p, mode)
        assert np.array_equal(total.counts(CPU, p, mode), want_b.counts(CPU, p, mode))
    assert gf[4] == EMPTY and np.isnan(got[4])
    lin = total.percentile(CPU, "95", mode="linear")
    for s, x in enumerate(series):
        if not np.isnan(x).all():
            assert lin[s] == np.percentile(x[~np.isnan(x)], 95), s
    # the replica count is a compact series in which 0 is a value
    up = ov.as_batch("active")
    assert not up.series(CPU).gaps_are_nan
    st = up.stats(CPU)
    assert st.count.tolist() == ov.slots.tolist()
    assert st.min[0] == ov.of(0, "active").min() and st.sum[0] == ov.count[0]
    # a further rollup: hourly windows of the total
    ru = total.rollup(CPU, 60, align)
    assert ru.n_windows.tolist() == [-(-int(n) // 60) for n in ov.slots]
    for s in (0, 7, S - 1):
        wins = [series[s][w:w + 60] for w in range(0, 300, 60)]
        assert ru.of(s, "wcount").tolist() == [int(np.count_nonzero(~np.isnan(w))) for w in wins], s
        want = [w[~np.isnan(w)].max() if not np.isnan(w).all() else nan for w in wins]
        assert np.array_equal(ru.of(s, "max"), want, equal_nan=True), s
    # peak: the largest slot value
    peak, most, top = ov.peak(), ov.peak("active"), ov.peak("max")
    for s, (a, sm, mx, _) in enumerate(ref):
        if a.size == 0 or a.max() == 0:
            assert np.isnan(peak[s]) and np.isnan(top[s]) and (np.isnan(most[s]) if a.size == 0 else most[s] == 0), s
        else:
            assert peak[s] == np.nanmax(series[s]) and most[s] == a.max() and top[s] == np.nanmax(mx), s
    # dense: justified by the alignment
    d = ov.dense("max")
    assert d.shape == (S, 300) and np.isnan(d[4]).all()
    assert np.array_equal(d[0], ov.of(0, "max"), equal_nan=True)


def test_dense_justifies_objects_of_different_length(histories):
    from krr_amd.api import FleetBatch

    for align in ALIGNS:
        ov = FleetBatch(histories, device=0).overlay(CPU, align)
        d = ov.dense("sum")
        assert d.shape == (N, int(ov.slots.max()))
        for s in range(N):
            n = int(ov.slots[s])
            row, pad = (d[s, d.shape[1] - n:], d[s, :d.shape[1] - n]) if align == "end" else (d[s, :n], d[s, n:])
            assert np.array_equal(row, ov.of(s, "sum")) and np.isnan(pad).all(), s


def test_second_call_does_not_launch(histories, monkeypatch):
    from krr_amd import _native
    from krr_amd.api import FleetBatch

    calls = []
    real = _native.Context.pods_overlay
    monkeypatch.setattr(_native.Context, "pods_overlay",
                        lambda self, pods, groups, n, align, *a, **k: (calls.append((n, align)),
                                                                       real(self, pods, groups, n, align, *a, **k))[1])
    batch = FleetBatch(histories, device=0)
    ov = batch.overlay(CPU)
    assert calls == [(N, END)]  # "end" is the default
    assert batch.overlay(CPU) is ov and batch.overlay(CPU, "end") is ov and calls == [(N, END)]
    batch.overlay(CPU, "start")
    assert calls == [(N, END), (N, START)]
    with pytest.raises(ValueError, match="pod boundaries"):
        batch.per_pod(CPU).overlay(CPU)
    assert calls == [(N, END), (N, START)]


def test_balanced_strategy_equals_a_numpy_computation_per_object(histories):
    """The example's requests against numpy per object, exactly: the restatement's series has the
    kernel's bits, and the percentile kernel's linear rule is numpy's."""
    import decimal

    from examples.balanced_strategy import BalancedSettings, BalancedStrategy
    from krr_amd.api.models import K8sObjectData
    from krr_amd.core.abstract.strategies import supports_batch
    from krr_amd.core.rounding import reference_context
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.utils.prom_decimal import prom_decimal

    objects = [K8sObjectData(cluster="k", name=f"app-{o}", container="main", pods=list(h[CPU]), namespace="ns",
                             kind="Deployment", allocations=ResourceAllocations(requests={}, limits={}))
               for o, h in enumerate(histories)]
    strategy = BalancedStrategy(BalancedSettings(cpu_percentile=Decimal(95), cpu_limit_percentile=Decimal(99),
                                                 memory_buffer_percentage=Decimal(10)))
    assert supports_batch(strategy)
    raw = strategy.run_batch(histories, objects)
    assert len(raw) == N == len(BatchedRunner(strategy).recommend(objects, histories))
    for o, h in enumerate(histories):
        pods = _pods(h, CPU)
        m = np.array([float(x) for samples in h[MEM].values() for x in samples])
        if not pods:
            assert o in (3, 11)
            assert raw[o][CPU].request.is_nan() and raw[o][CPU].limit.is_nan() and raw[o][MEM].request.is_nan()
            continue
        slots = overlay_one(pods, END, False)
        share = np.array([e[1] / e[0] for e in slots])
        envelope = np.array([e[2] for e in slots])
        assert raw[o][CPU].request == prom_decimal(float(np.percentile(share, 95))), o
        assert raw[o][CPU].limit == prom_decimal(float(np.percentile(envelope, 99))), o
        with decimal.localcontext(reference_context()):
            mem = prom_decimal(float(m.max())) * (1 + Decimal(10) / 100)
        assert raw[o][MEM].request == mem == raw[o][MEM].limit, o

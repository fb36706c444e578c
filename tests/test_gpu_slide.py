"""krr_segmented_slide (k_slide) on the MI355X against the plain restatement.

The series are test_gpu_rollup's: one per layout (compact; NaN-gapped with about 30% of the slots
absent and long absent stretches) that holds every length at an even and at an odd start offset,
with one-sample filler segments in between.  A row of the skeleton is 128 slots and a chunk 1,024;
the kernel takes steps of at most 64 slots, folds windows of up to 24 slots directly and works in
blocks of W slots counted from slot 0 above that: the lengths and the windows sit on both sides of
each, and cover W > L.  The truth is
tests/_slide_ref.py's: counts and extrema by numpy over every window, the sum as an exact integer
on the 2^-1074 lattice with the derived bound (c-1) u / (1 - (c-1) u) sum|x| — none of it measured
on the code under test.  One launch per (layout, W, min_count) is shared by its tests.
"""
import ctypes

import numpy as np
import pytest

import _lattice
from _rollup_ref import START, np_rollup
from _slide_ref import np_slide, scaled, sum_within_bound
from test_gpu_rollup import LENGTHS, NAN_AT, _layout

pytestmark = pytest.mark.gpu

QNAN = 0x7FF8000000000000
MAXW = 1536
WINDOWS = [1, 2, 3, 5, 7, 24, 25, 60, 64, 65, 127, 128, 129, 1000, 1024, 1025, 1440, MAXW]  # 24 | 25: the two kernels
SLOT = ("mean", "sum", "max", "min", "wcount")
SEG = ("peak", "peak_slot", "count", "flags")
GUARD = 8
SENTINEL = -777


def _min_counts(W):
    return sorted({1, -(-W // 2), W})


COMBOS = [(W, m) for W in WINDOWS for m in _min_counts(W)]


def _launch(world, W, minc, want=SLOT + ("peak", "peak_slot")):
    """One launch into guarded, sentinel-filled buffers; {name: whole buffer incl. guards}."""
    import torch

    ctx, dev, S, n = world["ctx"], world["dev"], world["S"], world["vals"].size
    dt = {"wcount": torch.int32, "peak_slot": torch.int64, "count": torch.int64, "flags": torch.int32}
    bufs = {k: torch.full(((n if k in SLOT else S) + 2 * GUARD,), SENTINEL, dtype=dt.get(k, torch.float64), device=dev)
            for k in SLOT + SEG}
    arg = {k: (bufs[k][GUARD:-GUARD] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.segmented_slide(world["series"], W, minc, arg["mean"], arg["sum"], arg["max"], arg["min"], arg["wcount"],
                        arg["peak"], arg["peak_slot"], arg["count"], arg["flags"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _inner(bufs):
    return {k: v[GUARD:-GUARD] for k, v in bufs.items()}


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()
    _WORLDS.clear()
    _RUNS.clear()
    _CACHES.clear()


_WORLDS, _RUNS, _CACHES = {}, {}, {}


def _make_world(gpu, vals, offs, gaps, **more):
    import torch

    ctx, dev = gpu
    S = offs.size - 1
    series = ctx.series(torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev), int(np.diff(offs).max()), gaps)
    ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
    torch.cuda.synchronize()
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, S=S, series=series,
                kstats={k: v.cpu().numpy() for k, v in ks.items()}, **more)


def _world(gpu, layout):
    if layout not in _WORLDS:
        gaps = layout == "gapped"
        vals, offs, index, cases = _layout(gaps)
        _WORLDS[layout] = _make_world(gpu, vals, offs, gaps, index=index, cases=cases)
    return _WORLDS[layout]


def _run(gpu, layout, W, minc):
    """The restatement and one full launch of a combination, built once."""
    key = (layout, W, minc)
    if key not in _RUNS:
        world = _world(gpu, layout)
        ref = np_slide(world["vals"], world["offs"], W, minc, world["gaps"], cache=_CACHES.setdefault((layout, W), {}))
        full = _launch(world, W, minc)
        _RUNS[key] = dict(world=world, ref=ref, full=full, got=_inner(full))
    return _RUNS[key]


@pytest.fixture(scope="module", params=["compact", "gapped"])
def layout(request):
    return request.param


@pytest.fixture(scope="module", params=COMBOS, ids=[f"W{w}-m{m}" for w, m in COMBOS])
def run(request, gpu, layout):
    W, minc = request.param
    return _run(gpu, layout, W, minc), W, minc


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _guards_hold(bufs):
    for k, v in bufs.items():
        assert (v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all(), k


def test_layout_and_windows(gpu, layout):
    from krr_amd import _native

    world = _world(gpu, layout)
    assert _native.KRR_SLIDE_MAX_WINDOW == MAXW >= 1440
    assert {n for n, _ in world["index"]} >= {f"cpu{n}" for n in LENGTHS} | {f"mem{n}" for n in LENGTHS}
    assert max(WINDOWS) > max(LENGTHS) / 2 and min(LENGTHS[1:]) < 2  # W > L occurs at every window
    for (name, parity), s in world["index"].items():
        assert world["offs"][s] % 2 == parity, name


def test_counts_and_extrema_equal_the_restatement(run):
    r, W, minc = run
    ref, got = r["ref"], r["got"]
    assert np.array_equal(got["wcount"].view(np.uint32), ref["wcount"])
    for k in ("min", "max"):
        bad = np.flatnonzero(_u64(got[k]) != _u64(np.where(np.isnan(ref[k]), np.float64(np.nan), ref[k])))
        # the restatement's NaN is numpy's default quiet NaN, 0x7FF8000000000000
        assert bad.size == 0, (k, W, minc, bad[:8], got[k][bad[:8]], ref[k][bad[:8]])
    off = ~ref["emitted"] | ref["poison"]
    for k in ("mean", "sum", "min", "max"):
        assert (_u64(got[k])[off] == QNAN).all(), k
    if minc > 1 or r["world"]["gaps"]:
        assert (~ref["emitted"]).any()
    if r["world"]["gaps"] and W <= 127:
        assert (ref["wcount"] == 0).any()  # windows absent wholly occur


def test_sum_within_the_derived_bound(run):
    """|sum - exact| <= (c-1) u / (1 - (c-1) u) sum|x| in integers; the IEEE result where infinite
    samples decide it; the quiet NaN where the window is poisoned.  The count of inexact sums is
    printed (run with -s) before anything is asserted."""
    r, W, minc = run
    ref, got = r["ref"], r["got"]
    fails, inexact = [], 0
    gs, cs = got["sum"].tolist(), ref["wcount"].tolist()
    for i in np.flatnonzero(ref["emitted"]).tolist():
        e, g = ref["exact"][i], gs[i]
        if isinstance(e, int):
            if not sum_within_bound(g, e, ref["mag"][i], cs[i]):
                fails.append((i, g, cs[i]))
            elif scaled(g) != e:
                inexact += 1
        elif e != e:
            if int(_u64(got["sum"][i:i + 1])[0]) != QNAN:
                fails.append((i, g, "nan"))
        elif g != e:
            fails.append((i, g, e))
    print(f"W={W} min_count={minc}: inexact sums {inexact} of {int(ref['emitted'].sum())}")
    assert not fails, fails[:8]


def _mean_only(r, W, minc):
    if "mean_only" not in r:
        r["mean_only"] = _launch(r["world"], W, minc, want=("mean",))
    return r["mean_only"]


def _peak_only(r, W, minc):
    if "peak_only" not in r:
        r["peak_only"] = _launch(r["world"], W, minc, want=("peak", "peak_slot"))
    return r["peak_only"]


def test_mean_is_one_division_of_the_kernels_sum(run):
    r, W, minc = run
    ref, got = r["ref"], r["got"]
    live = ref["emitted"] & ~np.isnan(got["sum"])
    with np.errstate(all="ignore"):
        want = got["sum"] / ref["wcount"].astype(np.float64)
    want = np.where(live & ~np.isnan(want), want, np.float64(np.nan))
    assert np.array_equal(_u64(got["mean"]), _u64(want))
    part = _mean_only(r, W, minc)
    assert np.array_equal(_u64(part["mean"]), _u64(r["full"]["mean"]))
    for k in ("sum", "max", "min", "wcount", "peak", "peak_slot"):
        assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


def test_peak_and_its_slot(run):
    r, W, minc = run
    world, ref, got = r["world"], r["ref"], r["got"]
    offs, mean = world["offs"], got["mean"]
    seen = dict(nan=0, none=0, inf=0, plain=0)
    for s in range(world["S"]):
        a, b = int(offs[s]), int(offs[s + 1])
        m, em = mean[a:b], ref["emitted"][a:b]
        pk, at = got["peak"][s], int(got["peak_slot"][s])
        nan_at = np.flatnonzero(em & np.isnan(m))
        if not em.any():
            assert int(_u64(got["peak"][s:s + 1])[0]) == QNAN and at == -1
            seen["none"] += 1
        elif nan_at.size:
            assert int(_u64(got["peak"][s:s + 1])[0]) == QNAN and at == nan_at[0]
            seen["nan"] += 1
        else:
            assert 0 <= at < b - a and em[at]
            want = 0 if m[at] == 0 else int(_u64(m[at:at + 1])[0])
            assert int(_u64(got["peak"][s:s + 1])[0]) == want
            assert not (m[:at][em[:at]] == pk).any()
            assert not (m[em] > pk).any()
            seen["inf" if np.isinf(pk) else "plain"] += 1
    assert seen["none"] and (seen["plain"] or minc > 1)  # segments of no slot; full windows of a gapped series are rare
    if not world["gaps"] and minc == 1:
        assert seen["nan"] >= 2 * len(NAN_AT)  # every nan_sample case, and +Inf next to -Inf once W >= 2
        assert seen["inf"] == (2 if W == 1 else 0)
    part = _peak_only(r, W, minc)
    for k in ("peak", "peak_slot", "count", "flags"):
        assert np.array_equal(part[k].view(np.uint8), r["full"][k].view(np.uint8)), k
    for k in SLOT:
        assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


def test_count_and_flags_equal_segmented_stats(run):
    r, W, minc = run
    got, ks, ref = r["got"], r["world"]["kstats"], r["ref"]
    assert np.array_equal(got["count"], ks["count"]) and np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32))
    assert np.array_equal(got["flags"].view(np.uint32), ref["flags"])
    _guards_hold(r["full"])


def test_two_launches_give_equal_bits(run):
    r, W, minc = run
    again = _launch(r["world"], W, minc)
    for k, v in r["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("want", [("sum", "wcount"), ("min", "peak"), ("max", "mean", "peak_slot"), ()],
                         ids=["sum_wcount", "min_peak", "max_mean_slot", "count_flags_only"])
@pytest.mark.parametrize("W,minc", [(1, 1), (5, 3), (24, 12), (25, 13), (64, 32), (129, 1), (1440, 720)])
def test_null_outputs(gpu, layout, W, minc, want):
    """A NULL output is not written, the others hold the full launch's bits, and nothing lands
    outside the given buffers."""
    r = _run(gpu, layout, W, minc)
    part, full = _launch(r["world"], W, minc, want=want), r["full"]
    for k in SLOT + SEG:
        if k in want or k in ("count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k
        else:
            assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


@pytest.mark.parametrize("W", [1, 5, 128, 1000])
def test_compact_nan_sample_poisons_its_windows_only(gpu, W):
    r = _run(gpu, "compact", W, 1)
    world, got = r["world"], r["got"]
    for n, at in NAN_AT:
        for p in (0, 1):
            s = world["index"][(f"nan_sample{n}_{at}", p)]
            assert got["flags"][s] == 1 and got["count"][s] == n
            o = int(world["offs"][s])
            hit = np.zeros(n, bool)
            hit[at:at + W] = True
            for k in ("mean", "sum", "min", "max"):
                assert np.array_equal(_u64(got[k][o:o + n]) == QNAN, hit), (n, at, p, k)
            assert np.array_equal(got["wcount"][o:o + n], np.minimum(np.arange(n) + 1, W))


@pytest.mark.parametrize("W", [1, 3, 64, 129])
def test_zeros_and_infinities(gpu, layout, W):
    """An extremum of zero is +0.0 whatever zeros the window holds; +-Inf are plain IEEE."""
    r = _run(gpu, layout, W, 1)
    world, got = r["world"], r["got"]
    for p in (0, 1):
        for name in ("pos_zero", "neg_zero"):
            s = world["index"][(name, p)]
            a, b = world["offs"][s:s + 2]
            live = got["wcount"][a:b] > 0
            assert live.any()
            for k in ("min", "max"):
                assert (_u64(got[k][a:b])[live] == 0).all(), (name, k)
            assert (got["sum"][a:b][live] == 0).all() and (got["mean"][a:b][live] == 0).all()
        s = world["index"][("inf", p)]
        a = int(world["offs"][s])
        x = world["cases"]["inf"]
        for i in range(x.size):
            xs = x[max(0, i - W + 1):i + 1]
            xs = xs[~np.isnan(xs)]
            if xs.size == 0:
                continue
            with np.errstate(invalid="ignore"):
                want = xs.sum()
            assert got["max"][a + i] == xs.max() and got["min"][a + i] == xs.min()
            if not np.isfinite(want):
                assert np.array_equal(got["sum"][a + i], want, equal_nan=True), i
                assert np.array_equal(got["mean"][a + i], want, equal_nan=True), i
        assert got["flags"][s] == 0


@pytest.mark.parametrize("W", [1, 5, 24, 25, 64, 129, 1025])
def test_slide_at_a_window_end_equals_the_rollup(gpu, layout, W):
    """The slide at slot (w+1) W - 1 covers the start-aligned rollup window w: wcount, min and max
    are bit-equal to krr_segmented_rollup's, and both sums lie inside the same bound."""
    import torch

    r = _run(gpu, layout, W, 1)
    world, ref, got = r["world"], r["ref"], r["got"]
    ctx, dev, S, offs = world["ctx"], world["dev"], world["S"], world["offs"]
    roll = np_rollup(world["vals"], offs, W, START, world["gaps"])
    n = int(roll["offsets"][-1])
    out = {k: torch.empty(n, dtype=torch.int32 if k == "wcount" else torch.float64, device=dev)
           for k in ("min", "max", "sum", "wcount")}
    cnt, flg = torch.empty(S, dtype=torch.int64, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    ctx.segmented_rollup(world["series"], W, START, torch.from_numpy(roll["offsets"]).to(dev), out["min"], out["max"],
                         out["sum"], out["wcount"], cnt, flg)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    pairs = [(int(roll["offsets"][s]) + w, int(offs[s]) + (w + 1) * W - 1)
             for s in range(S) for w in range(int(offs[s + 1] - offs[s]) // W)]
    assert len(pairs) >= 20
    wi, si = np.array(pairs).T
    assert np.array_equal(out["wcount"][wi], got["wcount"][si])
    live = got["wcount"][si] > 0
    for k in ("min", "max"):
        assert np.array_equal(_u64(out[k][wi][live]), _u64(got[k][si][live])), k
    for w, i in zip(wi[live].tolist(), si[live].tolist()):
        e = ref["exact"][i]
        if isinstance(e, int):
            c = int(ref["wcount"][i])
            assert sum_within_bound(float(out["sum"][w]), e, ref["mag"][i], c), (w, i)
            assert sum_within_bound(float(got["sum"][i]), e, ref["mag"][i], c), (w, i)


@pytest.mark.parametrize("W", [5, 129, 1025])
@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_lattice(gpu, gaps, W):
    """The edge-geometry lattice with every filler two slots longer (shift=1): fillers of +-1e300
    never reach a neighbour's first windows, which would change its extrema and its sum's size."""
    vals, offs, index = _lattice.build(gaps, seed=91 if gaps else 92, shift=1)
    world = _make_world(gpu, vals, offs, gaps)
    ref = np_slide(vals, offs, W, 1, gaps, exact=False)
    full = _launch(world, W, 1)
    got = _inner(full)
    _guards_hold(full)
    assert np.array_equal(got["wcount"].view(np.uint32), ref["wcount"])
    for k in ("min", "max"):
        assert np.array_equal(_u64(got[k]), _u64(np.where(np.isnan(ref[k]), np.float64(np.nan), ref[k]))), k
    names = _lattice.names(offs, index)
    for s, (content, n, _) in enumerate(names):
        a, b = int(offs[s]), int(offs[s + 1])
        if content != "filler":
            live = ref["emitted"][a:b] & ~ref["poison"][a:b]
            assert (np.abs(got["sum"][a:b][live]) < 1e290).all(), names[s]
            with np.errstate(all="ignore"):
                assert np.array_equal(_u64(got["mean"][a:b][live]),
                                      _u64((got["sum"][a:b] / ref["wcount"][a:b])[live])), names[s]
    assert np.array_equal(got["count"], world["kstats"]["count"])
    assert np.array_equal(got["flags"].view(np.uint32), world["kstats"]["flags"].view(np.uint32))


def test_argument_errors(gpu):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    world = _world(gpu, "compact")
    lib = _native.load_library()
    assert lib.krr_abi_version() == 3
    call = lib.krr_segmented_slide
    none = (None,) * 10
    assert call(None, None, 5, 1, *none) == _native.KRR_E_INVALID
    assert call(ctx._h, None, 5, 1, *none) == _native.KRR_E_INVALID
    series, S = world["series"], world["S"]
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    sp = ctypes.byref(series)
    outs = (None,) * 7
    for W in (0, -1, MAXW + 1, 2 ** 40):
        assert call(ctx._h, sp, W, 1, *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    for W, m in ((5, 0), (5, -1), (5, 6), (1, 2), (MAXW, MAXW + 1)):
        assert call(ctx._h, sp, W, m, *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, 5, 1, *outs, None, flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, 5, 1, *outs, cnt.data_ptr(), None, None) == _native.KRR_E_INVALID
    torch.cuda.synchronize()
    assert (cnt == SENTINEL).all() and (flg == SENTINEL).all()  # a refused call launches nothing
    with pytest.raises(_native.NativeError):
        ctx.segmented_slide(series, 0, 1, None, None, None, None, None, None, None, cnt, flg)
    # every data output NULL is a valid launch: count and flags only
    assert call(ctx._h, sp, MAXW, MAXW, *outs, cnt.data_ptr(), flg.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), world["kstats"]["count"])


def test_no_segments_launches_nothing(gpu):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert lib.krr_segmented_slide(ctx._h, ctypes.byref(empty), 5, 1, *(None,) * 10) == 0
    assert lib.krr_segmented_slide(ctx._h, ctypes.byref(empty), 0, 1, *(None,) * 10) == _native.KRR_E_INVALID

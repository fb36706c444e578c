"""krr_segmented_rollup (k_rollup) on the MI355X against the plain restatement.

One series per layout (compact; NaN-gapped with about 30% of the slots absent and stretches in
which whole windows are absent) holds every length at an even and at an odd start offset: the
streaming skeleton reads an unaligned first or last sample with the last chunk, the two slots the
kernel has to put into the first and the last window itself.  A row is 128 slots and a chunk 1,024:
the lengths and the windows sit on both sides of each, and cover W > L, L % W == 0 and the
body-less L <= 2.  The truth is tests/_rollup_ref.py's: counts and extrema by plain loops, the sum
as an exact rational with the derived bound (m-1) u / (1 - (m-1) u) sum|x| — none of it measured on
the code under test.  One launch per (layout, W, align) is shared by the tests of that combination.
"""
from fractions import Fraction

import numpy as np
import pytest

from _rollup_ref import CAPACITY, EMPTY, END, NAN, START, np_rollup, window_bounds

pytestmark = pytest.mark.gpu

QNAN = 0x7FF8000000000000
LENGTHS = [0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2049, 3000]
WINDOWS = [1, 2, 3, 5, 7, 60, 64, 127, 128, 129, 1000, 1024, 1025, 5000]
ALIGNS = {"start": START, "end": END}
STATS = ("min", "max", "sum", "wcount")
GUARD = 8
SENTINEL = -777
INF = float("inf")
NAN_AT = ((1, 0), (2, 1), (3, 0), (129, 128), (1025, 0), (1025, 1024), (2049, 1000), (3000, 2999))


def _layout(gaps):
    """name -> samples, then every case at an even and at an odd start offset (one-sample filler
    segments shift the parity)."""
    rng = np.random.default_rng(17 if gaps else 18)
    cases = {}
    for n in LENGTHS:
        x = rng.gamma(2.0, 0.05, n)
        x[rng.random(n) < 0.02] = 0.0
        x[rng.random(n) < 0.02] = -0.0
        cases[f"cpu{n}"] = x
        cases[f"mem{n}"] = np.floor(rng.normal(2e8, 2e7, n))
    cases["signed"] = rng.normal(0.0, 1.0, 700)
    cases["pos_zero"] = np.zeros(300)
    cases["neg_zero"] = -np.zeros(300)
    z = rng.normal(0.0, 1.0, 400)
    z[::3] = -0.0  # windows whose minimum or maximum is a zero of either sign
    z[1::7] = 0.0
    cases["mixed_zero"] = z
    x = rng.gamma(2.0, 0.05, 1300)
    x[[0, 5, 6, 130, 1299]] = INF
    x[[7, 640, 1298]] = -INF
    cases["inf"] = x
    if gaps:
        for name, x in list(cases.items()):
            x = x.copy()
            holes = rng.random(x.size) < 0.3
            if x.size == 1:
                holes[:] = False
            x[holes] = np.nan
            if x.size >= 1023:
                x[40:300] = np.nan  # windows absent wholly, W up to 127
            if x.size >= 3000:
                x[900:2100] = np.nan  # ... and W = 1000, 1024
            cases[name] = x
        for n in (1, 2, 129, 1025):
            cases[f"all_gap{n}"] = np.full(n, np.nan)
        x = np.full(1400, np.nan)
        x[[0, 3, 130, 600, 1025, 1399]] = [1.5, -2.0, 0.0, 7.0, -0.0, 3.0]
        cases["sparse"] = x
    else:
        for n, at in NAN_AT:
            x = np.floor(rng.normal(2e8, 2e7, n))
            x[at] = np.nan
            cases[f"nan_sample{n}_{at}"] = x
    segs, index, pos = [], {}, 0
    for name, x in cases.items():
        for parity in (0, 1):
            if pos % 2 != parity:
                segs.append(np.array([7.0]))
                pos += 1
            index[(name, parity)] = len(segs)
            segs.append(x)
            pos += x.size
    offs = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    return np.concatenate(segs), offs, index, cases


def _launch(world, W, align, woffs, want=STATS):
    """One launch into guarded, sentinel-filled buffers; {name: whole buffer incl. guards}."""
    import torch

    ctx, dev, S = world["ctx"], world["dev"], world["S"]
    n = int(woffs.max())
    bufs = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32 if k == "wcount" else torch.float64,
                          device=dev) for k in STATS}
    bufs["count"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    bufs["flags"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    arg = {k: (bufs[k][GUARD:-GUARD] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.segmented_rollup(world["series"], W, align, torch.from_numpy(woffs).to(dev), arg["min"], arg["max"],
                         arg["sum"], arg["wcount"], arg["count"], arg["flags"])
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


_WORLDS, _RUNS = {}, {}


def _world(gpu, layout):
    if layout not in _WORLDS:
        import torch

        ctx, dev = gpu
        gaps = layout == "gapped"
        vals, offs, index, cases = _layout(gaps)
        S = offs.size - 1
        series = ctx.series(torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev), int(np.diff(offs).max()), gaps)
        ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
        ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
        torch.cuda.synchronize()
        _WORLDS[layout] = dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, index=index, cases=cases, S=S,
                               series=series, kstats={k: v.cpu().numpy() for k, v in ks.items()})
    return _WORLDS[layout]


def _run(gpu, layout, W, align):
    """The restatement and one full launch of a combination, built once."""
    key = (layout, W, align)
    if key not in _RUNS:
        world = _world(gpu, layout)
        ref = np_rollup(world["vals"], world["offs"], W, ALIGNS[align], world["gaps"])
        full = _launch(world, W, ALIGNS[align], ref["offsets"])
        _RUNS[key] = dict(world=world, ref=ref, full=full, got=_inner(full))
    return _RUNS[key]


@pytest.fixture(scope="module", params=["compact", "gapped"])
def layout(request):
    return request.param


@pytest.fixture(scope="module", params=list(ALIGNS))
def align(request):
    return request.param


@pytest.fixture(scope="module", params=WINDOWS, ids=[f"W{w}" for w in WINDOWS])
def run(request, gpu, layout, align):
    return _run(gpu, layout, request.param, align), request.param, align


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _guards_hold(bufs):
    for k, v in bufs.items():
        assert (v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all(), k


def test_layout_covers_both_parities(gpu, layout):
    world = _world(gpu, layout)
    offs, index = world["offs"], world["index"]
    for (name, parity), s in index.items():
        assert offs[s] % 2 == parity, name
        assert offs[s + 1] - offs[s] == world["cases"][name].size <= 3000
    assert {n for n, _ in index} >= {f"cpu{n}" for n in LENGTHS} | {f"mem{n}" for n in LENGTHS}
    if world["gaps"]:
        x = world["cases"]["cpu3000"]
        assert abs(np.isnan(x[2100:]).mean() - 0.3) < 0.05 and np.isnan(x[900:2100]).all()


def test_counts_and_extrema_equal_the_restatement(run):
    r, W, align = run
    ref, got = r["ref"], r["got"]
    assert ref["written"].all() and got["wcount"].size == ref["wcount"].size == int(ref["offsets"][-1])
    assert np.array_equal(got["wcount"].view(np.uint32), ref["wcount"])
    for k in ("min", "max"):
        bad = np.flatnonzero(_u64(got[k]) != _u64(np.where(np.isnan(ref[k]), np.float64(np.nan), ref[k])))
        # the restatement's NaN is numpy's default quiet NaN, 0x7FF8000000000000
        assert bad.size == 0, (k, W, align, bad[:8], got[k][bad[:8]], ref[k][bad[:8]])
    empty = ref["wcount"] == 0
    assert (_u64(got["min"])[empty] == QNAN).all() and (_u64(got["max"])[empty] == QNAN).all()
    if r["world"]["gaps"] and W <= 127:
        assert empty.any()  # windows absent wholly occur


def test_sum_within_the_derived_bound(run):
    """|wsum - exact| <= (m-1) u / (1 - (m-1) u) sum|x| in rationals; +0.0 bits for an empty
    window; the IEEE result where infinite samples decide it.  The worst error / bound is printed
    (run with -s) before anything is asserted."""
    r, W, align = run
    ref, got = r["ref"], r["got"]
    fails, worst, inexact = [], Fraction(0), 0
    for i, (e, b) in enumerate(zip(ref["exact"], ref["bound"])):
        g = float(got["sum"][i])
        if not isinstance(e, Fraction):  # nan window (compact NaN sample), or infinite samples
            same = (g != g and e != e) or g == e
            if e != e and ref["wcount"][i] and not r["world"]["gaps"] and np.isnan(ref["min"][i]):
                same = same and int(_u64(got["sum"][i:i + 1])[0]) == QNAN
            if not same:
                fails.append((i, g, e))
        elif ref["wcount"][i] == 0:
            if int(_u64(got["sum"][i:i + 1])[0]) != 0:
                fails.append((i, "not +0.0", g))
        else:
            err = abs(Fraction(g) - e) if np.isfinite(g) else None
            if err is None or err > b:
                fails.append((i, g, float(e), float(b)))
            elif err > 0:
                inexact += 1
                worst = max(worst, err / b)
    print(f"W={W} {align}: worst sum error / bound {float(worst):.3g}, inexact sums {inexact}")
    assert not fails, fails[:8]


def test_count_and_flags_equal_segmented_stats(run):
    r, W, align = run
    got, ks, ref = r["got"], r["world"]["kstats"], r["ref"]
    assert np.array_equal(got["count"], ks["count"]) and np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32))
    assert np.array_equal(got["flags"].view(np.uint32), ref["flags"])
    _guards_hold(r["full"])


def test_two_launches_give_equal_bits(run):
    r, W, align = run
    again = _launch(r["world"], W, ALIGNS[align], r["ref"]["offsets"])
    for k, v in r["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("want", [("sum", "wcount"), ("min",), ("max", "min", "sum"), ("wcount",), ()],
                         ids=["sum_wcount", "min_only", "no_wcount", "wcount_only", "count_flags_only"])
def test_null_outputs(run, want):
    """A NULL per-window output is not written, the others hold the full launch's bits, and nothing
    lands outside the given buffers."""
    r, W, align = run
    part, full = _launch(r["world"], W, ALIGNS[align], r["ref"]["offsets"], want=want), r["full"]
    for k in STATS + ("count", "flags"):
        if k in want or k in ("count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k
        else:
            assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


@pytest.mark.parametrize("W", [1, 5, 128, 1000])
def test_compact_nan_sample_gives_nan_windows(gpu, align, W):
    """NaN propagates per window: exactly the windows that hold the NaN sample are NaN in min, max
    and sum, with their slot count, and the segment is flagged."""
    r = _run(gpu, "compact", W, align)
    world, ref, got = r["world"], r["ref"], r["got"]
    seen = 0
    for n, at in NAN_AT:
        for p in (0, 1):
            s = world["index"][(f"nan_sample{n}_{at}", p)]
            assert got["flags"][s] == NAN and got["count"][s] == n
            o = int(ref["offsets"][s])
            for w, (lo, hi) in enumerate(window_bounds(n, W, ALIGNS[align])):
                hit = lo <= at < hi
                for k in ("min", "max", "sum"):
                    assert (int(_u64(got[k][o + w:o + w + 1])[0]) == QNAN) == hit, (n, at, p, w, k)
                assert got["wcount"][o + w] == hi - lo
                seen += hit
    assert seen == 2 * len(NAN_AT)


@pytest.mark.parametrize("W", [1, 3, 64, 129])
def test_zeros_and_infinities(gpu, layout, align, W):
    """An extremum of zero is +0.0 whatever zeros the window holds; +-Inf are plain IEEE."""
    r = _run(gpu, layout, W, align)
    world, ref, got = r["world"], r["ref"], r["got"]
    for p in (0, 1):
        for name in ("pos_zero", "neg_zero"):
            s = world["index"][(name, p)]
            a, b = ref["offsets"][s:s + 2]
            live = got["wcount"][a:b] > 0
            assert live.any()
            for k in ("min", "max"):
                assert (_u64(got[k][a:b])[live] == 0).all(), (name, k)
            assert (got["sum"][a:b] == 0).all()
        s = world["index"][("inf", p)]
        a, b = ref["offsets"][s:s + 2]
        x = world["cases"]["inf"]
        for w, (lo, hi) in enumerate(window_bounds(x.size, W, ALIGNS[align])):
            xs = x[lo:hi][~np.isnan(x[lo:hi])]
            if xs.size == 0:
                continue
            with np.errstate(invalid="ignore"):
                want = xs.sum()
            assert got["max"][a + w] == xs.max() and got["min"][a + w] == xs.min()
            if not np.isfinite(want):
                assert np.array_equal(got["sum"][a + w], want, equal_nan=True), (w, lo, hi)
        assert got["flags"][s] == 0


@pytest.mark.parametrize("W", [1, 5, 128, 1025])
def test_small_span_sets_capacity_and_writes_nothing(gpu, layout, align, W):
    """win_offsets with slack everywhere (any layout with at least nw entries is allowed) and one
    entry too few for some segments: those get KRR_FLAG_CAPACITY and keep the sentinels, the
    others are written at their own offsets as the restatement says."""
    world = _world(gpu, layout)
    offs, S = world["offs"], world["S"]
    nw = -(-np.diff(offs) // W)
    victims = [s for s in range(S) if nw[s] > 0 and s % 5 == 2]
    span = nw + 1
    span[victims] = nw[victims] - 1
    woffs = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    ref = np_rollup(world["vals"], offs, W, ALIGNS[align], world["gaps"], win_offsets=woffs)
    got = _launch(world, W, ALIGNS[align], woffs)
    _guards_hold(got)
    got = _inner(got)
    assert victims and all(ref["flags"][s] & CAPACITY for s in victims)
    assert np.array_equal(got["flags"].view(np.uint32), ref["flags"])
    assert np.array_equal(got["count"], ref["count"])
    wr = ref["written"]
    assert wr.any() and (~wr).any()
    for k in STATS:
        assert (got[k][~wr] == SENTINEL).all(), k
    assert np.array_equal(got["wcount"][wr].view(np.uint32), ref["wcount"][wr])
    for k in ("min", "max"):
        assert np.array_equal(_u64(got[k][wr]), _u64(ref[k][wr])), k
    for i in np.flatnonzero(wr):
        e = ref["exact"][i]
        if isinstance(e, Fraction) and ref["wcount"][i]:
            assert abs(Fraction(float(got["sum"][i])) - e) <= ref["bound"][i], i


def test_argument_errors(gpu):
    import ctypes

    import torch

    from krr_amd import _native

    ctx, dev = gpu
    world = _world(gpu, "compact")
    lib = _native.load_library()
    assert (_native.KRR_ROLLUP_START, _native.KRR_ROLLUP_END) == (START, END)
    assert lib.krr_abi_version() == 3

    def call(h, sp, W, align, *rest):
        return lib.krr_segmented_rollup(h, sp, W, align, *rest)

    none = (None,) * 8
    assert call(None, None, 5, 0, *none) == _native.KRR_E_INVALID
    assert call(ctx._h, None, 5, 0, *none) == _native.KRR_E_INVALID
    series, S = world["series"], world["S"]
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    wo = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    sp = ctypes.byref(series)
    outs = (None,) * 4
    for W in (0, -1, 2 ** 31, 2 ** 40):
        assert call(ctx._h, sp, W, 0, wo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    for a in (-1, 2, 7):
        assert call(ctx._h, sp, 5, a, wo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, 5, 0, None, *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, 5, 0, wo.data_ptr(), *outs, None, flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, 5, 0, wo.data_ptr(), *outs, cnt.data_ptr(), None, None) == _native.KRR_E_INVALID
    torch.cuda.synchronize()
    assert (cnt == SENTINEL).all() and (flg == SENTINEL).all()  # a refused call launches nothing
    with pytest.raises(_native.NativeError):
        ctx.segmented_rollup(series, 0, 0, wo, None, None, None, None, cnt, flg)
    # the largest window is accepted: every segment is one window
    assert call(ctx._h, sp, 2 ** 31 - 1, 1, wo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), world["kstats"]["count"])


def test_no_segments_launches_nothing(gpu):
    import ctypes

    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert lib.krr_segmented_rollup(ctx._h, ctypes.byref(empty), 5, 1, *(None,) * 8) == 0

"""krr_segmented_exceed (k_exceed) on the MI355X against the plain restatement.

The plan is tests/test_gpu_moments.py's: one series per layout (compact, NaN-gapped with about a
fifth of the slots absent) holds every case, each at an even and at an odd start offset (the
streaming skeleton reads an unaligned first or last sample with the last chunk — the two slots
whose ORDER the kernel has to restore), one launch of four threshold rows per layout in a module
fixture, guarded output buffers.  The truth is tests/_exceed_ref.py's: integers by a plain loop,
the excess as an exact rational sum with the derived bound m u / (1 - m u) E — none of it measured
on the code under test.  A row is 128 slots and a chunk 1,024: the lengths and the placed runs sit
on both sides of each.
"""
from fractions import Fraction

import numpy as np
import pytest

from _exceed_ref import INT_FIELDS, compacted, exceed_one

pytestmark = pytest.mark.gpu

EMPTY, NAN = 4, 1
QNAN = 0x7FF8000000000000
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17]
NAN_AT = ((1, 0), (2, 1), (65, 64), (1500, 3), (2049, 2048))
R = 4
FIELDS = INT_FIELDS + ("excess",)
GUARD = 8
SENTINEL = -777
INF = float("inf")
LO, HI, TAU = 1.0, 3.0, 2.0  # the placed patterns: samples LO (below) and HI (above) around TAU


def _runs(n, runs, lo=LO, hi=HI):
    x = np.full(n, lo)
    for a, b in runs:
        x[a:b] = hi
    return x


def _cases():
    """name -> (float64 samples (<= 5,000), four thresholds)."""
    rng = np.random.default_rng(31)
    cases = {}
    special = [TAU, np.nan, INF, -INF]
    for n in LENGTHS:
        # tau rows: none above | equal to every sample (strict: none above) | all above | all above, excess +Inf
        cases[f"flat{n}"] = (np.full(n, LO), [TAU, LO, LO / 2, -INF])
        cases[f"alt_up{n}"] = (np.where(np.arange(n) % 2 == 0, HI, LO), special)    # slot 0 above
        cases[f"alt_down{n}"] = (np.where(np.arange(n) % 2 == 1, HI, LO), special)  # slot 0 below
        x = rng.gamma(2.0, 0.05, n)
        p = np.sort(x)
        pick = (lambda q: p[int((n - 1) * q)]) if n else (lambda q: 0.1)  # an own sample: equality occurs
        cases[f"gamma{n}"] = (x, [pick(0.5), pick(0.9), pick(0.99), np.nan])
    for i, n in enumerate(rng.integers(1, 5001, 40).tolist()):
        x = rng.gamma(2.0, 0.05, n) if i % 2 else np.floor(rng.normal(2e8, 2e7, n))
        p = np.sort(x)
        cases[f"{'cpu' if i % 2 else 'mem'}{i}"] = (x, [p[(n - 1) // 2], p[int((n - 1) * 0.9)], p[int((n - 1) * 0.99)],
                                                     p[0] - 1.0])
    four = [TAU] * 4
    # runs across a row boundary (slot 128 of the body: either parity shifts it by one) and a chunk's
    for a, b in ((100, 140), (127, 129), (128, 130), (126, 128), (1000, 1060), (1023, 1026), (1024, 1025),
                 (90, 1300), (255, 257), (2040, 2060)):
        cases[f"run{a}_{b}"] = (_runs(2500, [(a, b)]), four)
    cases["two_equal_runs"] = (_runs(2100, [(50, 67), (1500, 1517)]), four)
    cases["equal_runs_one_row"] = (_runs(300, [(140, 145), (150, 155)]), four)
    cases["longer_first"] = (_runs(2100, [(10, 300), (1500, 1517)]), four)
    cases["longer_last"] = (_runs(2100, [(10, 30), (1500, 1917)]), four)
    # the head and tail slots: runs that include slot 0 / slot L - 1, L even and odd
    for n in (2, 3, 64, 65, 130, 131, 1026, 1027, 2052, 2053):
        for k in (1, 2, min(n, 200)):
            cases[f"starts{n}_{k}"] = (_runs(n, [(0, k)]), four)
            cases[f"ends{n}_{k}"] = (_runs(n, [(n - k, n)]), four)
            cases[f"both{n}_{k}"] = (_runs(n, [(0, k), (n - k, n)]), four)
        cases[f"inner{n}"] = (_runs(n, [(1, n - 1)]), four)  # everything but the two ends
    # signed zeros: +0.0 > -0.0 is false, and so is the reverse
    z = np.zeros(200)
    cases["pos_zero"] = (z, [-0.0, 0.0, -1.0, np.nan])
    cases["neg_zero"] = (-z, [0.0, -0.0, -1.0, INF])
    cases["inf_samples"] = (np.array([1.0, INF, INF, 0.5, INF]), [2.0, INF, -INF, np.nan])
    cases["neg_inf_sample"] = (np.array([1.0, -INF, 2.0, -INF]), [-INF, 0.0, 1.0, np.nan])  # -Inf > -Inf is false
    return cases


def _layout(cases, gaps, seed):
    """Every case at an even and at an odd start offset (one-sample filler segments shift the
    parity).  gaps: about a fifth of the slots of every case become NaN (absent; one-slot cases
    stay), plus runs interrupted by absent slots only (they must not break) and by one below
    sample among gaps (they must), lone samples among gaps and all-gap segments; compact: NaN
    samples in segments of their own."""
    rng = np.random.default_rng(seed)
    cases = dict(cases)
    four = [TAU] * 4
    if gaps:
        for name, (x, taus) in list(cases.items()):
            x = x.copy()
            holes = rng.random(x.size) < 0.2
            if x.size == 1:
                holes[:] = False
            x[holes] = np.nan
            cases[name] = (x, taus)
        for a, b in ((100, 160), (1000, 1100), (0, 40), (1460, 1500)):
            x = _runs(1500, [(a, b)])
            x[a + 3:b - 3:2] = np.nan          # every other slot inside the run absent
            x[a + 10:a + 20] = np.nan          # and a hole of ten
            cases[f"gap_run{a}_{b}"] = (x, four)
            y = x.copy()
            y[a + 15] = LO                     # one below sample in the hole: two runs
            cases[f"gap_broken{a}_{b}"] = (y, four)
        x = np.full(1400, np.nan)              # a run of 5 samples spread over 11 rows
        x[[3, 130, 600, 1025, 1399]] = HI
        cases["sparse_run"] = (x, four)
        y = x.copy()
        y[601] = LO
        cases["sparse_run_broken"] = (y, four)
        for n, at in ((4, 2), (1500, 1499), (1500, 0), (2050, 1031)):
            x = np.full(n, np.nan)
            x[at] = 5.5
            cases[f"lone{n}_{at}"] = (x, [5.0, 5.5, 6.0, -INF])
        for n in (1, 64, 1025):
            cases[f"all_gap{n}"] = (np.full(n, np.nan), four)
    else:
        for n, at in NAN_AT:
            x = np.floor(rng.normal(2e8, 2e7, n))
            x[at] = np.nan
            cases[f"nan_sample{n}"] = (x, [1e8, 2e8, -INF, np.nan])
    segs, thr, index, pos = [], [], {}, 0
    for name, (x, taus) in cases.items():
        for parity in (0, 1):
            if pos % 2 != parity:
                segs.append(np.array([7.0]))
                thr.append([1.0, 7.0, 8.0, np.nan])
                pos += 1
            index[(name, parity)] = len(segs)
            segs.append(x)
            thr.append(taus)
            pos += x.size
    offs = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    return np.concatenate(segs), offs, np.ascontiguousarray(np.array(thr, dtype=np.float64).T), index, cases


def _launch(ctx, series, thr, S, dev, want=FIELDS):
    """One launch of thr.shape[0] rows into guarded buffers; {name: whole buffer incl. guards}."""
    import torch

    rows = thr.shape[0]
    d_thr = torch.from_numpy(np.ascontiguousarray(thr)).to(dev)
    bufs = {k: torch.full((rows * S + 2 * GUARD,), SENTINEL, dtype=torch.float64 if k == "excess" else torch.int64,
                          device=dev) for k in FIELDS}
    bufs["count"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    bufs["flags"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    arg = {k: (bufs[k][GUARD:-GUARD] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.segmented_exceed(series, d_thr, rows, arg["above"], arg["excess"], arg["longest"], arg["head"], arg["tail"],
                         arg["last"], arg["count"], arg["flags"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _inner(bufs, S):
    return {k: (v[GUARD:-GUARD] if k in ("count", "flags") else v[GUARD:-GUARD].reshape(-1, S)) for k, v in bufs.items()}


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


_WORLDS = {}


def _world(gpu, layout):
    """The layout's series in HBM, the kernel's outputs (one launch of four rows), k_stats' count /
    flags on the same tensors and the restatement per case and row (shared by the two parities).
    Built once per layout."""
    if layout not in _WORLDS:
        _WORLDS[layout] = _build_world(gpu, layout == "gapped")
    return _WORLDS[layout]


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    yield _world(gpu, request.param)


@pytest.fixture(scope="module")
def gapped(gpu):
    yield _world(gpu, "gapped")
    _WORLDS.clear()


def _build_world(gpu, gaps):
    import torch

    ctx, dev = gpu
    vals, offs, thr, index, cases = _layout(_cases(), gaps, seed=5 if gaps else 6)
    S = offs.size - 1
    d_vals, d_offs = torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev)
    series = ctx.series(d_vals, d_offs, int(np.diff(offs).max()), gaps)
    full = _launch(ctx, series, thr, S, dev)
    ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
    torch.cuda.synchronize()
    ref = {}
    for name, (x, taus) in cases.items():
        if gaps or not np.isnan(x).any():
            ref[name] = [exceed_one(x, t) for t in taus]
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, thr=thr, index=index, cases=cases, S=S,
                series=series, d_offs=d_offs, full=full, got=_inner(full, S),
                kstats={k: v.cpu().numpy() for k, v in ks.items()}, ref=ref)


def _bits(a, i):
    return int(np.ascontiguousarray(a).reshape(-1)[i:i + 1].view(np.uint64)[0])


def test_layout_covers_both_parities(world):
    offs, index = world["offs"], world["index"]
    for (name, parity), s in index.items():
        assert offs[s] % 2 == parity, name
        assert offs[s + 1] - offs[s] == world["cases"][name][0].size <= 5000
        assert np.array_equal(world["thr"][:, s], np.array(world["cases"][name][1]), equal_nan=True)
    for kind in ("flat", "alt_up", "alt_down", "gamma"):
        assert {n for n, _ in index} >= {f"{kind}{n}" for n in LENGTHS}
    assert world["S"] > 2 * 200


def test_count_and_flags_equal_segmented_stats(world):
    got, ks = world["got"], world["kstats"]
    assert np.array_equal(got["count"], ks["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32))
    for (name, _), s in world["index"].items():
        x = world["cases"][name][0]
        assert got["count"][s] == (np.count_nonzero(~np.isnan(x)) if world["gaps"] else x.size), name
    assert set(np.unique(got["flags"]).tolist()) <= {0, EMPTY, NAN}


def test_integers_equal_the_restatement(world):
    got, fails, checked = world["got"], [], 0
    for (name, parity), s in world["index"].items():
        rows = world["ref"].get(name)
        if rows is None or rows[0]["count"] == 0:
            continue
        assert got["flags"][s] == 0 and got["count"][s] == rows[0]["count"], name
        for r, e in enumerate(rows):
            for k in INT_FIELDS:
                if got[k][r, s] != e[k]:
                    fails.append((name, parity, r, k, int(got[k][r, s]), e[k]))
            checked += 1
    assert not fails, fails[:12]
    assert checked > 4 * 2 * 190


def test_excess_within_the_derived_bound(world):
    """|excess - E| <= m u / (1 - m u) E in rationals; +0.0 bits where nothing is above; +Inf where
    the IEEE sum is.  The worst error / bound is printed (run with -s) before anything is asserted."""
    got, fails, worst, checked, inexact = world["got"], [], (Fraction(0), None), 0, 0
    for (name, parity), s in world["index"].items():
        rows = world["ref"].get(name)
        if rows is None or rows[0]["count"] == 0:
            continue
        for r, e in enumerate(rows):
            g = float(got["excess"][r, s])
            if e["above"] == 0:
                if _bits(got["excess"][r], s) != 0:
                    fails.append((name, parity, r, "not +0.0", g))
            elif not isinstance(e["excess"], Fraction):
                if g != e["excess"]:
                    fails.append((name, parity, r, "not +inf", g))
            else:
                err = abs(Fraction(g) - e["excess"]) if np.isfinite(g) else None
                if err is None or err > e["bound"]:
                    fails.append((name, parity, r, g, float(e["excess"]), float(e["bound"])))
                elif err > 0:
                    inexact += 1
                    if err / e["bound"] > worst[0]:
                        worst = (err / e["bound"], (name, parity, r))
            checked += 1
    print("worst excess error / bound:", float(worst[0]), worst[1], "inexact sums:", inexact)
    assert not fails, fails[:12]
    assert checked > 4 * 2 * 190 and inexact > 50


def test_special_thresholds(world):
    """NaN and +Inf: nothing above, no flag.  -Inf: every present sample above, excess +Inf.  A
    threshold equal to the samples and the signed zeros: the comparison is strict."""
    got, index, cases = world["got"], world["index"], world["cases"]
    for (name, parity), s in index.items():
        x, taus = cases[name]
        n = got["count"][s]
        if got["flags"][s]:
            continue
        for r, t in enumerate(taus):
            if np.isnan(t) or t == INF:
                assert got["above"][r, s] == 0 and got["last"][r, s] == -1 and _bits(got["excess"][r], s) == 0, (name, r)
                assert got["longest"][r, s] == got["head"][r, s] == got["tail"][r, s] == 0
            elif t == -INF and name != "neg_inf_sample":
                assert got["above"][r, s] == got["longest"][r, s] == got["head"][r, s] == got["tail"][r, s] == n
                assert got["excess"][r, s] == INF, (name, r)
    for p in (0, 1):
        for name in ("pos_zero", "neg_zero"):
            s = index[(name, p)]
            assert got["above"][:2, s].tolist() == [0, 0] and got["above"][2, s] == got["count"][s] > 0
            assert got["excess"][2, s] == float(got["count"][s])
        s = index[("flat1025", p)]
        assert got["above"][:, s].tolist() == [0, 0, got["count"][s], got["count"][s]]  # row 1: tau == every sample


def test_flagged_segments(world):
    got, index, gaps = world["got"], world["index"], world["gaps"]
    empties = ["flat0", "gamma0"] + ([f"all_gap{n}" for n in (1, 64, 1025)] if gaps else [])
    for name in empties:
        for p in (0, 1):
            s = index[(name, p)]
            assert got["flags"][s] == EMPTY and got["count"][s] == 0
            for r in range(R):
                assert all(got[k][r, s] == 0 for k in ("above", "longest", "head", "tail")), (name, p, r)
                assert got["last"][r, s] == -1 and _bits(got["excess"][r], s) == 0
    if not gaps:
        for n, _ in NAN_AT:
            for p in (0, 1):
                s = index[(f"nan_sample{n}", p)]
                assert got["flags"][s] == NAN and got["count"][s] == n
                for r in range(R):
                    assert all(got[k][r, s] == 0 for k in ("above", "longest", "head", "tail")), (n, p, r)
                    assert got["last"][r, s] == -1 and _bits(got["excess"][r], s) == QNAN


def test_gapped_integers_equal_the_compacted_series(gapped):
    """Absent slots are transparent: every integer output but ``last`` is that of the same cases
    with the absent slots removed, run through the kernel in the compact layout."""
    import torch

    world = gapped
    ctx, dev, index, cases = world["ctx"], world["dev"], world["index"], world["cases"]
    order = sorted(index, key=index.get)
    segs = [compacted(cases[name][0]) for name, _ in order]
    offs = np.concatenate([[0], np.cumsum([x.size for x in segs])]).astype(np.int64)
    thr = np.ascontiguousarray(world["thr"][:, [index[k] for k in order]])
    series = ctx.series(torch.from_numpy(np.concatenate(segs)).to(dev), torch.from_numpy(offs).to(dev),
                        int(np.diff(offs).max()), False)
    packed = _inner(_launch(ctx, series, thr, len(order), dev), len(order))
    for j, key in enumerate(order):
        s = index[key]
        assert packed["count"][j] == world["got"]["count"][s], key
        for k in ("above", "longest", "head", "tail"):
            assert np.array_equal(packed[k][:, j], world["got"][k][:, s]), (key, k)
        lost = compacted(cases[key[0]][0]).size != cases[key[0]][0].size
        if not lost:
            assert np.array_equal(packed["last"][:, j], world["got"]["last"][:, s]), key


def test_gapped_runs_break_only_at_present_samples(gapped):
    got, index = gapped["got"], gapped["index"]
    for p in (0, 1):
        s, b = index[("sparse_run", p)], index[("sparse_run_broken", p)]
        assert got["longest"][0, s] == got["head"][0, s] == got["tail"][0, s] == got["above"][0, s] == 5
        assert got["last"][0, s] == 1399
        assert got["above"][0, b] == 5 and got["longest"][0, b] == 3 and got["head"][0, b] == 3 and got["tail"][0, b] == 2
        for a, e in ((100, 160), (1000, 1100), (0, 40), (1460, 1500)):
            s, b = index[(f"gap_run{a}_{e}", p)], index[(f"gap_broken{a}_{e}", p)]
            assert got["longest"][0, s] == got["above"][0, s] > 10
            assert got["above"][0, b] == got["above"][0, s] and got["longest"][0, b] < got["longest"][0, s]


def test_four_rows_equal_four_single_launches(world):
    """The bits of row r do not depend on n_thresholds or on the other rows, excess included."""
    ctx, series, S, dev, full = world["ctx"], world["series"], world["S"], world["dev"], _inner(world["full"], world["S"])
    for r in range(R):
        one = _inner(_launch(ctx, series, world["thr"][r:r + 1], S, dev), S)
        for k in FIELDS:
            assert np.array_equal(one[k][0].view(np.uint64), full[k][r].view(np.uint64)), (r, k)
        for k in ("count", "flags"):
            assert np.array_equal(one[k], full[k]), (r, k)
    two = _inner(_launch(ctx, series, world["thr"][[3, 1]], S, dev), S)  # other rows, another order
    for j, r in enumerate((3, 1)):
        for k in FIELDS:
            assert np.array_equal(two[k][j].view(np.uint64), full[k][r].view(np.uint64)), (r, k)
    three = _inner(_launch(ctx, series, world["thr"][:3], S, dev), S)
    for k in FIELDS:
        assert np.array_equal(three[k].view(np.uint64), full[k][:3].view(np.uint64)), k


def _guards_hold(bufs):
    for k, v in bufs.items():
        assert (v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all(), k


def test_two_launches_give_equal_bits_and_guards_hold(world):
    again = _launch(world["ctx"], world["series"], world["thr"], world["S"], world["dev"])
    for k, v in world["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k
    _guards_hold(world["full"])


@pytest.mark.parametrize("want", [("excess",), ("above", "longest"), ("head", "tail", "last"), ()],
                         ids=["excess_only", "above_longest", "ends", "count_flags_only"])
def test_null_outputs(world, want):
    """A NULL per-threshold output is not written, the others are unchanged, and nothing lands
    outside the given buffers."""
    part, full = _launch(world["ctx"], world["series"], world["thr"], world["S"], world["dev"], want=want), world["full"]
    for k in FIELDS + ("count", "flags"):
        if k in want or k in ("count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k
        else:
            assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


def test_argument_errors(gpu, world):
    import ctypes

    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    assert _native.KRR_MAX_THRESHOLDS == 4
    none = (None,) * 9

    def call(h, sp, thr, n, *rest):
        return lib.krr_segmented_exceed(h, sp, thr, n, *rest)

    assert call(None, None, None, 1, *none) == _native.KRR_E_INVALID
    assert call(ctx._h, None, None, 1, *none) == _native.KRR_E_INVALID
    series, S = world["series"], world["S"]
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    thr = torch.zeros(5 * S, dtype=torch.float64, device=dev)
    sp = ctypes.byref(series)
    outs = (None,) * 6
    for n in (0, -1, 5, 64):
        assert call(ctx._h, sp, thr.data_ptr(), n, *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, None, 1, *outs, cnt.data_ptr(), flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, thr.data_ptr(), 1, *outs, None, flg.data_ptr(), None) == _native.KRR_E_INVALID
    assert call(ctx._h, sp, thr.data_ptr(), 1, *outs, cnt.data_ptr(), None, None) == _native.KRR_E_INVALID
    torch.cuda.synchronize()
    assert (cnt == SENTINEL).all() and (flg == SENTINEL).all()  # a refused call launches nothing
    with pytest.raises(_native.NativeError):
        ctx.segmented_exceed(series, thr, 5, None, None, None, None, None, None, cnt, flg)
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert call(ctx._h, ctypes.byref(empty), None, 0, *none) == 0  # nothing to do

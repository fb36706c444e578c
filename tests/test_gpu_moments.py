"""krr_segmented_moments (k_moments) on the MI355X against exact rational arithmetic.

The plan is tests/test_gpu_stats.py's: one series per layout (compact, NaN-gapped with about a
fifth of the slots absent) holds every case, each at an even and at an odd start offset (the
streaming skeleton reads an unaligned first or last sample with the last chunk — the two slots
whose POSITION the kernel has to rebuild), one launch per layout in a module fixture, guarded
output buffers.  The reference and the five bounds are tests/_moments_ref.py's: exact integer
sums of the float64 inputs, one rational division, bounds from Chan, Golub and LeVeque — none of
them measured on the code under test.  The conditioning cases (1e9 + U, 1e12 + 0.01 U) are the ones
a sum-of-squares shortcut misses by orders of magnitude.
"""
from fractions import Fraction

import numpy as np
import pytest

from _moments_ref import FIELDS, bounds, exact_moments, ratios

pytestmark = pytest.mark.gpu

EMPTY, NAN = 4, 1
QNAN = 0x7FF8000000000000
LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17]  # the chunk is 1,024 slots
RAMPS = [(-3, 1500), (0, 1500), (7, 1500), (7, 37), (-3, 2049)]
NAN_AT = ((1, 0), (2, 1), (65, 64), (1500, 3), (2049, 2048))
NONFINITE = ("pos_inf", "neg_inf", "both_inf", "overflow")
GUARD = 8
SENTINEL = -777.25


def _cases():
    """name -> float64 samples (each <= 5,000)."""
    rng = np.random.default_rng(23)
    mem = lambda n: np.floor(rng.normal(2e8, 2e7, n))  # noqa: E731
    cpu = lambda n: rng.gamma(2.0, 0.05, n) * rng.choice([1.0, 1.0, -1.0], n)  # noqa: E731
    cases = {f"len{n}": mem(n) for n in LENGTHS}
    for i, n in enumerate(rng.integers(0, 5001, 200).tolist()):
        cases[f"rand{i}"] = mem(n) if i % 2 == 0 else cpu(n)
    cases["cond1e9"] = 1e9 + rng.random(3000)            # kappa ~ 3e9
    cases["cond1e12"] = 1e12 + 0.01 * rng.random(3000)   # kappa ~ 3e14
    cases["spike_first"] = np.concatenate([[1e6], rng.gamma(2.0, 0.05, 2500)])
    giant = 1e-3 * rng.random(1200)
    giant[777] = 1e15
    cases["giant_among_tiny"] = giant
    cases["constant"] = np.full(777, 2.5)
    cases["noisy_ramp"] = 5e7 + 1e4 * np.arange(4000) + rng.normal(0, 1e6, 4000)
    for b, n in RAMPS:
        cases[f"ramp{b}_{n}"] = 1000.0 + b * np.arange(n, dtype=np.float64)
    cases["pos_inf"] = np.array([1.0, np.inf, 2.0])
    cases["neg_inf"] = np.array([1.0, -np.inf, 2.0] + [0.5] * 100)
    cases["both_inf"] = np.concatenate([cpu(300), [np.inf], cpu(900), [-np.inf], cpu(10)])
    cases["overflow"] = np.array([1e308, 1e308])
    cases["one_negzero"] = np.array([-0.0])
    return cases


def _layout(cases, gaps, seed):
    """Every case at an even and at an odd start offset (one-sample filler segments shift the
    parity).  gaps: about a fifth of the slots of every case become NaN (absent; infinities, the
    1e308 pair and one-slot cases stay), plus a ramp with every other slot absent, lone samples
    among gaps and all-gap segments; compact: NaN samples in segments of their own."""
    rng = np.random.default_rng(seed)
    cases = dict(cases)
    if gaps:
        for name, x in list(cases.items()):
            x = x.copy()
            holes = rng.random(x.size) < 0.2
            holes[(np.abs(x) > 1e307)] = False
            if x.size == 1:
                holes[:] = False
            x[holes] = np.nan
            cases[name] = x
        alt = 1000.0 + 7 * np.arange(2049, dtype=np.float64)
        alt[1::2] = np.nan
        cases["ramp7_alternate"] = alt
        for n, at in ((4, 2), (1500, 1499), (1500, 0), (2050, 1031)):
            x = np.full(n, np.nan)
            x[at] = 5.5
            cases[f"lone{n}_{at}"] = x
        for n in (1, 64, 1025):
            cases[f"all_gap{n}"] = np.full(n, np.nan)
    else:
        for n, at in NAN_AT:
            x = np.floor(rng.normal(2e8, 2e7, n))
            x[at] = np.nan
            cases[f"nan_sample{n}"] = x
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


def _launch(ctx, series, S, dev, want=FIELDS):
    """One launch into guarded buffers; returns {name: whole buffer incl. guards} (host)."""
    import torch

    bufs = {k: torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev) for k in FIELDS}
    bufs["count"] = torch.full((S + 2 * GUARD,), -777, dtype=torch.int64, device=dev)
    bufs["flags"] = torch.full((S + 2 * GUARD,), -777, dtype=torch.int32, device=dev)
    arg = {k: (bufs[k][GUARD:GUARD + S] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.segmented_moments(series, *(arg[k] for k in FIELDS), arg["count"], arg["flags"])
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


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    """The layout's series in HBM, the kernel's outputs (one launch), k_stats' count / flags on the
    same tensors and the exact reference per case (shared by the case's two parities)."""
    import torch

    ctx, dev = gpu
    gaps = request.param == "gapped"
    vals, offs, index, cases = _layout(_cases(), gaps, seed=5 if gaps else 6)
    S = offs.size - 1
    d_vals, d_offs = torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev)
    series = ctx.series(d_vals, d_offs, int(np.diff(offs).max()), gaps)
    full = _launch(ctx, series, S, dev)
    ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
    torch.cuda.synchronize()
    exact = {}
    for name, x in cases.items():
        p = x[~np.isnan(x)]
        if p.size and np.isfinite(p).all() and (gaps or p.size == x.size):
            e = exact_moments(x)
            if e["n"] * e["A"] < 2 ** 1023 and e["Sxx"] < 2 ** 1023:  # "overflow" is finite samples, not a finite case
                exact[name] = e
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, index=index, cases=cases, S=S, series=series,
                full=full, got=_inner(full), kstats={k: v.cpu().numpy() for k, v in ks.items()}, exact=exact)


def _bits(a, s):
    return int(a[s:s + 1].view(np.uint64)[0])


def test_layout_covers_both_parities(world):
    offs, index = world["offs"], world["index"]
    for (name, parity), s in index.items():
        assert offs[s] % 2 == parity, name
        assert offs[s + 1] - offs[s] == world["cases"][name].size <= 5000
    assert {n for n, _ in index} >= {f"len{n}" for n in LENGTHS} and world["S"] > 2 * 230


def test_count_and_flags_equal_segmented_stats(world):
    got, ks = world["got"], world["kstats"]
    assert np.array_equal(got["count"], ks["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32))
    for (name, _), s in world["index"].items():
        x = world["cases"][name]
        assert got["count"][s] == (np.count_nonzero(~np.isnan(x)) if world["gaps"] else x.size), name
    assert set(np.unique(got["flags"]).tolist()) <= {0, EMPTY, NAN}


def test_five_bounds_against_exact_arithmetic(world):
    """Every finite case, both parities: each output within its bound of the exact value.  The
    worst error / bound per output is printed (run with -s) before anything is asserted."""
    got, worst, fails, checked = world["got"], dict.fromkeys(FIELDS, (0.0, None)), [], 0
    for (name, parity), s in world["index"].items():
        e = world["exact"].get(name)
        if e is None:
            continue
        assert got["flags"][s] == 0 and got["count"][s] == e["n"], name
        g = {k: got[k][s] for k in FIELDS}
        assert all(np.isfinite(v) for v in g.values()), (name, parity, g)
        for k, r in ratios(g, e).items():
            if r > worst[k][0]:
                worst[k] = (r, (name, parity))
            if r > 1.0:
                fails.append((name, parity, k, r, g[k], float(e[k])))
        checked += 1
    print("worst error / bound:", {k: (round(r, 4), at) for k, (r, at) in worst.items()})
    assert not fails, fails[:10]
    assert checked > 430


def test_full_segments_match_the_closed_forms(world):
    """Every slot present (all finite cases of the compact layout; the few without a hole of the
    gapped one): tmean = (L - 1) / 2 and t2 = L (L^2 - 1) / 12.  A misplaced head or tail slot
    moves tmean by about 1 and t2 by about L: far outside the bounds."""
    got, checked = world["got"], 0
    for (name, parity), s in world["index"].items():
        e = world["exact"].get(name)
        if e is None or e["n"] != e["L"]:
            continue
        L, b = e["L"], bounds(e)
        assert abs(Fraction(float(got["tmean"][s])) - Fraction(L - 1, 2)) <= b["tmean"], (name, parity)
        assert abs(Fraction(float(got["t2"][s])) - Fraction(L * (L * L - 1), 12)) <= b["t2"], (name, parity)
        checked += 1
    assert checked > (2 if world["gaps"] else 430)


def test_ramp_slopes(world):
    """x = a + b i: cxt / t2 is b up to the two outputs' own bounds propagated through the
    quotient (taken exactly here): |cxt / t2 - b| <= (B_cxt + |b| B_t2) / (T2 - B_t2)."""
    got = world["got"]
    names = [f"ramp{b}_{n}" for b, n in RAMPS] + (["ramp7_alternate"] if world["gaps"] else [])
    for name in names:
        b = int(name[4:].split("_")[0])
        for parity in (0, 1):
            s = world["index"][(name, parity)]
            e = world["exact"][name]
            assert e["cxt"] == b * e["t2"] and e["t2"] > 0  # the reference knows the slope exactly
            B = bounds(e)
            tol = (B["cxt"] + abs(b) * B["t2"]) / (e["t2"] - B["t2"])
            slope = Fraction(float(got["cxt"][s])) / Fraction(float(got["t2"][s]))
            assert abs(slope - b) <= tol, (name, parity, float(slope))
            if b == 0:
                assert got["m2"][s] == 0.0 and got["cxt"][s] == 0.0  # integers below 2^53: exact sums


def test_single_sample_is_exact(world):
    got, index = world["got"], world["index"]
    lone = [("len1", 0, None), ("one_negzero", 0, 1 << 63)]
    if world["gaps"]:
        lone += [("lone4_2", 2, None), ("lone1500_1499", 1499, None), ("lone1500_0", 0, None), ("lone2050_1031", 1031, None)]
    for name, slot, mean_bits in lone:
        x = world["cases"][name]
        for parity in (0, 1):
            s = index[(name, parity)]
            assert got["count"][s] == 1 and got["flags"][s] == 0
            want = mean_bits if mean_bits is not None else _bits(x[~np.isnan(x)], 0)
            assert _bits(got["mean"], s) == want, (name, parity)
            assert got["tmean"][s] == float(slot), (name, parity)
            for k in ("m2", "t2", "cxt"):
                assert _bits(got[k], s) == 0, (name, parity, k)  # +0.0


def test_flagged_segments_hold_the_quiet_nan(world):
    got, index, gaps = world["got"], world["index"], world["gaps"]
    empties = ["len0"] + ([f"all_gap{n}" for n in (1, 64, 1025)] if gaps else [])
    for name in empties:
        for p in (0, 1):
            s = index[(name, p)]
            assert got["flags"][s] == EMPTY and got["count"][s] == 0
            assert all(_bits(got[k], s) == QNAN for k in FIELDS), (name, p)
    if not gaps:
        for n, _ in NAN_AT:
            for p in (0, 1):
                s = index[(f"nan_sample{n}", p)]
                assert got["flags"][s] == NAN and got["count"][s] == n
                assert all(_bits(got[k], s) == QNAN for k in FIELDS), (n, p)


def test_non_finite_samples_are_plain_ieee(world):
    """No flag; mean and m2 non-finite; tmean and t2 depend only on which slots are present."""
    got, index = world["got"], world["index"]
    for name in NONFINITE:
        x = world["cases"][name]
        e = exact_moments(np.where(np.isnan(x), np.nan, 1.0))  # the slots' own moments
        for p in (0, 1):
            s = index[(name, p)]
            assert got["flags"][s] == 0 and got["count"][s] == e["n"], name
            assert not np.isfinite(got["mean"][s]) and not np.isfinite(got["m2"][s]), (name, p)
            r = ratios({"tmean": got["tmean"][s], "t2": got["t2"][s]}, e)
            assert r["tmean"] <= 1.0 and r["t2"] <= 1.0, (name, p, r)


def test_two_launches_give_equal_bits(world):
    again = _launch(world["ctx"], world["series"], world["S"], world["dev"])
    for k, v in world["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k


def _guards_hold(bufs):
    for k, v in bufs.items():
        sentinel = -777 if v.dtype.kind == "i" else SENTINEL
        assert (v[:GUARD] == sentinel).all() and (v[-GUARD:] == sentinel).all(), k


def test_no_trend_launch_equals_the_full_one(world):
    part, full = _launch(world["ctx"], world["series"], world["S"], world["dev"], want=("mean", "m2")), world["full"]
    for k in ("mean", "m2", "count", "flags"):
        assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k  # guards included
    for k in ("tmean", "t2", "cxt"):
        assert (part[k] == SENTINEL).all(), k
    _guards_hold(full)


@pytest.mark.parametrize("want", [("m2", "tmean", "t2", "cxt"), ("mean", "tmean", "t2", "cxt"), ("m2",), ()],
                         ids=["no_mean", "no_m2", "m2_only", "count_flags_only"])
def test_null_outputs(world, want):
    """A NULL out_mean / out_m2 is not written, the others are unchanged, and nothing lands
    outside the given buffers."""
    part, full = _launch(world["ctx"], world["series"], world["S"], world["dev"], want=want), world["full"]
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
    none8 = (None,) * 8
    assert lib.krr_segmented_moments(None, None, *none8) == _native.KRR_E_INVALID
    assert lib.krr_segmented_moments(ctx._h, None, *none8) == _native.KRR_E_INVALID
    series, S = world["series"], world["S"]
    cnt = torch.empty(S, dtype=torch.int64, device=dev)
    flg = torch.empty(S, dtype=torch.int32, device=dev)
    d = [torch.empty(S, dtype=torch.float64, device=dev) for _ in range(3)]
    sp = ctypes.byref(series)
    assert lib.krr_segmented_moments(ctx._h, sp, None, None, None, None, None, cnt.data_ptr(), None,
                                     None) == _native.KRR_E_INVALID  # out_flags is required
    assert lib.krr_segmented_moments(ctx._h, sp, None, None, None, None, None, None, flg.data_ptr(),
                                     None) == _native.KRR_E_INVALID  # out_count is required
    for missing in range(3):  # one of the three trend outputs NULL
        ptrs = [None if j == missing else t.data_ptr() for j, t in enumerate(d)]
        assert lib.krr_segmented_moments(ctx._h, sp, None, None, *ptrs, cnt.data_ptr(), flg.data_ptr(),
                                         None) == _native.KRR_E_INVALID
    ptrs = [d[0].data_ptr(), None, None]  # two of them NULL
    assert lib.krr_segmented_moments(ctx._h, sp, None, None, *ptrs, cnt.data_ptr(), flg.data_ptr(),
                                     None) == _native.KRR_E_INVALID
    with pytest.raises(ValueError, match="all three or none"):
        ctx.segmented_moments(series, None, None, d[0], None, d[2], cnt, flg)
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert lib.krr_segmented_moments(ctx._h, ctypes.byref(empty), *none8) == 0  # nothing to do

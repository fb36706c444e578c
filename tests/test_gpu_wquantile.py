"""krr_segmented_wquantile (k_wquantile) on the MI355X against the plain restatement.

The plan is tests/test_gpu_exceed.py's: one series per layout (compact, NaN-gapped with about a
fifth of the slots absent) holds every case, each at an even and at an odd start offset with
one-sample filler segments between (the streaming skeleton reads an unaligned first or last
sample with the last chunk: the two slots whose AGE the kernel has to get right), guarded output
buffers, one launch per (table, percentile) kept by a module fixture.  The truth is
tests/_wquantile_ref.py's, in Python integers.  Everything is compared for EQUALITY: the value's
bits, the total weight, and count and flags against krr_segmented_stats.  There is no tolerance.
``passes`` is held to the bound derived from the bin count (1 + ceil(64 / 10) + 1 = 9)."""
import numpy as np
import pytest

from _wquantile_ref import EMPTY, MAX_PASSES, NAN, QNAN, Sorted, bits, fraction_of
from krr_amd.api import decay_weights, window_weights  # noqa: F401  (the feature: absent, nothing here runs)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17]
NAN_AT = ((1, 0), (2, 1), (65, 64), (1500, 3), (2049, 2048))
GUARD = 8
SENTINEL = -777
INF = float("inf")
PERCENTILES = ("0.000000001", "50", "99", "100")
SINGLE_AGES = (0, 1, 2, 63, 64, 127, 128, 1023, 1024)  # age L - 1 of the lengths 1, 2, 3, 64, ...: slot 0


def _tables():
    """name -> (uint64 table, percentiles asked with it)."""
    from krr_amd.api import decay_weights, window_weights

    longest = max(LENGTHS)
    tables = {
        "unit": (np.array([1], np.uint64), PERCENTILES),
        "decay64": (decay_weights(64, longest), PERCENTILES),
        "decay700": (decay_weights(700, longest), PERCENTILES),
        "window100": (window_weights(100, longest), PERCENTILES),
        "short": (np.array([7, 0, 2 ** 32, 3, 0, 5], np.uint64), PERCENTILES),  # shorter than most series: the clamp
        "zero": (np.zeros(4, np.uint64), ("50",)),
    }
    for a in SINGLE_AGES:  # one positive weight at one age, nothing older: the answer is that slot's sample
        t = np.zeros(a + 2, np.uint64)
        t[a] = 3
        tables[f"single{a}"] = (t, ("50",))
    return tables


def _cases():
    """name -> float64 samples (<= 3,100)."""
    rng = np.random.default_rng(41)
    cases = {}
    for n in LENGTHS:
        cases[f"gamma{n}"] = rng.gamma(2.0, 0.05, n)                 # CPU-like
        cases[f"mem{n}"] = np.floor(rng.normal(2e8, 2e7, n))         # memory-like: integers, ties
        cases[f"ramp{n}"] = np.arange(n, dtype=np.float64)           # distinct: the answer names its slot
    cases["knife100"] = rng.permutation(100).astype(np.float64)      # unit weights, p50: C den == W num at 49.0
    cases["narrow3000"] = 1e9 + rng.random(3000)                     # many keys in a narrow range
    x = 1e9 + rng.random(3000)
    x[[7, 1500, 2999]] = [-1e300, 1e300, 5e-324]                     # ... and a key range of 2^64: the first
    cases["narrow_outliers"] = x                                     # histogram's bin holds them all, narrowed again
    x = np.zeros(2500)
    x[rng.integers(0, 2500, 40)] = rng.gamma(2.0, 5.0, 40)
    cases["mostly_zero"] = x                                         # one key above the collect capacity
    cases["all_equal"] = np.full(1500, 0.25)
    cases["ties"] = rng.integers(1, 4, 999).astype(np.float64)       # three keys: ties straddle every target
    cases["zeros_mp"] = np.where(np.arange(200) % 2 == 0, -0.0, 0.0)
    cases["zeros_pm"] = np.where(np.arange(201) % 2 == 0, 0.0, -0.0)
    x = rng.normal(0, 1, 300)
    x[rng.integers(0, 300, 30)] = INF
    x[rng.integers(0, 300, 30)] = -INF
    cases["infs"] = x
    cases["all_inf"] = np.full(130, INF)
    cases["denormals"] = rng.integers(-50, 50, 700).astype(np.float64) * 5e-324
    return cases


def _layout(cases, gaps, seed):
    rng = np.random.default_rng(seed)
    cases = dict(cases)
    if gaps:
        for name, x in list(cases.items()):
            x = x.copy()
            holes = rng.random(x.size) < 0.2
            if x.size == 1:
                holes[:] = False
            x[holes] = np.nan
            cases[name] = x
        for n, at in ((4, 2), (1500, 1499), (1500, 0), (2050, 1031), (1025, 1)):
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


def _launch(ctx, series, table, p, S, dev, want=("wsum", "passes")):
    """One launch into guarded buffers; {name: whole buffer incl. guards} as host arrays."""
    import torch

    d_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64)).to(dev)
    dt = {"value": torch.float64, "wsum": torch.int64, "passes": torch.int32, "count": torch.int64, "flags": torch.int32}
    bufs = {k: torch.full((S + 2 * GUARD,), SENTINEL, dtype=t, device=dev) for k, t in dt.items()}
    arg = {k: (v[GUARD:-GUARD] if k in want or k in ("value", "count", "flags") else None) for k, v in bufs.items()}
    ctx.segmented_wquantile(series, d_tab, *fraction_of(p), arg["value"], arg["wsum"], arg["passes"], arg["count"],
                            arg["flags"])
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


_WORLDS = {}


def _build_world(gpu, gaps):
    import torch

    ctx, dev = gpu
    vals, offs, index, cases = _layout(_cases(), gaps, seed=5 if gaps else 6)
    S = offs.size - 1
    d_vals, d_offs = torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev)
    series = ctx.series(d_vals, d_offs, int(np.diff(offs).max()), gaps)
    tables = _tables()
    full = {(t, p): _launch(ctx, series, tab, p, S, dev) for t, (tab, ps) in tables.items() for p in ps}
    ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
    torch.cuda.synchronize()
    ref = {name: Sorted(x) for name, x in cases.items() if gaps or not np.isnan(x).any()}  # sorted once, shared
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, index=index, cases=cases, S=S, series=series,
                tables=tables, full=full, got={k: _inner(v) for k, v in full.items()},
                kstats={k: v.cpu().numpy() for k, v in ks.items()}, ref=ref)


def _world(gpu, layout):
    """The layout's series in HBM, every (table, percentile) launch, k_stats' count / flags on the
    same tensors and the cases sorted once for the restatement.  Built once per layout."""
    if layout not in _WORLDS:
        _WORLDS[layout] = _build_world(gpu, layout == "gapped")
    return _WORLDS[layout]


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    yield _world(gpu, request.param)


@pytest.fixture(scope="module")
def compact(gpu):
    yield _world(gpu, "compact")
    _WORLDS.clear()


def _vbits(got, s):
    return int(got["value"][s:s + 1].view(np.uint64)[0])


def test_layout_covers_both_parities(world):
    offs, index = world["offs"], world["index"]
    for (name, parity), s in index.items():
        assert offs[s] % 2 == parity, name
        assert offs[s + 1] - offs[s] == world["cases"][name].size <= 3100
    for kind in ("gamma", "mem", "ramp"):
        assert {n for n, _ in index} >= {f"{kind}{n}" for n in LENGTHS}
    assert len(world["full"]) == 5 * len(PERCENTILES) + 1 + len(SINGLE_AGES)


def test_count_and_flags_equal_segmented_stats(world):
    ks = world["kstats"]
    for key, got in world["got"].items():
        assert np.array_equal(got["count"], ks["count"]), key
        assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32)), key
    assert set(np.unique(ks["flags"]).tolist()) <= {0, EMPTY, NAN}
    assert (ks["flags"] == (EMPTY if world["gaps"] else NAN)).sum() >= 6


def test_value_bits_and_wsum_equal_the_restatement(world):
    fails, checked, answered = [], 0, 0
    for (t, p), got in world["got"].items():
        table, frac = world["tables"][t][0], fraction_of(p)
        for (name, parity), s in world["index"].items():
            ref = world["ref"].get(name)
            if ref is None:
                continue  # a NaN sample in the compact layout: test_flagged_segments
            b, W = ref.answer(table, *frac)
            if _vbits(got, s) != b or int(got["wsum"][s]) != W:
                fails.append((t, p, name, parity, hex(_vbits(got, s)), hex(b), int(got["wsum"][s]), W))
            checked += 1
            answered += W > 0
    assert not fails, (len(fails), fails[:10])
    assert checked > 30 * 2 * 55 and answered > checked // 3


def test_passes_within_the_derived_bound(world):
    """1 <= passes <= 1 + ceil(64 / log2(bins)) + 1 everywhere; one pass where pass 0 settles it.  The
    statistics are printed (run with -s) before anything is asserted."""
    index, allp = world["index"], np.concatenate([g["passes"] for g in world["got"].values()])
    print("passes: mean", float(allp.mean()), "max", int(allp.max()), "histogram", np.bincount(allp).tolist())
    assert allp.min() >= 1 and allp.max() <= MAX_PASSES == 9
    unit = world["got"][("unit", "50")]
    for p in (0, 1):
        assert unit["passes"][index[("all_equal", p)]] == 1          # lo == hi after the totals
        assert unit["passes"][index[("all_inf", p)]] == 1
        assert unit["passes"][index[("gamma0", p)]] == 1             # empty
        assert unit["passes"][index[("gamma129", p)]] == 2           # within the collect capacity: totals, collect
        assert unit["passes"][index[("mostly_zero", p)]] == 3        # totals, the bin of zeros, the bin is one key
        assert unit["passes"][index[("narrow_outliers", p)]] >= 4    # two histograms before the collect
    zero = world["got"][("zero", "50")]
    assert (zero["passes"] == 1).all() and (zero["wsum"] == 0).all()
    assert (zero["value"].view(np.uint64) == QNAN).all()             # no weight: the quiet NaN, flags as k_stats'


def test_window_equals_unit_weights_on_the_last_100_slots(world):
    checked = 0
    for p in PERCENTILES:
        got, frac = world["got"][("window100", p)], fraction_of(p)
        for (name, parity), s in world["index"].items():
            if name not in world["ref"]:
                continue
            b, W = Sorted(world["cases"][name][-100:]).answer([1], *frac)
            assert (_vbits(got, s), int(got["wsum"][s])) == (b, W), (p, name, parity)
            checked += 1
    assert checked > 4 * 2 * 55


def test_single_weight_names_its_slot(world):
    """One positive weight at age a: the answer is slot L - 1 - a's sample (ramp: the slot index
    itself), the quiet NaN when the series is shorter or the slot absent.  L = a + 1 is slot 0: the
    unaligned head slot at an odd offset; age 0 the tail slot."""
    for a in SINGLE_AGES:
        got = world["got"][(f"single{a}", "50")]
        for n in LENGTHS:
            for parity in (0, 1):
                s = world["index"][(f"ramp{n}", parity)]
                x = world["cases"][f"ramp{n}"]
                want = x[n - 1 - a] if n > a else np.nan
                if np.isnan(want):
                    assert _vbits(got, s) == QNAN and got["wsum"][s] == 0, (a, n, parity)
                else:
                    assert got["value"][s] == want == n - 1 - a and got["wsum"][s] == 3, (a, n, parity)
                    assert got["passes"][s] == 1


def test_knife_edge_and_signed_zeros(compact):
    """Exact counts of unit weights: the compact layout."""
    index, unit = compact["index"], compact["got"]
    for p in (0, 1):
        s = index[("knife100", p)]
        assert unit[("unit", "50")]["value"][s] == 49.0 and unit[("unit", "50")]["wsum"][s] == 100  # >=, not >
        assert unit[("unit", "100")]["value"][s] == 99.0 and unit[("unit", "0.000000001")]["value"][s] == 0.0
        assert _vbits(unit[("unit", "50")], index[("zeros_mp", p)]) == bits(-0.0)   # 100 of each: C(-0.0) is half
        assert _vbits(unit[("unit", "50")], index[("zeros_pm", p)]) == bits(0.0)    # 100 -0.0 of 201: short of half
        assert _vbits(unit[("unit", "100")], index[("zeros_mp", p)]) == bits(0.0)
        assert _vbits(unit[("unit", "0.000000001")], index[("zeros_pm", p)]) == bits(-0.0)
        assert unit[("unit", "100")]["value"][index[("infs", p)]] == INF
        assert unit[("unit", "0.000000001")]["value"][index[("infs", p)]] == -INF


def test_flagged_segments(world):
    index, gaps = world["index"], world["gaps"]
    empties = ["gamma0", "mem0", "ramp0"] + ([f"all_gap{n}" for n in (1, 64, 1025)] if gaps else [])
    for key, got in world["got"].items():
        for name in empties:
            for p in (0, 1):
                s = index[(name, p)]
                assert got["flags"][s] == EMPTY and got["count"][s] == 0 and got["wsum"][s] == 0, (key, name)
                assert _vbits(got, s) == QNAN and got["passes"][s] == 1
        if not gaps:
            for n, _ in NAN_AT:
                for p in (0, 1):
                    s = index[(f"nan_sample{n}", p)]
                    assert got["flags"][s] == NAN and got["count"][s] == n and got["wsum"][s] == 0, (key, n)
                    assert _vbits(got, s) == QNAN and got["passes"][s] == 1
    if gaps:
        got = world["got"][("unit", "50")]
        for n, at in ((4, 2), (1500, 1499), (1500, 0), (2050, 1031), (1025, 1)):
            for p in (0, 1):
                s = index[(f"lone{n}_{at}", p)]
                assert got["value"][s] == 5.5 and got["wsum"][s] == 1 and got["count"][s] == 1 and got["passes"][s] == 1


def test_same_bits_at_either_parity_and_on_a_second_launch(world):
    """Integer sums: the same samples give the same bits at an even and at an odd offset, and the
    whole launch repeats bit for bit; nothing lands outside the buffers."""
    for key, got in world["got"].items():
        for (name, parity), s in world["index"].items():
            if parity == 0:
                o = world["index"][(name, 1)]
                assert _vbits(got, s) == _vbits(got, o) and got["wsum"][s] == got["wsum"][o], (key, name)
                assert got["passes"][s] == got["passes"][o], (key, name)
    for key in (("decay64", "50"), ("unit", "99")):
        again = _launch(world["ctx"], world["series"], world["tables"][key[0]][0], key[1], world["S"], world["dev"])
        for k, v in world["full"][key].items():
            assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), (key, k)
    for key, bufs in world["full"].items():
        for k, v in bufs.items():
            assert (v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all(), (key, k)


@pytest.mark.parametrize("want", [("wsum",), ("passes",), ()], ids=["wsum_only", "passes_only", "neither"])
def test_null_outputs(world, want):
    key = ("decay700", "99")
    part = _launch(world["ctx"], world["series"], world["tables"][key[0]][0], key[1], world["S"], world["dev"], want=want)
    for k, v in world["full"][key].items():
        if k in want or k in ("value", "count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), v.view(np.uint8)), k
        else:
            assert (part[k] == SENTINEL).all(), k


def test_argument_errors(gpu, world):
    import ctypes

    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    call = lib.krr_segmented_wquantile
    E = _native.KRR_E_INVALID
    assert call(None, None, None, 1, 50, 1, *(None,) * 6) == E
    assert call(ctx._h, None, None, 1, 50, 1, *(None,) * 6) == E
    series, S = world["series"], world["S"]
    val = torch.full((S,), SENTINEL, dtype=torch.float64, device=dev)
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    tab = torch.ones(4, dtype=torch.int64, device=dev)
    sp, t, v, c, f = ctypes.byref(series), tab.data_ptr(), val.data_ptr(), cnt.data_ptr(), flg.data_ptr()
    assert call(ctx._h, sp, None, 4, 50, 1, v, None, None, c, f, None) == E            # null age_weights
    for n in (0, -1):
        assert call(ctx._h, sp, t, n, 50, 1, v, None, None, c, f, None) == E            # n_weights < 1
    for num, den in ((0, 1), (-5, 1), (50, 0), (50, -1), (101, 1), (100 * 7 + 1, 7), (1, 10 ** 15 + 1)):
        assert call(ctx._h, sp, t, 4, num, den, v, None, None, c, f, None) == E, (num, den)
    assert call(ctx._h, sp, t, 4, 50, 1, None, None, None, c, f, None) == E            # a required output NULL
    assert call(ctx._h, sp, t, 4, 50, 1, v, None, None, None, f, None) == E
    assert call(ctx._h, sp, t, 4, 50, 1, v, None, None, c, None, None) == E
    torch.cuda.synchronize()
    assert (val == SENTINEL).all() and (cnt == SENTINEL).all() and (flg == SENTINEL).all()  # nothing launched
    with pytest.raises(_native.NativeError):
        ctx.segmented_wquantile(series, tab, 101, 1, val, None, None, cnt, flg)
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert call(ctx._h, ctypes.byref(empty), None, 0, 0, 0, *(None,) * 6) == 0  # nothing to do
    # the bounds themselves are accepted: p = 100 and p_den = 10^15
    assert call(ctx._h, sp, t, 4, 100, 1, v, None, None, c, f, None) == 0
    assert call(ctx._h, sp, t, 4, 1, 10 ** 15, v, None, None, c, f, None) == 0
    torch.cuda.synchronize()

"""krr_pods_overlay (k_overlay) on the MI355X against the plain restatement, bit for bit.

One fleet per layout (compact; NaN-gapped with about 30% of the slots absent) holds the shapes at
which the kernel can go wrong: a tile is 8 rows of 64 slots (16 rows for an object with one pod),
so pod lengths sit on both sides of a row, of two rows and of a tile, and 2049 / 4099 exceed twice
any tile; the pods come two at a time, so pod counts are odd and even, and 64 / 65 / 130 of them
cross the lanes of the pass that finds the longest pod; mixed lengths inside an object put the
END shift Lg - Lp on both sides of a row.  The whole fleet is launched a second time behind a
one-slot filler pod, which flips the parity of every pod's start: the per-slot outputs must not
change by a bit.  The truth is tests/_overlay_ref.py's loops; the sum has ONE order, so there is no
tolerance anywhere.  One launch per (layout, align, placement) is shared by the tests."""
import numpy as np
import pytest

from _overlay_ref import CAPACITY, EMPTY, END, NAN, START, np_overlay

pytestmark = pytest.mark.gpu

QNAN = 0x7FF8000000000000
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049, 4099]
SHORT = [0, 1, 2, 63, 64, 65]
SHIFTS = [1, 2, 63, 64, 65, 127, 128, 129]
POD_COUNTS = [0, 1, 2, 3, 5, 17, 64, 65, 130]
ALIGNS = {"start": START, "end": END}
STATS = ("sum", "max", "min", "active")
GUARD = 8
SENTINEL = -777
INF = float("inf")


def _shapes():
    """name -> the pod lengths of one object."""
    rng = np.random.default_rng(5)
    shapes = {"none_first": []}
    for n in LENGTHS:
        shapes[f"one{n}"] = [n]
        shapes[f"two{n}"] = [n, n]
    for d in SHIFTS:  # Lg - Lp = d, the longest pod first, in the middle and last
        for L in (d, 1025):
            shapes[f"shift{d}_{L}_first"] = [L, L - d, L - d]
            shapes[f"shift{d}_{L}_mid"] = [L - d, L, L - d]
            shapes[f"shift{d}_{L}_last"] = [L - d, L - d, L]
        shapes[f"shift{d}_4099"] = [4099 - d, 4099, 4099 - d]
    shapes["none_mid"] = []
    shapes["three"] = [1024, 129, 1025]
    shapes["five"] = [1023, 0, 1025, 64, 2]
    shapes["five_long"] = [2049] * 5
    shapes["three_long"] = [4099, 2049, 4099]
    shapes["seventeen"] = [int(x) for x in rng.choice(LENGTHS[:9], 17)]
    for k in (64, 65, 130):
        lens = [int(x) for x in rng.choice(SHORT, k)]
        lens[-1] = 65  # the longest pod in the last lane's reach
        shapes[f"many{k}"] = lens
    shapes["zeros"] = [130, 130, 130]
    shapes["inf"] = [70, 70, 70]
    shapes["absent_pod"] = [200, 200, 200]
    shapes["nan_sample"] = [300, 129, 300]
    shapes["none_last"] = []
    return shapes


def _fleet(gaps):
    """The fleet's values, pod offsets and groups, and name -> object."""
    rng = np.random.default_rng(29 if gaps else 30)
    shapes = _shapes()
    pods, groups, index = [], [0], {}
    for name, lens in shapes.items():
        index[name] = len(groups) - 1
        for k, n in enumerate(lens):
            x = rng.gamma(2.0, 0.05, n)
            x[rng.random(n) < 0.05] = 0.0  # +-0.0 ties across pods at the same slot
            x[rng.random(n) < 0.05] = -0.0
            if name == "zeros":
                x[:] = (-0.0, 0.0, -0.0)[k]
                x[k::3] = 0.0
                x[40:60] = (0.0, -0.0, 0.0)[k]
            if name == "inf":
                x[3] = (INF, -INF, 1.0)[k]  # a NaN sum
                x[5] = (INF, INF, 1.0)[k]
                x[7] = (2.0, -INF, 1.0)[k]
                x[69] = (-INF, 2.0, INF)[k]
            if gaps:
                if n > 1:
                    x[rng.random(n) < 0.3] = np.nan
                if name == "absent_pod":
                    if k == 1:
                        x[:] = np.nan  # an all-absent pod
                    x[90:110] = np.nan  # slots no pod has a sample at
            elif name == "nan_sample":
                x[(0, 128, 299)[k]] = np.nan
            pods.append(x)
        groups.append(len(pods))
    pod_offs = np.concatenate([[0], np.cumsum([p.size for p in pods])]).astype(np.int64)
    return np.concatenate(pods), pod_offs, np.asarray(groups, dtype=np.int64), index, shapes


def _shifted(vals, pod_offs, groups):
    """The same fleet behind a one-slot filler pod in an object of its own."""
    return (np.concatenate([[7.0], vals]), np.concatenate([[0], pod_offs + 1]).astype(np.int64),
            np.concatenate([[0], groups + 1]).astype(np.int64))


def _launch(world, align, ooffs, want=STATS):
    """One launch into guarded, sentinel-filled buffers; {name: whole buffer incl. guards}."""
    import torch

    ctx, dev, S = world["ctx"], world["dev"], world["S"]
    n = int(ooffs.max())
    bufs = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32 if k == "active" else torch.float64,
                          device=dev) for k in STATS}
    bufs["count"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    bufs["flags"] = torch.full((S + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    arg = {k: (bufs[k][GUARD:-GUARD] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.pods_overlay(world["series"], world["d_groups"], S, align, torch.from_numpy(ooffs).to(dev), arg["sum"],
                     arg["max"], arg["min"], arg["active"], arg["count"], arg["flags"])
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


def _world(gpu, layout, shifted=False):
    if (layout, shifted) not in _WORLDS:
        import torch

        ctx, dev = gpu
        gaps = layout == "gapped"
        vals, pod_offs, groups, index, shapes = _fleet(gaps)
        if shifted:
            vals, pod_offs, groups = _shifted(vals, pod_offs, groups)
        S = groups.size - 1
        d_vals = torch.from_numpy(vals).to(dev)
        series = ctx.series(d_vals, torch.from_numpy(pod_offs).to(dev), int(np.diff(pod_offs).max()), gaps)
        obj_offs = pod_offs[groups]  # the pod segments tile this object-level series
        objects = ctx.series(d_vals, torch.from_numpy(obj_offs).to(dev), int(np.diff(obj_offs).max()), gaps)
        ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
        ctx.segmented_stats(objects, None, None, None, ks["count"], ks["flags"])
        torch.cuda.synchronize()
        _WORLDS[(layout, shifted)] = dict(
            ctx=ctx, dev=dev, gaps=gaps, vals=vals, pod_offs=pod_offs, groups=groups, index=index, shapes=shapes, S=S,
            series=series, d_groups=torch.from_numpy(groups).to(dev), kstats={k: v.cpu().numpy() for k, v in ks.items()})
    return _WORLDS[(layout, shifted)]


def _run(gpu, layout, align, shifted=False):
    """The restatement and one full launch of a combination, built once."""
    key = (layout, align, shifted)
    if key not in _RUNS:
        world = _world(gpu, layout, shifted)
        ref = np_overlay(world["vals"], world["pod_offs"], world["groups"], ALIGNS[align], world["gaps"])
        full = _launch(world, ALIGNS[align], ref["offsets"])
        _RUNS[key] = dict(world=world, ref=ref, full=full, got=_inner(full))
    return _RUNS[key]


@pytest.fixture(scope="module", params=["compact", "gapped"])
def layout(request):
    return request.param


@pytest.fixture(scope="module", params=list(ALIGNS))
def align(request):
    return request.param


@pytest.fixture(scope="module")
def run(gpu, layout, align):
    return _run(gpu, layout, align)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _guards_hold(bufs):
    for k, v in bufs.items():
        assert (v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all(), k


def _same_slots(got, ref, where=slice(None)):
    assert np.array_equal(got["active"].view(np.uint32)[where], ref["active"][where])
    for k in ("sum", "max", "min"):
        bad = np.flatnonzero(_u64(got[k])[where] != _u64(ref[k])[where])
        assert bad.size == 0, (k, bad[:8], got[k][where][bad[:8]], ref[k][where][bad[:8]])


def test_fleet_covers_the_shapes(gpu, layout):
    world = _world(gpu, layout)
    lens, groups = np.diff(world["pod_offs"]), world["groups"]
    assert world["vals"].size < 1_000_000
    assert set(lens.tolist()) >= set(LENGTHS)
    assert set(np.diff(groups).tolist()) >= set(POD_COUNTS)
    shifts = set()
    for g in range(world["S"]):
        own = lens[groups[g]:groups[g + 1]]
        shifts |= set((own.max(initial=0) - own).tolist())
    assert shifts >= set(SHIFTS)
    if world["gaps"]:
        x = world["vals"]
        assert abs(np.isnan(x).mean() - 0.3) < 0.05
    flipped = _world(gpu, layout, shifted=True)
    assert ((flipped["pod_offs"][1:-1] - world["pod_offs"][:-1]) == 1).all()


def test_every_output_equals_the_restatement(run):
    ref, got = run["ref"], run["got"]
    assert ref["written"].all() and got["active"].size == int(ref["offsets"][-1])
    _same_slots(got, ref)
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ref["flags"])
    _guards_hold(run["full"])
    empty = ref["active"] == 0
    assert (_u64(got["max"])[empty] == QNAN).all() and (_u64(got["min"])[empty] == QNAN).all()
    assert (_u64(got["sum"])[empty] == 0).all()  # +0.0
    if run["world"]["gaps"]:
        assert empty.any()  # slots no pod has a sample at occur


def test_the_other_parity_gives_equal_bits(gpu, layout, align):
    """Behind a one-slot filler pod every pod starts at the other parity: the objects' slots keep
    their bits, and the shifted launch equals the restatement of the shifted fleet."""
    a, b = _run(gpu, layout, align), _run(gpu, layout, align, shifted=True)
    _same_slots(b["got"], b["ref"])
    assert b["ref"]["offsets"][1] == 1 and b["got"]["sum"][0] == 7.0 and b["got"]["active"][0] == 1
    for k in STATS:
        assert np.array_equal(a["got"][k].view(np.uint8), b["got"][k][1:].view(np.uint8)), k
    assert np.array_equal(a["got"]["count"], b["got"]["count"][1:])
    assert np.array_equal(a["got"]["flags"], b["got"]["flags"][1:])
    _guards_hold(b["full"])


def test_count_and_flags_equal_segmented_stats(run):
    got, ks = run["got"], run["world"]["kstats"]
    assert np.array_equal(got["count"], ks["count"])
    assert np.array_equal(got["flags"].view(np.uint32), ks["flags"].view(np.uint32))


def test_two_launches_give_equal_bits(run, align):
    again = _launch(run["world"], ALIGNS[align], run["ref"]["offsets"])
    for k, v in run["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("want", [("sum", "active"), ("sum",), ("max",), ("min",), ("max", "min"), ("active",),
                                  ("sum", "max", "min"), ("sum", "min", "active"), ()],
                         ids=["sum_active", "sum", "max", "min", "max_min", "active", "no_active", "no_max",
                              "count_flags_only"])
def test_null_outputs(run, align, want):
    """A NULL per-slot output is not written, the others hold the full launch's bits, and nothing
    lands outside the given buffers."""
    part, full = _launch(run["world"], ALIGNS[align], run["ref"]["offsets"], want=want), run["full"]
    for k in STATS + ("count", "flags"):
        if k in want or k in ("count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k
        else:
            assert (part[k] == SENTINEL).all(), k
    _guards_hold(part)


def test_special_values(gpu, layout, align):
    """Zero ties keep the earlier pod's zero, infinities are plain IEEE, a compact NaN sample makes
    exactly its slot NaN and flags the object, an all-absent pod counts nowhere."""
    r = _run(gpu, layout, align)
    world, ref, got = r["world"], r["ref"], r["got"]
    gaps, index = world["gaps"], world["index"]
    o = int(ref["offsets"][index["zeros"]])
    live = got["active"][o:o + 130] > 0
    assert live.any() and (got["max"][o:o + 130][live] == 0).all() and (got["min"][o:o + 130][live] == 0).all()
    assert {0, 1 << 63} == set(_u64(got["max"][o:o + 130])[live].tolist())  # both zeros win somewhere
    if not gaps:
        o = int(ref["offsets"][index["inf"]])
        assert int(_u64(got["sum"][o + 3:o + 4])[0]) == QNAN and got["max"][o + 3] == INF and got["min"][o + 3] == -INF
        assert got["sum"][o + 5] == INF and got["sum"][o + 7] == -INF
        assert int(_u64(got["sum"][o + 69:o + 70])[0]) == QNAN
        assert got["flags"][index["inf"]] == 0
        g = index["nan_sample"]
        o = int(ref["offsets"][g])
        shift = 171 if align == "end" else 0
        hit = {0, 128 + shift, 299}
        for j in range(300):
            for k in ("sum", "max", "min"):
                assert (int(_u64(got[k][o + j:o + j + 1])[0]) == QNAN) == (j in hit), (j, k)
            assert got["active"][o + j] == 2 + (shift <= j < shift + 129)
        assert got["flags"][g] == NAN and got["count"][g] == 729
        assert (got["flags"][np.arange(world["S"]) != g] & NAN == 0).all()
    else:
        g = index["absent_pod"]
        o = int(ref["offsets"][g])
        assert got["active"][o:o + 200].max() <= 2 and (got["active"][o + 90:o + 110] == 0).all()
        assert (got["flags"] & NAN == 0).all()
    for name in ("none_first", "none_mid", "none_last"):
        g = index[name]
        assert got["flags"][g] == EMPTY and got["count"][g] == 0 and ref["slots"][g] == 0


def test_small_span_sets_capacity_and_writes_nothing(gpu, layout, align):
    """out_offsets with slack everywhere (any layout with at least Lg entries is allowed) and one
    entry too few for some objects: those get KRR_FLAG_CAPACITY and keep the sentinels, with count
    and the other flags as otherwise; the others are written at their own offsets."""
    r = _run(gpu, layout, align)
    world, Lg = r["world"], r["ref"]["slots"]
    victims = [g for g in range(world["S"]) if Lg[g] > 0 and g % 5 == 2]
    span = Lg + 1
    span[victims] = Lg[victims] - 1
    ooffs = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    ref = np_overlay(world["vals"], world["pod_offs"], world["groups"], ALIGNS[align], world["gaps"], out_offsets=ooffs)
    got = _launch(world, ALIGNS[align], ooffs)
    _guards_hold(got)
    got = _inner(got)
    assert victims and all(ref["flags"][g] & CAPACITY for g in victims)
    assert np.array_equal(got["flags"].view(np.uint32), ref["flags"])
    assert np.array_equal(got["flags"].view(np.uint32) & ~np.uint32(CAPACITY), r["ref"]["flags"])
    assert np.array_equal(got["count"], r["ref"]["count"])
    wr = ref["written"]
    assert wr.any() and (~wr).any()
    for k in STATS:
        assert (got[k][~wr] == SENTINEL).all(), k
    _same_slots(got, ref, wr)


def test_objects_without_pods_are_all_empty(gpu):
    import torch

    ctx, dev = gpu
    S = 70
    world = dict(ctx=ctx, dev=dev, S=S, d_groups=torch.zeros(S + 1, dtype=torch.int64, device=dev),
                 series=ctx.series(torch.empty(0, dtype=torch.float64, device=dev),
                                   torch.zeros(1, dtype=torch.int64, device=dev)))
    got = _launch(world, END, np.zeros(S + 1, dtype=np.int64))
    _guards_hold(got)
    got = _inner(got)
    assert (got["flags"] == EMPTY).all() and (got["count"] == 0).all() and got["sum"].size == 0


def test_argument_errors_and_no_objects(gpu):
    import ctypes

    import torch

    from krr_amd import _native

    ctx, dev = gpu
    world = _world(gpu, "compact")
    lib = _native.load_library()
    assert (_native.KRR_OVERLAY_START, _native.KRR_OVERLAY_END) == (START, END)
    assert lib.krr_abi_version() == 3
    series, S = world["series"], world["S"]
    sp, grp = ctypes.byref(series), world["d_groups"].data_ptr()
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    oo = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    outs = (None,) * 4
    call = lib.krr_pods_overlay
    bad = _native.KRR_E_INVALID
    assert call(None, sp, grp, S, 1, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == bad
    assert call(ctx._h, None, grp, S, 1, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == bad
    assert call(ctx._h, sp, None, S, 1, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == bad
    assert call(ctx._h, sp, grp, S, 1, None, *outs, cnt.data_ptr(), flg.data_ptr(), None) == bad
    assert call(ctx._h, sp, grp, S, 1, oo.data_ptr(), *outs, None, flg.data_ptr(), None) == bad
    assert call(ctx._h, sp, grp, S, 1, oo.data_ptr(), *outs, cnt.data_ptr(), None, None) == bad
    for a in (-1, 2, 7):
        assert call(ctx._h, sp, grp, S, a, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == bad
    with pytest.raises(_native.NativeError):
        ctx.pods_overlay(series, world["d_groups"], S, 5, oo, None, None, None, None, cnt, flg)
    # no objects: nothing is launched, whatever else is passed
    assert call(ctx._h, sp, grp, 0, 1, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == 0
    assert call(None, None, None, 0, 9, None, *outs, None, None, None) == 0
    torch.cuda.synchronize()
    assert (cnt == SENTINEL).all() and (flg == SENTINEL).all()  # none of these calls launched
    # zero-width spans: every object with slots gets CAPACITY, count and the other flags as in a full launch
    assert call(ctx._h, sp, grp, S, 1, oo.data_ptr(), *outs, cnt.data_ptr(), flg.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), world["kstats"]["count"])
    lens, groups = np.diff(world["pod_offs"]), world["groups"]
    Lg = np.array([lens[groups[g]:groups[g + 1]].max(initial=0) for g in range(S)])
    want = world["kstats"]["flags"].view(np.uint32) | np.where(Lg > 0, np.uint32(CAPACITY), np.uint32(0))
    assert np.array_equal(flg.cpu().numpy().view(np.uint32), want)

"""krr_segmented_whist (k_whist) and krr_whist_query (k_whist_query) on the MI355X against the
plain restatement (tests/_whist_ref.py), through the raw ABI.

The series is the edge-geometry lattice (tests/_lattice.py): every length from 0 to 7 chunks at an
even and at an odd start offset, compact and NaN-gapped, fillers of +-1e300 between the cases.  The
bins are m = 3, e_lo = -2, octaves = 4 (36 words), so that normal(0, 1) contents reach the negative
bin, the zero bin, (0, 1/4) and the top bin as well as the 32 log-linear ones.  Everything is
compared for EQUALITY: rows, total weight, the bits of wmin / wmax, count and flags.  The only
inequality is the one derived from the bins' edge ratio: upper <= value * (1 + 2^-m)."""
import ctypes

import numpy as np
import pytest

import _lattice
from _whist_ref import (EMPTY, NAN, QNAN, SKETCH_RANGE, bins_of, bits, bracket, lower_edge, np_whist, pow2,
                        slot_weights, width_of)
from _wquantile_ref import fraction_of
from krr_amd.api import HistogramBins  # noqa: F401  (the feature: absent, nothing here runs)

pytestmark = pytest.mark.gpu

GEOM = (3, -2, 4)
WIDTH = width_of(*GEOM)
TOP = WIDTH - 1
GUARD = 8
SENTINEL = -777
PERCENTILES = ("50", "95", "99.9", "100")
QUERY_TABLES = ("unit", "decay", "short")


def _tables():
    from krr_amd.api import decay_weights, window_weights

    return {"unit": np.array([1], np.uint64), "decay": decay_weights(6, 130), "window": window_weights(7, 200),
            "short": np.array([0, 9, 2], np.uint64), "big": np.array([2 ** 32], np.uint64)}


def _params():
    from krr_amd import _native

    return _native.KrrSketchParams(*GEOM, 0)


def _dev_table(table, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64)).to(dev)


def _build(ctx, series, table, S, dev, base=None, want=("wsum", "wmin", "wmax")):
    """One krr_segmented_whist launch into guarded buffers: {name: whole buffer incl. guards}."""
    import torch

    dt = {"hist": torch.int64, "wsum": torch.int64, "wmin": torch.float64, "wmax": torch.float64,
          "count": torch.int64, "flags": torch.int32}
    bufs = {k: torch.full((S + 2 * GUARD, WIDTH) if k == "hist" else (S + 2 * GUARD,), SENTINEL, dtype=t, device=dev)
            for k, t in dt.items()}
    arg = {k: (v[GUARD:GUARD + S] if k in want or k in ("hist", "count", "flags") else None) for k, v in bufs.items()}
    d_base = None if base is None else torch.from_numpy(np.ascontiguousarray(base, dtype=np.int64)).to(dev)
    ctx.segmented_whist(series, _params(), _dev_table(table, dev), d_base, arg["hist"], arg["wsum"], arg["wmin"],
                        arg["wmax"], arg["count"], arg["flags"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _inner(bufs):
    S = bufs["count"].size - 2 * GUARD
    out = {k: v[GUARD:GUARD + S] for k, v in bufs.items()}
    out["hist"], out["wsum"] = out["hist"].view(np.uint64), out["wsum"].view(np.uint64)
    out["wmin"], out["wmax"] = out["wmin"].view(np.uint64), out["wmax"].view(np.uint64)
    return out


def _guards_intact(bufs):
    return all((v[:GUARD] == SENTINEL).all() and (v[-GUARD:] == SENTINEL).all() for v in bufs.values())


def _query(ctx, got, ps, dev):
    """One krr_whist_query launch of len(ps) percentiles over a build's rows: host arrays [P, S]."""
    import torch

    S = got["count"].size
    hist = torch.from_numpy(got["hist"].view(np.int64).copy()).to(dev)
    mn, mx = (torch.from_numpy(got[k].view(np.float64).copy()).to(dev) for k in ("wmin", "wmax"))
    out = {"bin": torch.full((len(ps), S), SENTINEL, dtype=torch.int32, device=dev),
           "lower": torch.full((len(ps), S), SENTINEL, dtype=torch.float64, device=dev),
           "upper": torch.full((len(ps), S), SENTINEL, dtype=torch.float64, device=dev),
           "flags": torch.full((len(ps), S), SENTINEL, dtype=torch.int32, device=dev)}
    ctx.whist_query(hist, mn, mx, _params(), [fraction_of(p) for p in ps], out["bin"], out["lower"], out["upper"],
                    out["flags"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


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
    vals, offs, index = _lattice.build(gaps, seed=71 if gaps else 72)
    S = offs.size - 1
    series = ctx.series(torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev), int(np.diff(offs).max()), gaps)
    tables = _tables()
    full = {t: _build(ctx, series, tab, S, dev) for t, tab in tables.items()}
    ks = {"count": torch.empty(S, dtype=torch.int64, device=dev), "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_stats(series, None, None, None, ks["count"], ks["flags"])
    torch.cuda.synchronize()
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, index=index, S=S, series=series, tables=tables,
                full=full, got={t: _inner(b) for t, b in full.items()},
                ref={t: np_whist(vals, offs, tab, GEOM, gaps) for t, tab in tables.items()},  # once, shared
                kstats={k: v.cpu().numpy() for k, v in ks.items()})


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    if request.param not in _WORLDS:
        _WORLDS[request.param] = _build_world(gpu, request.param == "gapped")
    yield _WORLDS[request.param]


def test_rows_sums_extremes_count_and_flags_equal_the_restatement(world):
    names = _lattice.names(world["offs"], world["index"])
    for t, got in world["got"].items():
        ref = world["ref"][t]
        for k in ("hist", "wsum", "wmin", "wmax", "count"):
            bad = np.flatnonzero((got[k] != ref[k]).reshape(world["S"], -1).any(axis=1))
            assert bad.size == 0, (t, k, [names[s] for s in bad[:8]])
        assert np.array_equal(got["flags"].view(np.uint32), ref["flags"].view(np.uint32)), t
        assert np.array_equal(got["count"], world["kstats"]["count"]), t
        assert np.array_equal(got["flags"].view(np.uint32), world["kstats"]["flags"].view(np.uint32)), t
        assert _guards_intact(world["full"][t]), t
    unit = world["ref"]["unit"]
    flagged = EMPTY if world["gaps"] else NAN  # the absent* / nan* contents are there, and are rows of zeros
    assert (unit["flags"] == flagged).sum() >= 6 and not unit["hist"][unit["flags"] != 0].any()
    assert (world["got"]["unit"]["wmin"][unit["flags"] != 0] == QNAN).all()
    seen = unit["hist"].sum(axis=0)
    assert (seen > 0).all()  # every word of the row is exercised, the four lumped ones included


def test_unit_table_equals_sketch_build(world):
    """Word for word on every row krr_segmented_whist fills: a KRR_FLAG_NAN row is zeros by its own
    rule (the restatement above), where krr_sketch_build still counts the other samples."""
    import torch

    ctx, dev, S = world["ctx"], world["dev"], world["S"]
    counts = torch.zeros((S, WIDTH), dtype=torch.int32, device=dev)
    vmin, vmax = torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)
    flags = torch.empty(S, dtype=torch.int32, device=dev)
    ctx.sketch_build(world["series"], _params(), counts, vmin, vmax, flags)
    torch.cuda.synchronize()
    got = world["got"]["unit"]
    rows = got["flags"] & NAN == 0
    assert (~rows).sum() == (world["ref"]["unit"]["flags"] == NAN).sum() == (0 if world["gaps"] else (~rows).sum())
    assert rows.sum() > S // 2
    assert np.array_equal(got["hist"][rows], counts.cpu().numpy().view(np.uint32).astype(np.uint64)[rows])
    assert np.array_equal(got["wsum"][rows], got["count"][rows].astype(np.uint64))


def test_the_largest_weight_needs_64_bits(world):
    n = 7 * 1024 + 1
    for parity in (0, 1):
        s = world["index"][("distinct", n, parity)]
        got = world["got"]["big"]
        present = int(got["count"][s])
        assert present == (n if not world["gaps"] else present) and present > 5000
        assert int(got["wsum"][s]) == present << 32 == int(got["hist"][s].sum(dtype=np.uint64))


def test_age_base_past_the_table_takes_the_last_entry(world):
    bufs = _build(world["ctx"], world["series"], world["tables"]["short"], world["S"], world["dev"],
                  base=np.full(world["S"], 10 ** 6, np.int64))
    got, unit = _inner(bufs), world["got"]["unit"]
    assert np.array_equal(got["hist"], 2 * unit["hist"]) and np.array_equal(got["wsum"], 2 * unit["wsum"])
    assert _guards_intact(bufs)
    neg = _inner(_build(world["ctx"], world["series"], world["tables"]["decay"], world["S"], world["dev"],
                        base=np.full(world["S"], -5, np.int64)))  # documented: a negative base is 0
    for k in ("hist", "wsum", "wmin", "wmax"):
        assert np.array_equal(neg[k], world["got"]["decay"][k]), k


def test_slices_add_up_to_the_whole(world):
    """Every case of at least 3 slots cut at slot 1, at L // 2 and at L - 1: the older part, built
    with age_base = the slots after it, plus the newer part is the whole, in every word.  A case
    with a NaN SAMPLE (compact layout) is left out: its whole is a row of zeros by the NaN rule,
    which its NaN-free part does not share."""
    import torch

    ctx, dev, vals, offs = world["ctx"], world["dev"], world["vals"], world["offs"]
    whole_flags = world["got"]["unit"]["flags"]
    old, new, base, of = [], [], [], []
    for key, s in world["index"].items():
        L = int(offs[s + 1] - offs[s])
        if L < 3 or whole_flags[s] & NAN:
            continue
        x = vals[offs[s]:offs[s + 1]]
        for k in (1, L // 2, L - 1):
            old.append(x[:k])
            new.append(x[k:])
            base.append(L - k)
            of.append(s)
    assert len(of) > 3 * 200
    of = np.array(of)
    parts = {}
    for name, segs in (("old", old), ("new", new)):
        o = np.concatenate([[0], np.cumsum([x.size for x in segs])]).astype(np.int64)
        series = ctx.series(torch.from_numpy(np.concatenate(segs)).to(dev), torch.from_numpy(o).to(dev),
                            int(np.diff(o).max()), world["gaps"])
        parts[name] = {t: _inner(_build(ctx, series, tab, len(segs), dev, base=base if name == "old" else None))
                       for t, tab in world["tables"].items()}
    for t in world["tables"]:
        a, b, w = parts["old"][t], parts["new"][t], world["got"][t]
        assert np.array_equal(a["hist"] + b["hist"], w["hist"][of]), t
        assert np.array_equal(a["wsum"] + b["wsum"], w["wsum"][of]), t
        assert np.array_equal(a["count"] + b["count"], w["count"][of]), t


def test_samples_on_the_bin_edges(gpu):
    """One series holding every edge of the bins, the float one ulp below each, +-0, a subnormal,
    -1e300 and +Inf, under a table with a distinct weight per age: every word is known in advance
    from the edges alone (an edge opens its bin, the float below it closes the one before)."""
    import torch

    ctx, dev = gpu
    m, e_lo, octaves = GEOM
    nb = octaves << m
    edges = np.array([float(lower_edge(m, e_lo, i)) for i in range(nb + 1)])
    assert edges[0] == 0.25 and edges[-1] == 4.0 and all(pow2(e_lo + k) == edges[k << m] for k in range(octaves + 1))
    below = np.nextafter(edges, 0.0)
    x = np.concatenate([edges, below, [0.0, -0.0, 5e-324, -1e300, np.inf]])
    where = np.concatenate([3 + np.arange(nb + 1), 2 + np.arange(nb + 1), [1, 1, 2, 0, TOP]])
    rng = np.random.default_rng(3)
    order = rng.permutation(x.size)
    x, where = x[order], where[order]
    table = (1000 + 7 * np.arange(x.size)).astype(np.uint64)
    want = np.zeros(WIDTH, np.uint64)
    np.add.at(want, where, slot_weights(x.size, table))
    for lead in (0, 1):  # an even and an odd start offset
        vals = np.concatenate([np.full(lead, 7.0), x])
        offs = np.array([0, lead, lead + x.size], np.int64)
        series = ctx.series(torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev), x.size, False)
        got = _inner(_build(ctx, series, table, 2, dev))
        assert np.array_equal(got["hist"][1], want), np.flatnonzero(got["hist"][1] != want)
        assert int(got["wsum"][1]) == int(table.sum()) and got["count"][1] == x.size and got["flags"][1] == 0
        assert int(got["wmin"][1]) == bits(-1e300) and int(got["wmax"][1]) == bits(np.inf)
        assert np.array_equal(bins_of(x, GEOM), where)  # the restatement agrees with the edges too


@pytest.fixture(scope="module")
def answers(world):
    """Per table of QUERY_TABLES: one query launch of the four percentiles, and the exact weighted
    percentile of each from krr_segmented_wquantile on the same series."""
    import torch

    ctx, dev, S = world["ctx"], world["dev"], world["S"]
    out = {}
    for t in QUERY_TABLES:
        q = _query(ctx, world["got"][t], PERCENTILES, dev)
        exact = np.empty((len(PERCENTILES), S))
        for j, p in enumerate(PERCENTILES):
            v = torch.empty(S, dtype=torch.float64, device=dev)
            c, f = torch.empty(S, dtype=torch.int64, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
            ctx.segmented_wquantile(world["series"], _dev_table(world["tables"][t], dev), *fraction_of(p), v, None,
                                    None, c, f)
            torch.cuda.synchronize()
            exact[j] = v.cpu().numpy()
        out[t] = (q, exact)
    return out


def test_query_bin_holds_the_exact_weighted_percentile(world, answers):
    m = GEOM[0]
    checked = lumped = 0
    for t, (q, exact) in answers.items():
        got = world["got"][t]
        has = got["wsum"] > 0
        assert has.sum() > world["S"] // 2
        for j, p in enumerate(PERCENTILES):
            v = exact[j][has]
            assert not np.isnan(v).any()
            b = q["bin"][j][has]
            assert np.array_equal(b, bins_of(v, GEOM)), (t, p)
            assert np.array_equal(b, HistogramBins(*GEOM).bin_of(v)), (t, p)
            lo, hi = q["lower"][j][has], q["upper"][j][has]
            assert (lo <= v).all() and (v <= hi).all(), (t, p)
            inner = (b >= 3) & (b < TOP) & (v > 0)
            assert (hi[inner] <= v[inner] * (1 + 2.0 ** -m)).all(), (t, p)  # the edge ratio, exact in float64
            lump = (b == 0) | (b == 2) | (b == TOP)
            assert np.array_equal(q["flags"][j][has], np.where(lump, SKETCH_RANGE, 0)), (t, p)
            checked += int(inner.sum())
            lumped += int(lump.sum())
            # no weight: bin -1, the quiet NaN twice, KRR_FLAG_EMPTY
            assert (q["bin"][j][~has] == -1).all() and (q["flags"][j][~has] == EMPTY).all()
            assert (q["lower"][j][~has].view(np.uint64) == QNAN).all()
            assert (q["upper"][j][~has].view(np.uint64) == QNAN).all()
        # p = 100 gives wmax itself: its bits, but for the zero bin, whose answer is +0.0 whichever zero wmax is
        top = PERCENTILES.index("100")
        up, zero = q["upper"][top][has].view(np.uint64), q["bin"][top][has] == 1
        assert np.array_equal(up[~zero], got["wmax"][has][~zero]) and (~zero).sum() > world["S"] // 2
        assert (up[zero] == 0).all() and (got["wmax"][has][zero] << np.uint64(1) == 0).all()
    assert checked > 1000 and lumped > 200


def test_query_equals_the_restatement_bit_for_bit(world, answers):
    for t, (q, _) in answers.items():
        got = world["got"][t]
        for j, p in enumerate(PERCENTILES):
            num, den = fraction_of(p)
            for s in range(world["S"]):
                want = bracket(got["hist"][s], int(got["wmin"][s]), int(got["wmax"][s]), GEOM, num, den)
                have = (int(q["bin"][j][s]), int(q["lower"][j][s:s + 1].view(np.uint64)[0]),
                        int(q["upper"][j][s:s + 1].view(np.uint64)[0]), int(q["flags"][j][s]))
                assert have == want, (t, p, s)


def test_one_percentile_alone_gives_the_same_bits(world, answers):
    q4 = answers["decay"][0]
    for j, p in enumerate(PERCENTILES):
        q1 = _query(world["ctx"], world["got"]["decay"], (p,), world["dev"])
        for k in q1:
            assert np.array_equal(q1[k][0].view(np.uint8), q4[k][j].view(np.uint8)), (p, k)


@pytest.mark.parametrize("want", [("wsum",), ("wmin", "wmax"), ()], ids=["wsum_only", "extremes_only", "neither"])
def test_null_outputs(world, want):
    part = _build(world["ctx"], world["series"], world["tables"]["decay"], world["S"], world["dev"], want=want)
    for k, v in world["full"]["decay"].items():
        if k in want or k in ("hist", "count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), v.view(np.uint8)), k  # and a second launch repeats the bits
        else:
            assert (part[k] == SENTINEL).all(), k


def test_argument_errors(gpu, world):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    build, query = lib.krr_segmented_whist, lib.krr_whist_query
    E, U = _native.KRR_E_INVALID, _native.KRR_E_UNSUPPORTED
    series, S = world["series"], world["S"]
    hist = torch.full((S, WIDTH), SENTINEL, dtype=torch.int64, device=dev)
    cnt = torch.full((S,), SENTINEL, dtype=torch.int64, device=dev)
    flg = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    tab = torch.ones(4, dtype=torch.int64, device=dev)
    ok, wide, bad = _params(), _native.KrrSketchParams(10, 0, 4, 0), _native.KrrSketchParams(11, 0, 4, 0)
    sp, bp, t = ctypes.byref(series), ctypes.byref(ok), tab.data_ptr()
    h, c, f = hist.data_ptr(), cnt.data_ptr(), flg.data_ptr()
    assert build(None, sp, bp, t, 4, None, h, None, None, None, c, f, None) == E
    assert build(ctx._h, None, bp, t, 4, None, h, None, None, None, c, f, None) == E
    assert build(ctx._h, sp, None, t, 4, None, h, None, None, None, c, f, None) == E             # null bins
    assert build(ctx._h, sp, ctypes.byref(bad), t, 4, None, h, None, None, None, c, f, None) == E  # invalid bins
    assert build(ctx._h, sp, ctypes.byref(wide), t, 4, None, h, None, None, None, c, f, None) == U  # 4100 words
    assert build(ctx._h, sp, bp, None, 4, None, h, None, None, None, c, f, None) == E            # null age_weights
    for n in (0, -1):
        assert build(ctx._h, sp, bp, t, n, None, h, None, None, None, c, f, None) == E           # n_weights < 1
    assert build(ctx._h, sp, bp, t, 4, None, None, None, None, None, c, f, None) == E            # required outputs
    assert build(ctx._h, sp, bp, t, 4, None, h, None, None, None, None, f, None) == E
    assert build(ctx._h, sp, bp, t, 4, None, h, None, None, None, c, None, None) == E

    mn = torch.zeros(S, dtype=torch.float64, device=dev)
    ob = torch.full((4, S), SENTINEL, dtype=torch.int32, device=dev)
    ol = torch.full((4, S), SENTINEL, dtype=torch.float64, device=dev)
    ou = torch.full((4, S), SENTINEL, dtype=torch.float64, device=dev)
    of = torch.full((4, S), SENTINEL, dtype=torch.int32, device=dev)
    rows = torch.zeros((S, WIDTH), dtype=torch.int64, device=dev)
    i64x = ctypes.c_int64 * 5
    outs = (ob.data_ptr(), ol.data_ptr(), ou.data_ptr(), of.data_ptr())

    def q(ctx_h=ctx._h, n=S, bins=bp, r=rows.data_ptr(), a=mn.data_ptr(), b=mn.data_ptr(), num=(50,), den=(1,),
          P=None, outs=outs):
        nums = i64x(*num) if num is not None else None
        dens = i64x(*den) if den is not None else None
        return query(ctx_h, n, bins, r, a, b, nums, dens, len(num) if P is None else P, *outs, None)

    assert q(ctx_h=None) == E and q(bins=None) == E and q(bins=ctypes.byref(bad)) == E
    assert q(bins=ctypes.byref(wide)) == U
    assert q(n=-1) == E and q(P=0) == E and q(num=(50,) * 5, den=(1,) * 5) == E
    assert q(num=None, P=1) == E and q(den=None, P=1) == E
    for num, den in ((0, 1), (-5, 1), (50, 0), (50, -1), (101, 1), (100 * 7 + 1, 7), (1, 10 ** 15 + 1)):
        assert q(num=(50, num), den=(1, den)) == E, (num, den)
    assert q(r=None) == E and q(a=None) == E and q(b=None) == E
    for k in range(4):
        assert q(outs=tuple(None if i == k else o for i, o in enumerate(outs))) == E
    torch.cuda.synchronize()
    for tns in (hist, cnt, flg, ob, ol, ou, of):
        assert (tns == SENTINEL).all()  # nothing launched
    with pytest.raises(_native.NativeError):
        ctx.whist_query(rows, mn, mn, ok, [(101, 1)], ob, ol, ou, of)
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert build(ctx._h, ctypes.byref(empty), None, None, 0, *(None,) * 8) == 0  # nothing to do
    assert q(n=0, r=None, a=None, b=None, outs=(None,) * 4) == 0
    # the bounds themselves are accepted: p = 100, p_den = 10^15, four percentiles, 4096 words
    assert q(num=(100, 1, 50, 99), den=(1, 10 ** 15, 1, 1)) == 0
    torch.cuda.synchronize()
    assert _native.Context.sketch_width(ctx, _native.KrrSketchParams(10, 0, 3, 0)) == 3076

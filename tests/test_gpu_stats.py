"""krr_segmented_stats (k_stats) on the MI355X against restatements written here.

One series per layout (compact, NaN-gapped) holds every case; each case appears once at an even
and once at an odd start offset (the streaming skeleton reads an unaligned first or last sample
with the last chunk).  The kernel runs once per layout (module fixture); the tests compare:

  max, count, flags   bits == krr_segmented_max on the same tensors, and == oracle.seg_max;
  min                 bits == -oracle.seg_max(-x): negation maps the first minimal element, zero
                      sign included, onto the first maximal one (flagged segments: the quiet NaN);
  sum                 integer-valued data below 2^53: == math.fsum (any order is exact);
                      any finite data: |sum - fsum(x)| <= n * 2^-53 * fsum(|x|).

The sum bound is not measured, it is the standard one: n - 1 float64 additions in ANY order err by
at most (n - 1) u sum|x| with u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms,
§4.2, gamma_{n-1}; without the higher-order term: Rump 2012), and fsum's own correctly rounded
result is within u |sum x| <= u sum|x| of the exact sum: together n u sum|x|.  The test first
holds np.sum and a left-to-right Python loop to the same bound on every case.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY, NAN = 4, 1
QNAN = np.uint64(0x7FF8000000000000)
LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17]  # the chunk is 1,024 slots
GUARD = 8


def _cases():
    """name -> float64 samples."""
    rng = np.random.default_rng(11)
    mem = lambda n: np.floor(rng.normal(2e8, 2e7, n))  # noqa: E731  integer-valued: exact sums
    cpu = lambda n: rng.gamma(2.0, 0.05, n) * rng.choice([1.0, 1.0, -1.0], n)  # noqa: E731
    cases = {f"len{n}": mem(n) for n in LENGTHS}
    for i, n in enumerate(rng.integers(0, 5001, 200).tolist()):  # ragged: exact and general data alternate
        cases[f"rand{i}"] = mem(n) if i % 2 == 0 else cpu(n)
    far = 1.0 + rng.random(2000)
    for name, sign, first, second in (("min_negzero_first", 1.0, -0.0, 0.0), ("min_poszero_first", 1.0, 0.0, -0.0),
                                      ("max_negzero_first", -1.0, -0.0, 0.0), ("max_poszero_first", -1.0, 0.0, -0.0)):
        t = np.array([3.0, first, 5.0, second, 1.0]) * np.array([sign, 1, sign, 1, sign])
        cases[name] = t
        t = sign * far.copy()  # the two zeros in different chunks and lanes
        t[[70, 1500]] = first, second
        cases[name + "_far"] = t
    cases["pos_inf"] = np.array([1.0, np.inf, 2.0])
    cases["neg_inf"] = np.array([1.0, -np.inf, 2.0] + [0.5] * 100)
    cases["both_inf"] = np.concatenate([cpu(300), [np.inf], cpu(900), [-np.inf], cpu(10)])
    cases["overflow"] = np.array([1e308, 1e308])
    cases["overflow_neg"] = np.concatenate([[-1e308] * 3, cpu(70)])
    cases["subnormal"] = np.array([5e-324, 1e-310, -5e-324, 2.5e-320] * 40)
    cases["negative"] = -1.0 - rng.random(1500)
    cases["constant"] = np.full(777, 2.5)
    cases["one_negzero"] = np.array([-0.0])
    return cases


def _layout(cases, gaps, seed):
    """Every case at an even and at an odd start offset (one-sample filler segments shift the
    parity).  gaps: a fifth of the slots of every case become NaN (absent), plus all-gap segments;
    compact: NaN samples in segments of their own.  Returns values, offsets, {(name, parity): s}."""
    rng = np.random.default_rng(seed)
    cases = dict(cases)
    if gaps:
        for name, x in list(cases.items()):
            x = x.copy()
            keep = [i for i in range(x.size) if x[i] == 0 or abs(x[i]) > 1e307]  # zeros, infinities, 1e308 stay
            holes = rng.random(x.size) < 0.2
            holes[keep] = False
            x[holes] = np.nan
            cases[name] = x
        for n in (1, 64, 1025):
            cases[f"all_gap{n}"] = np.full(n, np.nan)
    else:
        for n, at in ((1, 0), (2, 1), (65, 64), (1500, 3), (2049, 2048)):
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
    return np.concatenate(segs), offs, index


def _launch(ctx, series, S, dev, want=("min", "max", "sum"), fill=None):
    """One launch into guarded buffers; returns {name: whole buffer incl. guards} (host)."""
    import torch

    bufs = {}
    for k, dt, sentinel in (("min", torch.float64, -777.25), ("max", torch.float64, -777.25),
                            ("sum", torch.float64, -777.25), ("count", torch.int64, -777),
                            ("flags", torch.int32, -777)):
        bufs[k] = torch.full((S + 2 * GUARD,), sentinel, dtype=dt, device=dev)
    arg = {k: (bufs[k][GUARD:GUARD + S] if k in want or k in ("count", "flags") else None) for k in bufs}
    ctx.segmented_stats(series, arg["min"], arg["max"], arg["sum"], arg["count"], arg["flags"])
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
    """The layout's series in HBM, the kernel's outputs (one launch) and the references."""
    import torch

    from oracle import oracle

    ctx, dev = gpu
    gaps = request.param == "gapped"
    vals, offs, index = _layout(_cases(), gaps, seed=3 if gaps else 4)
    S = offs.size - 1
    d_vals, d_offs = torch.from_numpy(vals).to(dev), torch.from_numpy(offs).to(dev)
    series = ctx.series(d_vals, d_offs, int(np.diff(offs).max()), gaps)
    full = _launch(ctx, series, S, dev)
    km = {"value": torch.empty(S, dtype=torch.float64, device=dev), "count": torch.empty(S, dtype=torch.int64, device=dev),
          "flags": torch.empty(S, dtype=torch.int32, device=dev)}
    ctx.segmented_max(series, km["value"], km["count"], km["flags"])
    torch.cuda.synchronize()
    present = []
    for s in range(S):
        x = vals[offs[s]:offs[s + 1]]
        present.append(x[~np.isnan(x)] if gaps else x)
    return dict(ctx=ctx, dev=dev, gaps=gaps, vals=vals, offs=offs, index=index, S=S, series=series, full=full,
                got=_inner(full), kmax={k: v.cpu().numpy() for k, v in km.items()},
                omax=oracle.seg_max(vals, offs, gaps), omin=oracle.seg_max(-vals, offs, gaps), present=present)


def test_layout_covers_both_parities(world):
    offs, index = world["offs"], world["index"]
    for (name, parity), s in index.items():
        assert offs[s] % 2 == parity, name
    assert {n for n, _ in index} >= {f"len{n}" for n in LENGTHS} and world["S"] > 2 * 230


def test_max_count_flags_equal_segmented_max(world):
    got, kmax = world["got"], world["kmax"]
    assert np.array_equal(got["max"].view(np.uint64), kmax["value"].view(np.uint64))
    assert np.array_equal(got["count"], kmax["count"])
    assert np.array_equal(got["flags"], kmax["flags"])
    ov, on, of = world["omax"]
    assert np.array_equal(got["max"].view(np.uint64), ov.view(np.uint64))
    assert np.array_equal(got["count"], on)
    assert np.array_equal(got["flags"].view(np.uint32), of.astype(np.uint32))
    want_n = [x.size for x in world["present"]]
    assert np.array_equal(got["count"], want_n)


def test_min_is_the_first_minimal_element(world):
    got = world["got"]
    ov, on, of = world["omin"]
    assert np.array_equal(on, got["count"]) and np.array_equal(of.astype(np.uint32), got["flags"].view(np.uint32))
    want = (-ov).view(np.uint64).copy()
    want[of != 0] = QNAN  # EMPTY / NAN: the quiet NaN itself, not its negation
    assert np.array_equal(got["min"].view(np.uint64), want)
    # the zero cases by hand: the earlier zero's own bits, as Python min() / max() keep it
    index = world["index"]
    for parity in (0, 1):
        for far in ("", "_far"):
            for name, field, bits in (("min_negzero_first", "min", 1 << 63), ("min_poszero_first", "min", 0),
                                      ("max_negzero_first", "max", 1 << 63), ("max_poszero_first", "max", 0)):
                s = index[(name + far, parity)]
                assert int(got[field][s:s + 1].view(np.uint64)[0]) == bits, (name + far, parity)
    for s, x in enumerate(world["present"]):
        if x.size and not np.isnan(x).any():
            assert got["min"][s] == min(x.tolist()) and got["max"][s] == max(x.tolist())


def test_flagged_segments(world):
    got, index, gaps = world["got"], world["index"], world["gaps"]
    q = lambda k, s: int(got[k][s:s + 1].view(np.uint64)[0])  # noqa: E731
    empties = [("len0", p) for p in (0, 1)] + ([(f"all_gap{n}", p) for n in (1, 64, 1025) for p in (0, 1)] if gaps else [])
    for key in empties:
        s = index[key]
        assert got["flags"][s] == EMPTY and got["count"][s] == 0, key
        assert q("min", s) == QNAN and q("max", s) == QNAN and q("sum", s) == 0, key  # sum = +0.0
    if not gaps:
        for n in (1, 2, 65, 1500, 2049):
            for p in (0, 1):
                s = index[(f"nan_sample{n}", p)]
                assert got["flags"][s] == NAN and got["count"][s] == n
                assert q("min", s) == QNAN and q("max", s) == QNAN and q("sum", s) == QNAN
    assert set(np.unique(got["flags"]).tolist()) <= {0, EMPTY, NAN}


def _finite_sum_cases(world):
    with np.errstate(over="ignore"):  # the overflow cases are told apart by their infinite np.sum
        return [(s, x) for s, x in enumerate(world["present"])
                if x.size and np.isfinite(x).all() and np.isfinite(np.sum(x))]


def test_sum_exact_on_integer_valued_data(world):
    got, checked = world["got"], 0
    for s, x in _finite_sum_cases(world):
        if x.size <= 5000 and (x == np.floor(x)).all() and np.abs(x).sum() < 2.0 ** 53:
            assert got["sum"][s] == math.fsum(x.tolist()), s
            checked += 1
    assert checked > 200


def test_sum_within_the_summation_bound(world):
    got, checked = world["got"], 0
    for s, x in _finite_sum_cases(world):
        xs = x.tolist()
        exact, bound = math.fsum(xs), x.size * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
        loop = 0.0
        for v in xs:
            loop += v
        assert abs(float(np.sum(x)) - exact) <= bound and abs(loop - exact) <= bound, s  # the bound itself
        assert abs(got["sum"][s] - exact) <= bound, (s, got["sum"][s], exact, bound)
        if x.size == 1:
            assert got["sum"][s] == xs[0]
        checked += 1
    assert checked > 400


def test_sum_inf_and_nan_by_class(world):
    got, index, checked = world["got"], world["index"], 0
    for s, x in enumerate(world["present"]):
        if x.size == 0 or np.isnan(x).any():
            continue
        with np.errstate(all="ignore"):
            want = float(np.sum(x))
        if np.isfinite(want):
            continue
        g = got["sum"][s]
        assert (np.isnan(g) and np.isnan(want)) or g == want, (s, g, want)
        assert got["flags"][s] == 0  # plain IEEE: no flag
        checked += 1
    assert checked >= 10
    for p in (0, 1):
        assert got["sum"][index[("overflow", p)]] == np.inf and got["sum"][index[("overflow_neg", p)]] == -np.inf
        assert got["sum"][index[("pos_inf", p)]] == np.inf and got["sum"][index[("neg_inf", p)]] == -np.inf
        s = index[("both_inf", p)]
        assert np.isnan(got["sum"][s]) and got["min"][s] == -np.inf and got["max"][s] == np.inf


def test_two_launches_give_equal_bits(world):
    again = _launch(world["ctx"], world["series"], world["S"], world["dev"])
    for k, v in world["full"].items():
        assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("want", [("max", "sum"), ("min", "max"), ("min", "sum"), ()],
                         ids=["no_min", "no_sum", "no_max", "count_flags_only"])
def test_null_outputs(world, want):
    """A NULL output is not written, the others are unchanged, and nothing lands outside the
    given buffers (guard words on both sides of each)."""
    part, full = _launch(world["ctx"], world["series"], world["S"], world["dev"], want=want), world["full"]
    for k in ("min", "max", "sum", "count", "flags"):
        if k in want or k in ("count", "flags"):
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k  # guards included
        else:
            assert (part[k] == -777.25).all(), k
    for k, v in full.items():
        assert (v[:GUARD] == (-777 if v.dtype.kind == "i" else -777.25)).all(), k
        assert (v[-GUARD:] == (-777 if v.dtype.kind == "i" else -777.25)).all(), k


def test_argument_errors(gpu, world):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    lib = _native.load_library()
    assert lib.krr_segmented_stats(None, None, None, None, None, None, None, None) == _native.KRR_E_INVALID
    assert lib.krr_segmented_stats(ctx._h, None, None, None, None, None, None, None) == _native.KRR_E_INVALID
    import ctypes

    series = world["series"]
    cnt = torch.empty(world["S"], dtype=torch.int64, device=dev)
    assert lib.krr_segmented_stats(ctx._h, ctypes.byref(series), None, None, None, cnt.data_ptr(), None,
                                   None) == _native.KRR_E_INVALID  # out_flags is required
    empty = ctx.series(torch.empty(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert lib.krr_segmented_stats(ctx._h, ctypes.byref(empty), None, None, None, None, None, None) == 0  # nothing to do

"""krr_segmented_percentiles / krr_simple_run_multi on the MI355X: several percentiles from one
pass, every value, count and flag bit for bit against oracle.percentile per percentile (and
oracle.seg_max for the memory half), through both entry points.  The shared cases assert
``multi_plan(...).shared == 1`` so none passes by falling back to the per-percentile paths."""
from decimal import Decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ["ref_index", "sorted_lower", "linear"]
BIG = "99.99999999999999999999999999"


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


def params_of(ps, mode):
    from krr_amd.core.engine import percentile_params

    return [percentile_params(Decimal(str(p)), mode) for p in ps]


def oracle_one(x, offs, prm, gaps):
    from oracle import oracle

    max_n = int(np.diff(offs).max()) if offs.size > 1 else 0
    tab = None
    if prm.mode != 2 and prm.rule.needs_table(max_n):
        tab = prm.rule.table(max(max_n, 1))
    return oracle.percentile(x, offs, prm.mode, prm.p_num, prm.p_den, prm.q, gaps, k_table=tab)


def run_both(gpu, x, offs, mem, gaps, plist):
    """[(values [P, S], counts [S], flags [P, S])] from krr_segmented_percentiles and from
    krr_simple_run_multi, plus the latter's memory outputs."""
    import torch

    ctx, dev = gpu
    S, P = offs.size - 1, len(plist)
    Lmax = int(np.diff(offs).max()) if S else 0
    cs = ctx.series(torch.from_numpy(x).to(dev), torch.from_numpy(offs).to(dev), Lmax, gaps)
    ms = ctx.series(torch.from_numpy(mem).to(dev), torch.from_numpy(offs).to(dev), Lmax, gaps)
    v = torch.full((P, S), -1.0, dtype=torch.float64, device=dev)
    n = torch.full((S,), -1, dtype=torch.int64, device=dev)
    f = torch.full((P, S), -1, dtype=torch.int32, device=dev)
    ctx.segmented_percentiles(cs, plist, v, n, f)
    out = {"cpu_value": torch.full((P, S), -1.0, dtype=torch.float64, device=dev),
           "cpu_count": torch.full((S,), -1, dtype=torch.int64, device=dev),
           "cpu_flags": torch.full((P, S), -1, dtype=torch.int32, device=dev),
           "mem_value": torch.full((S,), -1.0, dtype=torch.float64, device=dev),
           "mem_count": torch.full((S,), -1, dtype=torch.int64, device=dev),
           "mem_flags": torch.full((S,), -1, dtype=torch.int32, device=dev)}
    ctx.simple_run_multi(cs, ms, plist, out)
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in out.items()}
    return [(v.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy()),
            (host["cpu_value"], host["cpu_count"], host["cpu_flags"])], host


def check(gpu, x, offs, mem, gaps, plist, shared, tag):
    from krr_amd import _native
    from oracle import oracle

    Lmax = int(np.diff(offs).max())
    assert _native.multi_plan(Lmax, plist).shared == shared, tag
    outs, host = run_both(gpu, x, offs, mem, gaps, plist)
    wants = [oracle_one(x, offs, prm, gaps) for prm in plist]
    for which, (v, n, f) in enumerate(outs):
        for j, (wv, wn, wf) in enumerate(wants):
            same = (v[j].view(np.uint64) == wv.view(np.uint64)) | (np.isnan(v[j]) & np.isnan(wv))
            if plist[j].mode == _native.KRR_PCT_LINEAR:  # the sign of a zero LINEAR result is unspecified
                same |= (v[j] == 0) & (wv == 0)
            bad = np.flatnonzero(~same)
            assert bad.size == 0, (tag, which, j, bad[:5], v[j][bad[:5]], wv[bad[:5]])
            assert np.array_equal(f[j].astype(np.uint32), wf.astype(np.uint32)), (tag, which, j)
            assert np.array_equal(n, wn), (tag, which, j)
    mv, mn, mf = oracle.seg_max(mem, offs, gaps)
    assert np.array_equal(host["mem_value"].view(np.uint64), mv.view(np.uint64)) or \
        np.array_equal(host["mem_value"], mv, equal_nan=True), tag
    assert np.array_equal(host["mem_count"], mn) and np.array_equal(host["mem_flags"].astype(np.uint32),
                                                                   mf.astype(np.uint32)), tag
    return wants


def ragged(rng, hi, last, gaps):
    lens = rng.integers(0, hi, 400)
    lens[:8] = [0, 1, 2, 3, 64, 1024, 1025, last]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = np.round(rng.gamma(2.0, 0.05, int(offs[-1])), 4)
    mem = np.floor(rng.normal(2e8, 2e7, x.size))
    if gaps:
        x[rng.random(x.size) < 0.1] = np.nan
        mem[rng.random(x.size) < 0.1] = np.nan
    return x, offs, mem


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_ragged_sets_share_one_pass(gpu, mode, gaps):
    rng = np.random.default_rng(23)
    x, offs, mem = ragged(rng, 6000, 5999, gaps)
    for ps in ((95, 99), (1, 5), (90, 95, 99, 100), (BIG, 99)):
        wants = check(gpu, x, offs, mem, gaps, params_of(ps, mode), 1, (mode, gaps, ps))
        # the percentiles of a set differ somewhere (else one answer copied P times would pass)
        assert (wants[0][0].view(np.uint64) != wants[-1][0].view(np.uint64)).any()
    # {5, 95}: whole segments sit in the buffer (both sides are needed)
    x, offs, mem = ragged(rng, 1346, 1345, gaps)
    check(gpu, x, offs, mem, gaps, params_of((5, 95), mode), 1, (mode, gaps, "5-95"))


def long_segments(rng, gaps):
    """A dozen long segments whose shapes stress the probe and the shared rank queries."""
    def exch(n):
        return np.round(rng.gamma(2.0, 0.05, n), 4)

    def zeros(n):  # mostly +-0 with both signs: two ranks fall inside the zero run
        z = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        i = rng.random(n)
        z[i < 0.004] = -rng.gamma(2.0, 0.05, int((i < 0.004).sum()))
        z[i > 0.997] = rng.gamma(2.0, 0.05, int((i > 0.997).sum()))
        return z

    def crowded(n):  # many copies of the value at the kept tail's edge
        v = exch(n)
        v[rng.random(n) < 0.05] = np.sort(v)[int(0.97 * n)]
        return v

    def infs(n):
        v = exch(n)
        i = rng.random(n)
        v[i < 0.02] = np.inf
        v[i > 0.99] = -np.inf
        return v

    def one_nan(n):  # a NaN SAMPLE in the compact layout: KRR_FLAG_NAN for every percentile
        v = exch(n)
        v[n // 3] = np.nan
        return v

    segs = [exch(70000), np.sort(exch(70000)), np.sort(exch(70000))[::-1].copy(), np.full(70000, 0.25), zeros(70000),
            crowded(70000), infs(70000), one_nan(70000),
            exch(50400), np.sort(exch(50400)), zeros(50400), crowded(50400),
            np.sort(exch(33024)), np.sort(exch(33024))[::-1].copy(), infs(33024), exch(33024)]
    x = np.concatenate(segs)
    offs = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    mem = np.floor(rng.normal(2e8, 2e7, x.size))
    if gaps:
        x[rng.random(x.size) < 0.1] = np.nan
    return x, offs, mem


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_probe_and_long_segments(gpu, mode, gaps):
    from krr_amd import _native

    rng = np.random.default_rng(29)
    x, offs, mem = long_segments(rng, gaps)
    plist = params_of((97, 99), mode)
    info = _native.multi_plan(70000, plist)
    assert (info.shared, info.tkeep, info.cap_keys, info.bottom) == (1, 2103, 2752, 0)
    wants = check(gpu, x, offs, mem, gaps, plist, 1, (mode, gaps, "long"))
    if not gaps:
        for wv, wn, wf in wants:
            assert wf[7] == _native.KRR_FLAG_NAN and np.isnan(wv[7])
            assert (np.delete(wf, 7) == 0).all()


@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
def test_fallback_set_is_still_exact(gpu, mode):
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 3000, 51)
    lens[17] = 70000
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = np.round(rng.gamma(2.0, 0.05, int(offs[-1])), 4)
    mem = np.floor(rng.normal(2e8, 2e7, x.size))
    check(gpu, x, offs, mem, False, params_of((50, 99), mode), 0, (mode, "fallback"))
    check(gpu, x, offs, mem, False, params_of((50, 99, 66), mode), 0, (mode, "fallback3"))


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_single_percentile_equals_simple_run(gpu, mode, gaps):
    import torch

    ctx, dev = gpu
    rng = np.random.default_rng(37)
    x, offs, mem = ragged(rng, 3000, 2999, gaps)
    S = offs.size - 1
    prm = params_of((99,), mode)[0]
    outs, host = run_both(gpu, x, offs, mem, gaps, [prm])
    cs = ctx.series(torch.from_numpy(x).to(dev), torch.from_numpy(offs).to(dev), 2999, gaps)
    ms = ctx.series(torch.from_numpy(mem).to(dev), torch.from_numpy(offs).to(dev), 2999, gaps)
    one = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
           (("cpu_value", torch.float64), ("cpu_count", torch.int64), ("cpu_flags", torch.int32),
            ("mem_value", torch.float64), ("mem_count", torch.int64), ("mem_flags", torch.int32))}
    ctx.simple_run(cs, ms, prm, one)
    torch.cuda.synchronize()
    for k, t in one.items():
        a, b = host[k].reshape(-1), t.cpu().numpy()
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                              b.view(np.uint64) if b.dtype == np.float64 else b), (mode, gaps, k)
    assert np.array_equal(outs[0][0][0].view(np.uint64), one["cpu_value"].cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_set_rows_equal_single_percentile_bits(gpu, mode, gaps):
    """The set's rows against krr_segmented_percentile per percentile, bit for bit: both paths
    take their value from the same rank query and finish, so even a LINEAR zero keeps its sign."""
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    rng = np.random.default_rng(41)
    x, offs, _ = ragged(rng, 2048, 2047, gaps)
    S = 48  # the eight fixed lengths and 40 random ones
    offs = offs[:S + 1].copy()
    x = x[:offs[-1]].copy()
    # zeros of both signs: the lowest ranks of segment 5, the highest of (negated) segment 7
    x[offs[7]:offs[8]] *= -1.0
    for s, at, run in ((5, 200, 300), (7, 900, 400)):
        x[offs[s] + at:offs[s] + at + run] = np.where(rng.random(run) < 0.5, 0.0, -0.0)
    Lmax = int(np.diff(offs).max())
    assert Lmax == 2047
    cs = ctx.series(torch.from_numpy(x).to(dev), torch.from_numpy(offs).to(dev), Lmax, gaps)
    zero_rows = 0
    for ps in ((95, 99), (1, 5)):
        plist = params_of(ps, mode)
        assert _native.multi_plan(Lmax, plist).shared == 1, (mode, gaps, ps)
        v = torch.full((2, S), -1.0, dtype=torch.float64, device=dev)
        n = torch.full((S,), -1, dtype=torch.int64, device=dev)
        f = torch.full((2, S), -1, dtype=torch.int32, device=dev)
        ctx.segmented_percentiles(cs, plist, v, n, f)
        for j, prm in enumerate(plist):
            v1 = torch.full((S,), -2.0, dtype=torch.float64, device=dev)
            n1 = torch.full((S,), -2, dtype=torch.int64, device=dev)
            f1 = torch.full((S,), -2, dtype=torch.int32, device=dev)
            ctx.segmented_percentile(cs, prm, v1, n1, f1)
            torch.cuda.synchronize()
            a, b = v[j].cpu().numpy(), v1.cpu().numpy()
            same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
            bad = np.flatnonzero(~same)
            assert bad.size == 0, (mode, gaps, ps, j, bad[:5], a[bad[:5]], b[bad[:5]])
            assert np.array_equal(n.cpu().numpy(), n1.cpu().numpy()), (mode, gaps, ps, j)
            assert np.array_equal(f[j].cpu().numpy(), f1.cpu().numpy()), (mode, gaps, ps, j)
            zero_rows += int((b[[5, 7]] == 0).sum())
    if mode != "ref_index":  # (REF_INDEX goes by position, not by rank among the values)
        assert zero_rows >= 4  # the zero runs are where the ranks fall, in both segments


def test_argument_errors(gpu):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    offs = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    vals = torch.arange(30, dtype=torch.float64, device=dev)
    series = ctx.series(vals, offs, 20)
    tab = torch.arange(16, dtype=torch.int64, device=dev)

    def both(plist):
        P = max(len(plist), 1)
        v = torch.empty((P, 2), dtype=torch.float64, device=dev)
        n = torch.empty(2, dtype=torch.int64, device=dev)
        f = torch.empty((P, 2), dtype=torch.int32, device=dev)
        out = {"cpu_value": v, "cpu_count": n, "cpu_flags": f, "mem_value": torch.empty(2, dtype=torch.float64, device=dev),
               "mem_count": torch.empty(2, dtype=torch.int64, device=dev),
               "mem_flags": torch.empty(2, dtype=torch.int32, device=dev)}
        for call in (lambda: ctx.segmented_percentiles(series, plist, v, n, f),
                     lambda: ctx.simple_run_multi(series, series, plist, out)):
            with pytest.raises(_native.NativeError) as e:
                call()
            assert e.value.code == _native.KRR_E_INVALID

    both([])
    both(params_of((90, 95, 97, 99, 100), "linear"))
    both(params_of((95,), "linear") + params_of((99,), "sorted_lower"))
    for mode in (_native.KRR_PCT_REF_INDEX, _native.KRR_PCT_SORTED_LOWER):
        short = _native.KrrPercentileParams(mode, 0, 99, 1, 0.99, tab.data_ptr(), tab.numel())
        both([_native.KrrPercentileParams(mode, 0, 95, 1, 0.95), short])
    torch.cuda.synchronize()

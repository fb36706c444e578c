"""GPU: exact time-sharded percentiles in ONE HBM pass (window export / merge,
include/krr_amd.h; config 5), through the C ABI.

Every series is cut into W time slices handled as W 'ranks' in one process: each slice
is exported (krr_window_export, its own launch, as on its own GPU), the headers and key
rows are stacked slice-major (what the all-to-all delivers to the owner) and merged
(krr_window_merge).  Results are checked bit for bit against the C oracle
(oracle/krr_oracle.c) on the whole series; a miss must be flagged, never wrong, and the
regather fallback (krr_amd.core.sketch.finish_window_misses) makes it exact."""
import os
import sys
import zlib

import numpy as np
import pytest

from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _window_model  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from krr_amd import _native

    c = _native.Context(0)
    yield c
    c.close()


def _dev(a, dt=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dt)).to("cuda:0")


def _same(got, want, mode):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if mode == "linear":  # the zero sign of a LINEAR result is unspecified (numpy's partition)
        ok |= got == want
    return ok


SENT_I = -777  # headers and key rows start as this (tests/_window_model.py: no sample's key)


def _emulate(ctx, x, W, params, gaps, key_cap=None, detail=None):
    """x: [S, L] (NaN = gap when gaps).  Export every slice, merge.  Returns value, count,
    flags, misses, headers (host arrays / int); detail (a dict) also takes the key rows, key_cap
    and the slices' column cuts."""
    import torch

    from krr_amd import _native

    S, L = x.shape
    cuts = np.array_split(np.arange(L), W)
    kc = key_cap or _native.window_key_cap(max(c.size for c in cuts), L - min(c.size for c in cuts), params)
    dev = torch.device("cuda:0")
    hdr = torch.full((W * S, _native.HDR_WORDS), SENT_I, dtype=torch.int64, device=dev)
    keys = torch.full((W * S, kc), SENT_I, dtype=torch.int64, device=dev)
    keep = []
    for j, c in enumerate(cuts):
        xs = _dev(np.ascontiguousarray(x[:, c]).ravel())
        o = _dev((np.arange(S + 1) * c.size).astype(np.int64), np.int64)
        ser = ctx.series(xs, o, c.size, gaps)
        ctx.window_export(ser, params, L - c.size, kc, hdr[j * S:(j + 1) * S], keys[j * S:(j + 1) * S])
        keep.append(ser)
    v = torch.empty(S, dtype=torch.float64, device=dev)
    n = torch.empty(S, dtype=torch.int64, device=dev)
    f = torch.empty(S, dtype=torch.int32, device=dev)
    miss = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.window_merge(S, W, S, hdr, keys, kc, params, v, n, f, miss)
    torch.cuda.synchronize()
    if detail is not None:
        detail.update(keys=keys.cpu().numpy(), key_cap=kc, cuts=cuts)
    return v.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy().astype(np.uint32), int(miss.item()), hdr.cpu().numpy()


def _mixed(rng, S, L):
    """Exchangeable Gamma series plus the adversarial ones (index: role)."""
    x = rng.gamma(2.0, 0.05, size=(S, L))
    x[rng.random(x.shape) < 0.02] = 0.0
    x[0] = np.where(rng.random(L) < 0.5, 0.0, -0.0)       # all zeros, both signs
    x[1] = 0.25                                            # constant: point windows
    x[2] = np.round(rng.gamma(2.0, 0.05, L), 2)            # heavily quantized (crowded keys)
    x[3] = np.linspace(0.0, 1.0, L)                        # trend: slices disagree -> misses allowed
    x[4, ::5] = -x[4, ::5]                                 # negatives
    x[5, rng.random(L) < 0.01] = np.inf
    x[6] = 0.25 + 0.002 * rng.standard_normal(L)           # low dispersion
    return x


TREND = 3


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mode,pct", [("linear", "99"), ("sorted_lower", "99"), ("linear", "50"),
                                      ("sorted_lower", "5"), ("linear", "100"), ("sorted_lower", "0.1")])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_window_emulated_ranks(ctx, gaps, mode, pct, W):
    from decimal import Decimal

    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(zlib.crc32(f"{gaps}{mode}{pct}{W}".encode()))
    S, L = 40, 12_000
    x = _mixed(rng, S, L)
    if gaps:
        x[rng.random(x.shape) < 0.15] = np.nan
        x[7, : L // 2] = np.nan   # empty in the first slices
        x[8] = np.nan             # empty series
    params = percentile_params(Decimal(pct), mode)
    exported = {}
    v, n, f, misses, hdr = _emulate(ctx, x, W, params, gaps, detail=exported)
    # every header and row keeps the promise of krr_window_hdr: exact counts against [lo, hi]
    broken = []
    for j, c in enumerate(exported["cuts"]):
        for i in range(S):
            r = j * S + i
            viol = _window_model.check_header(x[i, c], gaps, hdr[r], exported["keys"][r], exported["key_cap"], SENT_I)
            if viol:
                broken.append((f"series {i} slice {j}", viol, _window_model.unpack_header(hdr[r])))
    assert not broken, broken[:4]
    ov, on, of = oracle.percentile(x.ravel(), (np.arange(S + 1) * L).astype(np.int64), params.mode, params.p_num,
                                   params.p_den, params.q, gaps)
    is_miss = (f & _native.KRR_FLAG_WINDOW_MISS) != 0
    assert misses == int(is_miss.sum())
    ok = _same(v, ov, mode) & (n == on)
    bad = np.nonzero(~ok & ~is_miss)[0]
    detail = [(int(i), v[i], ov[i], int(n[i]), int(on[i]), int(f[i]),
               [(hex(int(hdr[j * S + i, 0]) % 2**64), hex(int(hdr[j * S + i, 1]) % 2**64), int(hdr[j * S + i, 2]),
                 int(hdr[j * S + i, 3]), int(hdr[j * S + i, 4]) & 0xFFFFFFFF, int(hdr[j * S + i, 4]) >> 32)
                for j in range(W)]) for i in bad[:3]]
    assert bad.size == 0, detail
    assert np.array_equal(f[~is_miss], of[~is_miss])
    # misses only where the data give a reason: the trend, a zero SORTED_LOWER result (its
    # sign comes from position), crowded/quantized keys; never on exchangeable Gamma series
    allowed = {0, 2, TREND, 6} | set(np.nonzero(ov == 0)[0].tolist())
    assert set(np.nonzero(is_miss)[0].tolist()) <= allowed, np.nonzero(is_miss)
    if W == 1:
        assert not (is_miss & (ov != 0))[[1, 4, 5]].any()


@pytest.mark.parametrize("mode", ["linear", "sorted_lower"])
def test_window_world1_flow_finishes_misses(ctx, mode):
    """window_exact_time_sharded at world size 1: the merge's misses (here: the all-zero
    series under SORTED_LOWER) are finished by selecting the series whole; every result
    equals the oracle."""
    from decimal import Decimal

    from krr_amd.core import sketch
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(21)
    S, L = 30, 9000
    x = _mixed(rng, S, L)
    x[rng.random(x.shape) < 0.1] = np.nan
    offs = (np.arange(S + 1) * L).astype(np.int64)
    ser = ctx.series(_dev(x.ravel()), _dev(offs, np.int64), 0, True)
    params = percentile_params(Decimal("50"), mode)
    res = sketch.window_exact_time_sharded(ctx, ser, params)
    ov, on, of = oracle.percentile(x.ravel(), offs, params.mode, params.p_num, params.p_den, params.q, True)
    assert _same(res["value"].cpu().numpy(), ov, mode).all()
    assert np.array_equal(res["count"].cpu().numpy(), on)
    assert np.array_equal(res["flags"].cpu().numpy().astype(np.uint32), of)
    if mode == "sorted_lower":
        assert res["misses"] >= 1  # the all-zero series went through the fallback


@pytest.mark.parametrize("mode", ["linear", "sorted_lower"])
def test_window_parts_equal_one_buffer(ctx, mode):
    """The same flow over the series split into parts in buffers of their own (one export
    launch per part, alternating streams — what bench.py --config 5 runs): the misses are
    regathered across parts, and every result equals the oracle."""
    from decimal import Decimal

    from krr_amd.core import sketch
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(23)
    S, L = 31, 9000
    x = _mixed(rng, S, L)
    x[rng.random(x.shape) < 0.1] = np.nan
    offs = (np.arange(S + 1) * L).astype(np.int64)
    cuts = [0, 4, 5, 17, 31]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        o = (np.arange(hi - lo + 1) * L).astype(np.int64)
        v = _dev(x[lo:hi].ravel())
        parts.append((lo, hi, ctx.series(v, _dev(o, np.int64), L, True)))
    params = percentile_params(Decimal("50"), mode)
    res = sketch.window_exact_time_sharded(ctx, parts, params)
    ov, on, of = oracle.percentile(x.ravel(), offs, params.mode, params.p_num, params.p_den, params.q, True)
    assert _same(res["value"].cpu().numpy(), ov, mode).all()
    assert np.array_equal(res["count"].cpu().numpy(), on)
    assert np.array_equal(res["flags"].cpu().numpy().astype(np.uint32), of)
    if mode == "sorted_lower":
        assert res["misses"] >= 1


def test_window_nan_in_compact_layout(ctx):
    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(5)
    x = rng.gamma(2.0, 0.05, size=(4, 3000))
    x[1, 2500] = np.nan  # in the last slice only
    v, n, f, misses, _ = _emulate(ctx, x, 3, percentile_params(99, "linear"), False)
    assert f[1] == _native.KRR_FLAG_NAN and np.isnan(v[1]) and misses == 0
    assert (f[[0, 2, 3]] == 0).all()


def test_window_rows_are_short(ctx):
    """A p99 export of 8 slices of a 172,800-sample series keeps ~2(6 sigma + 4) keys per
    slice (sigma: the global rank's spread among one slice's samples), not the LDS window."""
    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(9)
    S, L, W = 16, 172_800, 8
    x = rng.gamma(2.0, 0.05, size=(S, L))
    params = percentile_params(99, "linear")
    v, n, f, misses, hdr = _emulate(ctx, x, W, params, False)
    kc = _native.window_key_cap(L // W, L - L // W, params)
    cnt = hdr[:, 4] & 0xFFFFFFFF
    assert misses == 0 and (cnt <= kc).all() and kc <= 320, (kc, cnt.max())
    ov, on, _ = oracle.percentile(x.ravel(), (np.arange(S + 1) * L).astype(np.int64), 2, 99, 1, 0.99, False)
    assert _same(v, ov, "linear").all() and np.array_equal(n, on)


def test_window_forced_small_rows_miss_not_wrong(ctx):
    """Rows far too short for the data (key_cap 64 at p50 of 8 slices): exports overflow and
    are flagged, merges miss — and no series gets a wrong value."""
    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    rng = np.random.default_rng(10)
    S, L = 20, 40_000
    x = rng.gamma(2.0, 0.05, size=(S, L))
    params = percentile_params(50, "sorted_lower")
    v, n, f, misses, hdr = _emulate(ctx, x, 8, params, False, key_cap=64)
    is_miss = (f & _native.KRR_FLAG_WINDOW_MISS) != 0
    assert misses == int(is_miss.sum()) and misses > 0
    assert ((hdr[:, 4] >> 32) & _native.KRR_WIN_FAIL).any()
    ov, on, _ = oracle.percentile(x.ravel(), (np.arange(S + 1) * L).astype(np.int64), 1, 50, 1, 0.5, False)
    assert (_same(v, ov, "sorted_lower") | is_miss).all()


def test_window_bad_arguments(ctx):
    import torch

    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    dev = torch.device("cuda:0")
    params = percentile_params(99, "linear")
    x = torch.zeros(100, dtype=torch.float64, device=dev)
    o = torch.tensor([0, 100], dtype=torch.int64, device=dev)
    ser = ctx.series(x, o, 100, False)
    hdr = torch.empty((1, _native.HDR_WORDS), dtype=torch.int64, device=dev)
    keys = torch.empty((1, 4096), dtype=torch.int64, device=dev)
    with pytest.raises(_native.NativeError):
        ctx.window_export(ser, params, 0, 4096, hdr, keys)  # key_cap above the LDS window
    with pytest.raises(_native.NativeError):
        ctx.window_export(ser, percentile_params(99, "ref_index"), 0, 64, hdr, keys)
    v = torch.empty(1, dtype=torch.float64, device=dev)
    n = torch.empty(1, dtype=torch.int64, device=dev)
    f = torch.empty(1, dtype=torch.int32, device=dev)
    with pytest.raises(_native.NativeError):
        ctx.window_merge(1, 65, 1, hdr.repeat(65, 1), keys[:, :64].repeat(65, 1).contiguous(), 64, params, v, n, f)
    assert _native.window_key_cap(21_600, 151_200, params) % 64 == 0

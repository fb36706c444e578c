"""GPU: krr_window_export / krr_window_merge (config 5's exact time-sharded percentile) over the
edge-geometry lattice, held to exact counts (tests/_window_model.py; pinned on the CPU by
tests/test_window_model.py).

Every time slice is a whole lattice (tests/_lattice.py): slice j has seed 31 (compact) or 32
(gapped) + 10 j and its fillers shifted when j is odd, so the slices share segment numbers and
parities and differ in every offset and sample.  _window_model.compose says which segment of
slice j belongs to which series: with rot = 0 a series' slices have one length, with rot = 1 and 5
they have 0, 1 and 2 slots, or less than a chunk next to several chunks.

What is checked is the part the header promises to be exact: n, below, cnt and the row against
[lo, hi] (check_header), and the merge's outcome as a function of the very headers the export
produced (merge_model): a miss exactly where the counts say miss, and on a hit the oracle's value
bit for bit.  How the export chooses its window is free, except for the conditions that do not
depend on that choice; each test states them.

The kernel kind follows the DECLARED max_segment_len: the lattice's true 7,169 slots give
k_window_export<false> (1,088-key window), 50,400 and 172,800 give k_window_export<true>
(LANE_COUNTS, 2,304-key window, depth-2 ring), the latter with the XCD remap off.

Outputs are pre-filled with a sentinel, so an unwritten header, key or result shows.  A failure
names (content, length, parity) with the slice, layout, kind, mode and percentile.  Each test
prints one "window-lattice" line with its counts of FAIL and POINT slices and of missed series.
"""
import collections
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lattice  # noqa: E402
import _window_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"sorted_lower": wm.SORTED_LOWER, "linear": wm.LINEAR}
PCT = {"100": (100, 1), "99": (99, 1), "50": (50, 1), "5": (5, 1), "0.1": (1, 10)}
SENT_V, SENT_I = -777.25, wm.SENTINEL
MAXLEN = 7 * 1024 + 1
KINDS = {"short": 0, "long": 50_400}  # kind -> declared slots (0: the lattice's true maximum)
KEY_CAP_MAX = 2304                    # krr_window_export / krr_window_merge: key_cap <= the long window
LDS_FIXED, LDS_LIMIT = 1536, 160 * 1024  # the merge's LDS is LDS_FIXED + n_slices x key_cap keys; a gfx950 CU has 160 KiB
DISTINCT = {"distinct", "edge_hi", "edge_lo", "absent0", "absentL", "absent0L", "absent_all", "nan0", "nanL",
            "nanmid", "filler"}
ZEROS = {"zeros", "zeros_swap"}


def _params(mode, p):
    from krr_amd import _native

    p_num, p_den = PCT[p]
    return _native.KrrPercentileParams(MODES[mode], 0, p_num, p_den, float(p_num) / float(p_den) / 100.0)


def _key_cap(declared, ext, params):
    from krr_amd import _native

    return min(_native.window_key_cap(declared or MAXLEN, ext, params), KEY_CAP_MAX)


class Slice:
    """One slice lattice in HBM (uploaded once) with each segment's sorted present keys."""

    def __init__(self, ctx, dev, gaps, j):
        import torch

        self.ctx, self.gaps, self.j = ctx, gaps, j
        self.vals, self.offs, self.index = _lattice.build(gaps, (32 if gaps else 31) + 10 * j, shift=j % 2)
        self.d_vals = torch.from_numpy(self.vals).to(dev)
        self.d_offs = torch.from_numpy(self.offs).to(dev)
        self.vals.flags.writeable = self.offs.flags.writeable = False
        self.S = self.offs.size - 1
        self.names = _lattice.names(self.offs, self.index)
        assert int(np.diff(self.offs).max()) == MAXLEN
        self._keys = None

    def seg(self, s):
        return self.vals[self.offs[s]:self.offs[s + 1]]

    @property
    def keys(self):
        if self._keys is None:
            self._keys = [wm.sorted_keys(self.seg(s)) for s in range(self.S)]
        return self._keys

    def series(self, declared):
        return self.ctx.series(self.d_vals, self.d_offs, declared or MAXLEN, self.gaps)


class World:
    """The slice lattices of one layout, the composed series and their oracle results, each made
    once and read-only."""

    def __init__(self, ctx, dev, gaps):
        self.ctx, self.dev, self.gaps = ctx, dev, gaps
        self.layout = "gapped" if gaps else "compact"
        self._slices, self._composed, self._oracle = {}, {}, {}

    def slice(self, j):
        if j not in self._slices:
            self._slices[j] = Slice(self.ctx, self.dev, self.gaps, j)
            assert self._slices[j].index == self.slice(0).index
        return self._slices[j]

    def composed(self, W, rot):
        """perms [W, S] on the host and on the device, the composed values and offsets."""
        import torch

        if (W, rot) not in self._composed:
            lat = [(self.slice(j).vals, self.slice(j).offs, self.slice(j).index) for j in range(W)]
            perms, vals, offs = wm.compose(lat, rot)
            vals.flags.writeable = offs.flags.writeable = perms.flags.writeable = False
            self._composed[(W, rot)] = perms, torch.from_numpy(perms.copy()).to(self.dev), vals, offs
        return self._composed[(W, rot)]

    def oracle(self, W, rot, mode, p):
        key = (W, rot, mode, p)
        if key not in self._oracle:
            _, _, vals, offs = self.composed(W, rot)
            p_num, p_den = PCT[p]
            ref = oracle.percentile(vals, offs, MODES[mode], p_num, p_den, float(p_num) / float(p_den) / 100.0, self.gaps)
            for a in ref:
                a.flags.writeable = False
            self._oracle[key] = ref
        return self._oracle[key]

    def oracle_slice(self, j, mode, p):
        """The oracle over slice lattice j by itself."""
        key = ("slice", j, mode, p)
        if key not in self._oracle:
            sl = self.slice(j)
            p_num, p_den = PCT[p]
            ref = oracle.percentile(sl.vals, sl.offs, MODES[mode], p_num, p_den, float(p_num) / float(p_den) / 100.0, self.gaps)
            for a in ref:
                a.flags.writeable = False
            self._oracle[key] = ref
        return self._oracle[key]

    def full(self, shape, fill, dtype):
        import torch

        return torch.full(shape, fill, dtype=dtype, device=self.dev)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    ctx, dev = gpu
    return World(ctx, dev, request.param == "gapped")


def _assert_kind(kind, declared):
    """The export cannot pass by running the other kernel: the window launches of the two declared
    lengths differ in their LDS (the 1,088-key and the 2,304-key window), and this declared length
    has its kind's.  p50 is a window percentile at every one of these lengths."""
    from krr_amd import _native

    p50 = _params("sorted_lower", "50")
    short, long_ = _native.select_plan(MAXLEN, p50), _native.select_plan(50_400, p50)
    assert short.hselect == 1 and long_.hselect == 1 and long_.lds_bytes > short.lds_bytes
    plan = _native.select_plan(declared or MAXLEN, p50)
    assert plan.hselect == 1 and plan.lds_bytes == (short if kind == "short" else long_).lds_bytes, (kind, declared)


def _export(world, j, declared, params, ext, kc):
    import torch

    sl = world.slice(j)
    hdr = world.full((sl.S, wm.HDR_WORDS), SENT_I, torch.int64)
    keys = world.full((sl.S, kc), SENT_I, torch.int64)
    world.ctx.window_export(sl.series(declared), params, ext, kc, hdr, keys)
    return hdr, keys


def _flags(hdr):
    return (hdr[:, 4].view(np.uint64) >> np.uint64(32)).astype(np.int64)


def _by_content(names, mask):
    return dict(collections.Counter(names[s][0] for s in np.flatnonzero(mask)))


# kind, declared slots, percentile, mode, ext in longest slices, slice lattice
EXPORT_CASES = [(kind, KINDS[kind], p, mode, ext, 0) for kind, p, mode, ext in
                itertools.product(KINDS, PCT, MODES, (0, 2, 63))]
EXPORT_CASES.append(("long_noremap", 172_800, "99", "linear", 2, 0))  # >= 100,000 declared slots: no XCD remap
# slice lattice 1 (the shifted fillers: the same segments at other offsets), at the ext of W = 3
EXPORT_CASES += [(kind, KINDS[kind], p, mode, 2, 1) for kind, p, mode in itertools.product(KINDS, PCT, MODES)]
EXPORT_IDS = [f"{k}-p{p}-{m}-ext{e}" + ("-slice1" if j else "") for k, _, p, m, e, j in EXPORT_CASES]


@pytest.mark.parametrize("case", EXPORT_CASES, ids=EXPORT_IDS)
def test_export_headers(world, case):
    """Every slice's header and row keep the promise of krr_window_hdr (check_header), at ext = 0,
    2 and 63 times the longest slice (slice lattice 0; lattice 1 at ext = 2).  Whatever window the
    export chose:

      * no const slice FAILs at any length: it ends as the whole window or as POINT, in the stream
        (two chunks and more) and in export_shrink (one chunk, more keys than the row holds);
      * in the compact layout KRR_FLAG_NAN is on exactly the slices that hold a NaN sample, in the
        gapped layout on none;
      * no slice of the distinct-valued contents FAILs: export_shrink keeps at most
        2w + 3 <= key_cap - 63 keys, and the in-stream window holds exchangeable normal samples
        at 6 sigma."""
    import torch

    kind, declared, p, mode, ext_slices, j = case
    _assert_kind(kind, declared)
    sl = world.slice(j)
    ext = ext_slices * MAXLEN
    params = _params(mode, p)
    kc = _key_cap(declared, ext, params)
    hdr, keys = _export(world, j, declared, params, ext, kc)
    torch.cuda.synchronize()
    hdr, keys = hdr.cpu().numpy(), keys.cpu().numpy()
    where = f"slice={j} layout={world.layout} kind={kind} mode={mode} p={p} ext={ext} key_cap={kc}"
    bad = []
    for s in range(sl.S):
        v = wm.check_header(sl.seg(s), world.gaps, hdr[s], keys[s], kc, SENT_I, keys=sl.keys[s])
        if v:
            bad.append(f"{sl.names[s]} {where}: {'; '.join(v)} (header {wm.unpack_header(hdr[s])})")
    assert not bad, f"{len(bad)} of {sl.S} slices break the header's promise:\n" + "\n".join(bad[:8])

    flags = _flags(hdr)
    fail, point, nan = (flags & wm.WIN_FAIL) != 0, (flags & wm.WIN_POINT) != 0, (flags & wm.FLAG_NAN) != 0
    length = np.array([n for _, n, _ in sl.names])
    content = np.array([c for c, _, _ in sl.names])
    present = np.array([k.size for k in sl.keys])
    has_nan = np.array([bool(np.isnan(sl.seg(s)).any()) for s in range(sl.S)])
    print(f"window-lattice export {where}: FAIL {_by_content(sl.names, fail)} POINT {int(point.sum())}")

    def named(mask):
        return [sl.names[s] for s in np.flatnonzero(mask)][:8]

    const = content == "const"
    assert not (fail & const).any(), f"{where}: const slices FAIL: {named(fail & const)}"
    stream = const & (length >= 2 * wm.CHUNK) & (present > kc)
    shrunk = const & (length <= wm.CHUNK) & (present > kc)
    assert stream.any() and point[stream].all(), (f"{where}: const slices of two chunks and more (point window in the "
                                                  f"stream) without KRR_WIN_POINT: {named(stream & ~point)}")
    assert point[shrunk].all(), (f"{where}: const slices of one chunk (export_shrink ends on one key) without "
                                 f"KRR_WIN_POINT: {named(shrunk & ~point)}")
    if ext == 0:  # a 128-key row: the const slices of 1,023 and 1,024 slots (a gapped one of 129 may fit it)
        assert kc == 128 and shrunk.sum() >= 4, (where, kc, named(shrunk))
    want_nan = has_nan & (not world.gaps)
    assert np.array_equal(nan, want_nan), f"{where}: KRR_FLAG_NAN on the wrong slices: {named(nan != want_nan)}"
    distinct = np.isin(content, sorted(DISTINCT))
    assert not (fail & distinct).any(), f"{where}: distinct-valued slices FAIL: {named(fail & distinct)}"


@pytest.mark.parametrize("case", EXPORT_CASES, ids=EXPORT_IDS)
def test_export_one_chunk_never_fails(world, case):
    """No slice of at most 1,024 slots has KRR_WIN_FAIL: one chunk fits the empty 1,088-key
    window, and the padding is NaN, so the stream cannot fail; and key_cap holds the ranks
    export_shrink keeps, so a row that copies of repeated keys crowd ends as POINT on the key at
    the slice's own rank (the `ties` slices of 1,023 / 1,024 slots around the -0 / +0 boundary at
    p50), never as a failure.  A test of its own, over the same launches as test_export_headers:
    it reads the headers alone."""
    import torch

    kind, declared, p, mode, ext_slices, j = case
    sl = world.slice(j)
    ext = ext_slices * MAXLEN
    params = _params(mode, p)
    kc = _key_cap(declared, ext, params)
    hdr, _ = _export(world, j, declared, params, ext, kc)
    torch.cuda.synchronize()
    fail = (_flags(hdr.cpu().numpy()) & wm.WIN_FAIL) != 0
    length = np.array([n for _, n, _ in sl.names])
    bad = np.flatnonzero(fail & (length <= wm.CHUNK))
    where = f"slice={j} layout={world.layout} kind={kind} mode={mode} p={p} ext={ext} key_cap={kc}"
    print(f"window-lattice one-chunk {where}: FAIL {_by_content(sl.names, fail & (length <= wm.CHUNK))}")
    assert bad.size == 0, (f"{where}: {bad.size} slices within one chunk FAIL, "
                           f"{_by_content(sl.names, fail & (length <= wm.CHUNK))}: {[sl.names[s] for s in bad[:8]]}")


def _merge(world, W, rot, declared, mode, p):
    """Export slices 0 .. W-1, stack headers and rows slice-major by compose's permutations, merge.
    Returns the host copies: value, count, flags, miss counter, headers [W, S, 5], rows [W, S, kc]."""
    import torch

    params = _params(mode, p)
    ext = (W - 1) * MAXLEN
    kc = _key_cap(declared, ext, params)
    S = world.slice(0).S
    _, d_perms, _, _ = world.composed(W, rot)
    hdrs, rows = [], []
    for j in range(W):
        h, k = _export(world, j, declared, params, ext, kc)
        hdrs.append(h[d_perms[j]])
        rows.append(k[d_perms[j]])
    hdr, keys = torch.cat(hdrs), torch.cat(rows)
    lds = LDS_FIXED + W * kc * 8
    assert lds <= LDS_LIMIT, (W, kc, lds)
    v = world.full((S,), SENT_V, torch.float64)
    n = world.full((S,), SENT_I, torch.int64)
    f = world.full((S,), SENT_I, torch.int32)
    miss = world.full((1,), SENT_I, torch.int32)  # the merge zeroes it first
    world.ctx.window_merge(S, W, S, hdr, keys, kc, params, v, n, f, miss)
    torch.cuda.synchronize()
    return (v.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy().view(np.uint32), int(miss.item()),
            hdr.cpu().numpy().reshape(W, S, wm.HDR_WORDS), keys.cpu().numpy().reshape(W, S, kc), kc)


def _outcome_class(flags):
    if flags == wm.FLAG_WINDOW_MISS:
        return "miss"
    return {0: "hit", wm.FLAG_NAN: "nan", wm.FLAG_EMPTY: "empty"}.get(int(flags), f"flags {flags}")


def _check_merge(world, W, rot, kind, declared, mode, p):
    gv, gn, gf, misses, hdr, keys, kc = _merge(world, W, rot, declared, mode, p)
    ov, on, of = world.oracle(W, rot, mode, p)
    names = world.slice(0).names
    p_num, p_den = PCT[p]
    q = float(p_num) / float(p_den) / 100.0
    where = f"W={W} rot={rot} layout={world.layout} kind={kind} mode={mode} p={p} key_cap={kc}"
    bad, missed, reasons = [], np.zeros(len(names), dtype=bool), collections.Counter()
    for i, name in enumerate(names):
        what, _, _, _ = wm.merge_model(hdr[:, i], keys[:, i], MODES[mode], p_num, p_den, q)
        got = _outcome_class(gf[i])
        if got != what.split(":")[0]:
            bad.append(f"{name} {where}: the kernel says {got} (value {gv[i]!r}), the model over its headers {what}: "
                       f"{[wm.unpack_header(h) for h in hdr[:, i]][:4]}")
            continue
        if got == "miss":
            missed[i] = True
            reasons[what] += 1
            content_ok = name[0] not in DISTINCT and (name[0] not in ZEROS or (
                what == "miss:zero" and mode == "sorted_lower" and ov[i] == 0))
            if not content_ok:
                bad.append(f"{name} {where}: {what} on a content that gives no reason; oracle {ov[i]!r}: "
                           f"{[wm.unpack_header(h) for h in hdr[:, i]][:4]}")
            if not np.isnan(gv[i]):
                bad.append(f"{name} {where}: a miss with value {gv[i]!r}")
            continue
        same = (gv[i].view(np.uint64) == ov[i].view(np.uint64)) or (np.isnan(gv[i]) and np.isnan(ov[i]))
        if mode == "linear":  # the sign of a zero LINEAR result is unspecified
            same = same or (gv[i] == 0 and ov[i] == 0)
        if not (same and gn[i] == on[i] and gf[i] == of[i]):
            bad.append(f"{name} {where}: {got} ({gv[i]!r}, {gn[i]}, {gf[i]}), oracle ({ov[i]!r}, {on[i]}, {of[i]})")
    assert not bad, f"{len(bad)} of {len(names)} series differ:\n" + "\n".join(bad[:8])
    assert misses == int(missed.sum()), (where, misses, int(missed.sum()))
    flags = np.concatenate([_flags(hdr[j]) for j in range(W)])
    print(f"window-lattice merge {where}: missed {_by_content(names, missed)} {dict(reasons)} "
          f"FAIL slices {int(((flags & wm.WIN_FAIL) != 0).sum())} POINT slices {int(((flags & wm.WIN_POINT) != 0).sum())}")


@pytest.mark.parametrize("p", list(PCT))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("W,rot", [(3, 0), (3, 1), (3, 5), (1, 0)], ids=["W3-rot0", "W3-rot1", "W3-rot5", "W1"])
def test_merge_equals_model_and_oracle(world, W, rot, kind, mode, p):
    """Per series: the kernel's outcome (hit, miss, nan, empty) is merge_model's on the headers
    and rows the export produced, the miss counter counts the misses, and every hit, nan and empty
    equals the oracle on the composed series in value, count and flags.  Misses have reasons: none
    on the distinct-valued contents, on the zeros contents only a zero SORTED_LOWER result.  The
    count of a missed series is not checked: it is not defined until the caller finishes it."""
    _assert_kind(kind, KINDS[kind])
    _check_merge(world, W, rot, kind, KINDS[kind], mode, p)


@pytest.mark.parametrize("p", ["100", "99"])
@pytest.mark.parametrize("mode", list(MODES))
def test_merge_64_slices(world, mode, p):
    """n_slices = 64, the wave-wide limit of k_window_merge (one header per lane): rows of 128
    (p100) and 192 (p99) keys, 64 and 96 KiB of keys in LDS, checked to fit before the launch."""
    kc = _key_cap(0, 63 * MAXLEN, _params(mode, p))
    assert kc == (128 if p == "100" else 192) and kc == wm.key_cap_for(MAXLEN, 63 * MAXLEN, PCT[p][0] / 100.0)
    assert LDS_FIXED + 64 * kc * 8 <= LDS_LIMIT
    _assert_kind("short", 0)
    _check_merge(world, 64, 1, "short", 0, mode, p)


def _parts(world, sl, declared, cuts):
    """The lattice as (lo, hi, KrrSeries) parts, each in buffers of its own."""
    import torch

    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v = sl.vals[sl.offs[lo]:sl.offs[hi]]
        d_v = torch.from_numpy(v.copy() if v.size else np.zeros(1)).to(world.dev)
        d_o = torch.from_numpy(sl.offs[lo:hi + 1] - sl.offs[lo]).to(world.dev)
        parts.append((lo, hi, world.ctx.series(d_v, d_o, declared or MAXLEN, world.gaps)))
    return parts


@pytest.mark.parametrize("p", ["100", "50", "0.1"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("form", ["whole", "parts"])
@pytest.mark.parametrize("j", [0, 1], ids=["slice0", "slice1"])
def test_world1_flow_is_exact(world, j, form, kind, mode, p):
    """sketch.window_exact_time_sharded at world size 1 over one lattice (slice lattice 0, and 1 with
    the shifted fillers: every offset differs), whole and as parts cut at
    segments [0, 1, 2, S // 3, S - 1, S] (a one-segment part, a filler-only part): after
    finish_window_misses every segment equals the oracle, and 'misses' is the number of series the
    model calls a miss on the returned headers (the rows restated from the samples)."""
    import torch

    from krr_amd.core import sketch

    _assert_kind(kind, KINDS[kind])
    sl = world.slice(j)
    declared = KINDS[kind]
    series = sl.series(declared) if form == "whole" else _parts(world, sl, declared, [0, 1, 2, sl.S // 3, sl.S - 1, sl.S])
    res = sketch.window_exact_time_sharded(world.ctx, series, _params(mode, p))
    torch.cuda.synchronize()
    gv, gn = res["value"].cpu().numpy(), res["count"].cpu().numpy()
    gf = res["flags"].cpu().numpy().view(np.uint32)
    ov, on, of = world.oracle_slice(j, mode, p)
    where = f"world1 slice={j} {form} layout={world.layout} kind={kind} mode={mode} p={p}"
    same = (gv.view(np.uint64) == ov.view(np.uint64)) | (np.isnan(gv) & np.isnan(ov))
    if mode == "linear":
        same |= (gv == 0) & (ov == 0)
    bad = np.flatnonzero(~(same & (gn == on) & (gf == of)))
    msg = [f"{sl.names[s]} {where}: got ({gv[s]!r}, {gn[s]}, {gf[s]}) want ({ov[s]!r}, {on[s]}, {of[s]})" for s in bad[:8]]
    assert bad.size == 0, f"{bad.size} of {sl.S} segments differ:\n" + "\n".join(msg)

    hdr, kc = res["hdr"].cpu().numpy(), int(res["key_cap"])
    assert hdr.shape == (sl.S, wm.HDR_WORDS)
    p_num, p_den = PCT[p]
    missed = np.zeros(sl.S, dtype=bool)
    for s in range(sl.S):
        lo, hi, _, _, cnt, flags = wm.unpack_header(hdr[s])
        row = np.full(max(kc, cnt), SENT_I, dtype=np.int64)
        if not flags & (wm.WIN_FAIL | wm.WIN_POINT | wm.FLAG_NAN):
            k = sl.keys[s]
            k = k[np.searchsorted(k, np.uint64(lo), "left"):np.searchsorted(k, np.uint64(hi), "right")]
            row[:min(k.size, row.size)] = k[:row.size].view(np.int64)
        what = wm.merge_model(hdr[s:s + 1], row[None, :kc], MODES[mode], p_num, p_den, float(p_num) / float(p_den) / 100.0)[0]
        missed[s] = what.startswith("miss")
    assert res["misses"] == int(missed.sum()), (where, res["misses"], _by_content(sl.names, missed))
    print(f"window-lattice {where}: missed {_by_content(sl.names, missed)}")

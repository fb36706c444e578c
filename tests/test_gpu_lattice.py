"""The percentile, max and rank kernels over the edge-geometry lattice (tests/_lattice.py; what
it covers is pinned by tests/test_lattice_layout.py), bit-exact against the references the other
GPU tests use: oracle.percentile / seg_max / locate, oracle.sketch_ref.build, numpy for rank_of
and select_present.

The comparison is tests/test_gpu_kernels.py::_assert_same: counts and flags equal, values equal
bit for bit or both NaN, and the sign of a zero LINEAR result exempt.  Outputs are pre-filled with
a sentinel, so an unwritten segment shows.  A failure names (content, length, parity) of each bad
segment with the kind, mode and percentile.

The launch kind follows the DECLARED max_segment_len (an upper bound: declaring more is legal),
so one 7K-slot lattice goes through every kernel kind.  Each test first asserts the kind with
_native.select_plan / multi_plan.  The planner (krr_plan.h, pinned by tests/test_abi.py
test_select_plan_decisions) decides three of them otherwise than one might expect, and the tables
below state what it does:

  * p50 at the lattice's true maximum (7,169 slots, 3,587 kept keys) is the short window, not
    the single pass: no legal declared length puts p50 of a 7K-slot launch through the single
    pass.  It runs here all the same, as one more window launch.
  * p99 with 172,800 declared slots (1,731 kept keys, a 2,432-key buffer) is the single pass
    with the big buffer only in the FUSED launch (fused_hselect == 0); alone it is the long
    window (hselect == 1).  Both run.  The stand-alone big buffer (hselect == 0, cap_keys > 2048,
    probe) is reached with p99.6 at 500,000 declared slots, added for that.
  * the set {50, 95, 99} never shares a pass at 7K slots (shared == 0 for SORTED_LOWER / LINEAR:
    p50's keys do not fit the single pass); its rows are compared through the per-percentile
    launches it takes, {0.1, 5} shares on the bottom side, and {95, 99} is added for the shared
    pass on the top side.  REF_INDEX always shares.

Both launches with >= 100,000 declared slots also turn the XCD remap off (KRR_XCD_REMAP_MAXLEN).
"""
import os
import sys

import numpy as np
import pytest

from oracle import oracle, sketch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lattice  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"ref_index": 0, "sorted_lower": 1, "linear": 2}
PCT = {"100": (100, 1), "99.6": (996, 10), "99": (99, 1), "95": (95, 1), "50": (50, 1), "5": (5, 1), "0.1": (1, 10)}
SENT_V, SENT_I = -777.25, -777
M, ELO, OCT = 5, -24, 36  # tests/test_gpu_sketch.py
TRUE = 0  # declared length: the lattice's true maximum

# kind, declared slots, percentile, hselect (krr_segmented_percentile), fused_hselect (krr_simple_run)
SELECT_CASES = [
    ("single", TRUE, "100", 0, 0),
    ("single", TRUE, "99", 0, 0),
    ("single", TRUE, "50", 1, 1),       # 3,587 kept keys: the short window (module docstring)
    ("single", TRUE, "5", 0, 0),
    ("single", TRUE, "0.1", 0, 0),
    ("bigbuf", 172_800, "99", 1, 0),    # the big buffer in the fused launch, the long window alone
    ("bigbuf", 500_000, "99.6", 0, 1),  # the big buffer alone, the long window fused
    ("short_window", 20_160, "50", 1, 1),
    ("short_window", 20_160, "5", 1, 1),
    ("long_window", 50_400, "50", 1, 1),
    ("long_window", 50_400, "95", 1, 1),
    ("long_window", 50_400, "5", 1, 1),
]
SELECT_IDS = [f"{k}-{d or 'true'}-p{p}" for k, d, p, _, _ in SELECT_CASES]
# percentile set -> shared for SORTED_LOWER / LINEAR at the true maximum (REF_INDEX: always 1)
SETS = {("50", "95", "99"): 0, ("0.1", "5"): 1, ("95", "99"): 1}
SET_IDS = ["p50_95_99", "p0.1_5", "p95_99"]


def _params(mode, p):
    from krr_amd import _native

    p_num, p_den = PCT[p]
    return _native.KrrPercentileParams(MODES[mode], 0, p_num, p_den, float(p_num) / float(p_den) / 100.0)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


class Lattice:
    """One lattice in HBM (uploaded once) with its references, each computed once and read-only."""

    def __init__(self, ctx, dev, gaps, seed, shift):
        import torch

        self.ctx, self.dev, self.gaps = ctx, dev, gaps
        self.vals, self.offs, self.index = _lattice.build(gaps, seed, shift)
        self.d_vals = torch.from_numpy(self.vals).to(dev)
        self.d_offs = torch.from_numpy(self.offs).to(dev)
        _frozen(self.vals, self.offs)
        self.names = _lattice.names(self.offs, self.index)
        self.S = self.offs.size - 1
        self.maxlen = int(np.diff(self.offs).max())
        self.segs = [self.vals[self.offs[s]:self.offs[s + 1]] for s in range(self.S)]
        self.present = [x[~np.isnan(x)] for x in self.segs]
        self._refs = {}

    def series(self, declared=TRUE):
        return self.ctx.series(self.d_vals, self.d_offs, declared or self.maxlen, self.gaps)

    def ref_pct(self, mode, p):
        key = (mode, p)
        if key not in self._refs:
            p_num, p_den = PCT[p]
            q = float(p_num) / float(p_den) / 100.0
            self._refs[key] = _frozen(*oracle.percentile(self.vals, self.offs, MODES[mode], p_num, p_den, q, self.gaps))
        return self._refs[key]

    def ref_max(self):
        if "max" not in self._refs:
            self._refs["max"] = _frozen(*oracle.seg_max(self.vals, self.offs, self.gaps))
        return self._refs["max"]

    def outs(self, rows=None):
        import torch

        shape = (self.S,) if rows is None else (rows, self.S)
        return (torch.full(shape, SENT_V, dtype=torch.float64, device=self.dev),
                torch.full((self.S,), SENT_I, dtype=torch.int64, device=self.dev),
                torch.full(shape, SENT_I, dtype=torch.int32, device=self.dev))

    def full(self, dtype, fill, shape=None):
        import torch

        return torch.full((self.S,) if shape is None else shape, fill, dtype=dtype, device=self.dev)

    def upload(self, a, dtype):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)


def _host(v, n, f):
    return v.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy().view(np.uint32)


def _check(lat, got, want, mode, kind, p):
    """_assert_same of tests/test_gpu_kernels.py, naming the bad segments."""
    gv, gn, gf = got
    wv, wn, wf = want
    same = (gv.view(np.uint64) == wv.view(np.uint64)) | (np.isnan(gv) & np.isnan(wv))
    if mode == "linear":  # sign of a zero result is unspecified (numpy's partition is unstable)
        same |= (gv == 0) & (wv == 0)
    bad = np.flatnonzero(~(same & (gn == wn) & (gf == wf.astype(np.uint32))))
    msg = [f"{lat.names[s]} kind={kind} mode={mode} p={p}: got ({gv[s]!r}, {gn[s]}, {gf[s]}) "
           f"want ({wv[s]!r}, {wn[s]}, {wf[s]})" for s in bad[:8]]
    assert bad.size == 0, f"{bad.size} of {lat.S} segments differ:\n" + "\n".join(msg)


def _check_ints(lat, got, want, what, kind):
    bad = np.flatnonzero(got != want)
    msg = [f"{lat.names[s]} kind={kind} {what}: got {got[s]} want {want[s]}" for s in bad[:8]]
    assert bad.size == 0, f"{bad.size} of {lat.S} segments differ:\n" + "\n".join(msg)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


@pytest.fixture(scope="module", params=["compact", "gapped"])
def world(request, gpu):
    """The CPU lattice and the memory lattice (another seed, fillers shifted: other offsets, the
    same segments) of one layout."""
    ctx, dev = gpu
    gaps = request.param == "gapped"
    cpu = Lattice(ctx, dev, gaps, seed=32 if gaps else 31, shift=0)
    mem = Lattice(ctx, dev, gaps, seed=42 if gaps else 41, shift=1)
    assert cpu.S == mem.S and cpu.index == mem.index and (cpu.offs[1:] != mem.offs[1:]).all()
    assert cpu.maxlen == mem.maxlen == 7 * 1024 + 1
    return cpu, mem


def _assert_select_plan(lat, kind, declared, mode, p, hselect, fused_hselect, fused):
    """The launch cannot pass by running another kernel: the plan of this declared length."""
    from krr_amd import _native

    plan = _native.select_plan(declared or lat.maxlen, _params(mode, p))
    assert (plan.hselect, plan.fused_hselect) == (hselect, fused_hselect), (kind, declared, p, plan.tkeep)
    window = plan.fused_hselect if fused else plan.hselect
    if kind == "single" and p != "50":
        assert not window and plan.cap_keys <= 2048
    if kind == "bigbuf" and not window:
        # the buffer krr_plan.h capacity_for gives these keys (half a chunk and 128 keys of margin
        # above them, in 64-key steps); cap_keys itself describes the stand-alone launch
        cap = (plan.tkeep + 512 + 128 + 63) // 64 * 64
        assert cap > 2048
        if not fused:
            assert plan.cap_keys == cap and plan.probe == 1
    if kind in ("short_window", "long_window"):
        assert window
        short = _native.select_plan(20_160, _params(mode, p))
        long_ = _native.select_plan(50_400, _params(mode, p))
        assert short.hselect == 1 and long_.hselect == 1 and long_.lds_bytes > short.lds_bytes
        assert plan.lds_bytes == (long_ if kind == "long_window" else short).lds_bytes


@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
@pytest.mark.parametrize("case", SELECT_CASES, ids=SELECT_IDS)
def test_select(world, case, mode):
    """krr_segmented_percentile: k_select in its single-pass, probe-backed, short-window and
    long-window forms."""
    import torch

    cpu, _ = world
    kind, declared, p, hselect, fused_hselect = case
    _assert_select_plan(cpu, kind, declared, mode, p, hselect, fused_hselect, fused=False)
    v, n, f = cpu.outs()
    cpu.ctx.segmented_percentile(cpu.series(declared), _params(mode, p), v, n, f)
    torch.cuda.synchronize()
    _check(cpu, _host(v, n, f), cpu.ref_pct(mode, p), mode, kind, p)


def _fused(cpu, mem, declared, params):
    import torch

    cv, cn, cf = cpu.outs()
    mv, mn, mf = mem.outs()
    out = dict(cpu_value=cv, cpu_count=cn, cpu_flags=cf, mem_value=mv, mem_count=mn, mem_flags=mf)
    cpu.ctx.simple_run(cpu.series(declared), mem.series(declared), params, out)
    torch.cuda.synchronize()
    return _host(cv, cn, cf), _host(mv, mn, mf)


@pytest.mark.parametrize("mode", ["sorted_lower", "linear"])
@pytest.mark.parametrize("case", SELECT_CASES, ids=SELECT_IDS)
def test_simple_run(world, case, mode):
    """krr_simple_run's fused k_simple in its four kinds; the memory half (the one-site MaxProc
    loop) runs over the second lattice.  Both halves are checked."""
    cpu, mem = world
    kind, declared, p, hselect, fused_hselect = case
    _assert_select_plan(cpu, kind, declared, mode, p, hselect, fused_hselect, fused=True)
    got_cpu, got_mem = _fused(cpu, mem, declared, _params(mode, p))
    _check(cpu, got_cpu, cpu.ref_pct(mode, p), mode, f"fused {kind}", p)
    _check(mem, got_mem, mem.ref_max(), "max", f"fused {kind} memory half", p)


@pytest.mark.parametrize("p", ["100", "99", "50", "0.1"])
def test_ref_index(world, p):
    """k_refindex_dense (compact) and k_refindex_gaps (gapped): on the edge and absent-edge contents
    k lands on slot 0 and slot L - 1, and refindex_walk starts from either end."""
    import torch

    cpu, _ = world
    v, n, f = cpu.outs()
    cpu.ctx.segmented_percentile(cpu.series(), _params("ref_index", p), v, n, f)
    torch.cuda.synchronize()
    _check(cpu, _host(v, n, f), cpu.ref_pct("ref_index", p), "ref_index", "refindex", p)


@pytest.mark.parametrize("p,declared", [("100", TRUE), ("99", TRUE), ("50", TRUE), ("0.1", TRUE), ("99", 172_800),
                                        ("50", 20_160), ("50", 50_400)])
def test_simple_run_ref_index(world, p, declared):
    """krr_simple_run with REF_INDEX: the fused CPU_REF_GAPS kernel on the gapped layout (the
    compact layout is a gather and k_max, two launches), at the four declared lengths."""
    cpu, mem = world
    got_cpu, got_mem = _fused(cpu, mem, declared, _params("ref_index", p))
    _check(cpu, got_cpu, cpu.ref_pct("ref_index", p), "ref_index", "fused refindex", p)
    _check(mem, got_mem, mem.ref_max(), "max", "fused refindex memory half", p)


@pytest.mark.parametrize("declared", [TRUE, 172_800], ids=["true", "172800"])
@pytest.mark.parametrize("which", ["cpu", "mem"])
def test_segmented_max(world, which, declared):
    """krr_segmented_max (k_max, the three-buffer loop) over both lattices, XCD remap on and off."""
    import torch

    lat = world[0] if which == "cpu" else world[1]
    v, n, f = lat.outs()
    lat.ctx.segmented_max(lat.series(declared), v, n, f)
    torch.cuda.synchronize()
    _check(lat, _host(v, n, f), lat.ref_max(), "max", "k_max", "-")


def _assert_multi_plan(lat, pset, mode):
    from krr_amd import _native

    plist = [_params(mode, p) for p in pset]
    want = 1 if mode == "ref_index" else SETS[pset]
    assert _native.multi_plan(lat.maxlen, plist).shared == want, (pset, mode)
    return plist


def _check_rows(lat, v, n, f, pset, mode, kind):
    cnt = n.cpu().numpy()
    for j, p in enumerate(pset):  # row j equals the single-percentile reference
        got = v[j].cpu().numpy(), cnt, f[j].cpu().numpy().view(np.uint32)
        _check(lat, got, lat.ref_pct(mode, p), mode, f"{kind} row {j} of {pset}", p)


@pytest.mark.parametrize("mode", ["sorted_lower", "linear", "ref_index"])
@pytest.mark.parametrize("pset", list(SETS), ids=SET_IDS)
def test_segmented_percentiles(world, pset, mode):
    import torch

    cpu, _ = world
    plist = _assert_multi_plan(cpu, pset, mode)
    v, n, f = cpu.outs(rows=len(pset))
    cpu.ctx.segmented_percentiles(cpu.series(), plist, v, n, f)
    torch.cuda.synchronize()
    _check_rows(cpu, v, n, f, pset, mode, "multi")


@pytest.mark.parametrize("mode", ["sorted_lower", "linear", "ref_index"])
@pytest.mark.parametrize("pset", list(SETS), ids=SET_IDS)
def test_simple_run_multi(world, pset, mode):
    """krr_simple_run_multi (k_simple_multi; REF_INDEX on the compact layout gathers and takes the
    memory max apart), the memory half over the second lattice."""
    import torch

    cpu, mem = world
    plist = _assert_multi_plan(cpu, pset, mode)
    cv, cn, cf = cpu.outs(rows=len(pset))
    mv, mn, mf = mem.outs()
    out = dict(cpu_value=cv, cpu_count=cn, cpu_flags=cf, mem_value=mv, mem_count=mn, mem_flags=mf)
    cpu.ctx.simple_run_multi(cpu.series(), mem.series(), plist, out)
    torch.cuda.synchronize()
    _check_rows(cpu, cv, cn, cf, pset, mode, "fused multi")
    _check(mem, _host(mv, mn, mf), mem.ref_max(), "max", "fused multi memory half", "-")


def _edge_values(lat, slot):
    """Each segment's slot-0 (slot = 0) or slot-(L - 1) (slot = -1) value; 0.5 for an empty one."""
    return np.array([x[slot] if x.size else 0.5 for x in lat.segs])


@pytest.mark.parametrize("probe", ["slot0", "slotL", "below", "above"])
def test_rank_of(world, probe):
    """k_rank_of counts present samples (a NaN compares false) in either layout."""
    import torch

    cpu, _ = world
    v = {"slot0": _edge_values(cpu, 0), "slotL": _edge_values(cpu, -1), "below": np.full(cpu.S, -np.inf),
         "above": np.full(cpu.S, np.inf)}[probe]
    lt, le = cpu.full(torch.int64, SENT_I), cpu.full(torch.int64, SENT_I)
    cpu.ctx.rank_of(cpu.series(), cpu.upload(v, np.float64), lt, le)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        want_lt = np.array([int((x < v[s]).sum()) for s, x in enumerate(cpu.present)])
        want_le = np.array([int((x <= v[s]).sum()) for s, x in enumerate(cpu.present)])
    if probe == "below":
        assert not want_le.any()
    if probe == "above":
        assert np.array_equal(want_lt, [x.size for x in cpu.present])
    _check_ints(cpu, lt.cpu().numpy(), want_lt, "lt", f"rank_of {probe}")
    _check_ints(cpu, le.cpu().numpy(), want_le, "le", f"rank_of {probe}")


@pytest.mark.parametrize("which", ["first", "last", "past_even", "past_odd"])
def test_locate(world, which):
    """k_locate: the slot-0 value with rank -1 (the first equal sample), the slot-(L - 1) value
    with the rank of its last equal sample, a rank past the equal group (pos -1) on every other
    segment and rank -2 (outputs untouched) on the rest."""
    import torch

    cpu, _ = world
    v = _edge_values(cpu, -1 if which == "last" else 0)
    with np.errstate(invalid="ignore"):
        lt = np.array([int((x < v[s]).sum()) for s, x in enumerate(cpu.segs)])
        eq = np.array([int((x == v[s]).sum()) for s, x in enumerate(cpu.segs)])
    if which == "first":
        rank = np.full(cpu.S, -1, dtype=np.int64)
    elif which == "last":
        rank = (lt + eq - 1).astype(np.int64)
    else:
        rank = (lt + eq).astype(np.int64)
        rank[(0 if which == "past_odd" else 1)::2] = -2
    outs = [cpu.full(torch.int64, SENT_I) for _ in range(3)]
    cpu.ctx.locate(cpu.series(), cpu.upload(v, np.float64), cpu.upload(rank, np.int64), *outs)
    torch.cuda.synchronize()
    want = oracle.locate(cpu.vals, cpu.offs, v, rank)
    for name, g, w in zip(("lt", "eq", "pos"), outs, want):
        w = np.where(rank < -1, SENT_I, w)
        _check_ints(cpu, g.cpu().numpy(), w, name, f"locate {which}")
    pos = outs[2].cpu().numpy()
    if which == "past_even":
        assert (pos[0::2] == -1).all() and (pos[1::2] == SENT_I).all()
    for (content, n, parity), s in cpu.index.items():  # the reference itself, on the edge contents
        if content in ("distinct", "edge_hi", "edge_lo") and n and which in ("first", "last"):
            assert want[2][s] == (0 if which == "first" else n - 1), (content, n, parity)


@pytest.mark.parametrize("which", ["k0", "n-1", "n", "-1"])
def test_select_present(world, which):
    """k_select_present: the first and the last present sample, one past them (NaN), and k = -1
    (skipped: the output keeps the sentinel)."""
    import torch

    cpu, _ = world
    n = np.array([(p if cpu.gaps else x).size for x, p in zip(cpu.segs, cpu.present)], dtype=np.int64)
    k = {"k0": np.zeros(cpu.S, dtype=np.int64), "n-1": n - 1, "n": n, "-1": np.full(cpu.S, -1, dtype=np.int64)}[which]
    out = cpu.full(torch.float64, SENT_V)
    cpu.ctx.select_present(cpu.series(), cpu.upload(k, np.int64), out)
    torch.cuda.synchronize()
    want = np.empty(cpu.S)
    for s in range(cpu.S):
        x = cpu.present[s] if cpu.gaps else cpu.segs[s]
        want[s] = SENT_V if k[s] < 0 else (x[k[s]] if k[s] < x.size else np.nan)
    got = out.cpu().numpy()
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~same)
    msg = [f"{cpu.names[s]} kind=select_present k={which}: got {got[s]!r} want {want[s]!r}" for s in bad[:8]]
    assert bad.size == 0, f"{bad.size} of {cpu.S} segments differ:\n" + "\n".join(msg)


def test_sketch_build(world):
    """k_sketch_build (the one-site loop with LDS atomics): counts bit for bit, vmin and vmax by
    value (np.min / np.max do not define a zero's sign), the NaN flag of the compact layout."""
    import torch

    from krr_amd import _native

    cpu, _ = world
    sp = _native.KrrSketchParams(M, ELO, OCT, 0)
    W = cpu.ctx.sketch_width(sp)
    assert W == sketch_ref.width(M, ELO, OCT)
    counts = cpu.full(torch.int32, SENT_I, (cpu.S, W))
    vmin, vmax = cpu.full(torch.float64, SENT_V), cpu.full(torch.float64, SENT_V)
    flags = cpu.full(torch.int32, SENT_I)
    cpu.ctx.sketch_build(cpu.series(), sp, counts, vmin, vmax, flags)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy().view(np.uint32)
    vmin, vmax, flags = vmin.cpu().numpy(), vmax.cpu().numpy(), flags.cpu().numpy()
    bad = []
    for s, x in enumerate(cpu.segs):
        c, mn, mx = sketch_ref.build(x, M, ELO, OCT)
        flag = 1 if (not cpu.gaps and np.isnan(x).any()) else 0
        ok = (np.array_equal(counts[s], c) and np.array_equal(vmin[s], mn, equal_nan=True)
              and np.array_equal(vmax[s], mx, equal_nan=True) and flags[s] == flag)
        if not ok:
            bad.append(f"{cpu.names[s]} kind=sketch_build: vmin {vmin[s]!r}/{mn!r} vmax {vmax[s]!r}/{mx!r} "
                       f"flags {flags[s]}/{flag} counts differ at {np.flatnonzero(counts[s] != c)[:4]}")
    assert not bad, f"{len(bad)} of {cpu.S} segments differ:\n" + "\n".join(bad[:8])

"""krr_group_max on the MI355X, alone: per group the first maximal item with np.max's NaN
propagation, against a numpy restatement of the header's rules written here.  Outputs are
pre-filled with sentinels, so an unwritten slot is seen; values are compared by their bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY, NAN, CAP = 4, 1, 2
QNAN = np.uint64(0x7FF8000000000000)
SIZES = [0, 1, 2, 63, 64, 65, 128, 129, 1000]


@pytest.fixture(scope="module")
def gpu():
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    yield ctx, torch.device("cuda:0")
    ctx.close()


def fold(goffs, v, n, f):
    """The rules of include/krr_amd.h restated: v, f [R, N]; n [N] -> value bits, count, flags, arg."""
    R, G = v.shape[0], goffs.size - 1
    ov = np.zeros((R, G), dtype=np.uint64)
    on = np.zeros(G, dtype=np.int64)
    of = np.zeros((R, G), dtype=np.uint32)
    oa = np.zeros((R, G), dtype=np.int64)
    bits = v.view(np.uint64)
    for r in range(R):
        for g in range(G):
            a, e = int(goffs[g]), int(goffs[g + 1])
            items = [i for i in range(a, e) if not f[r, i] & EMPTY]
            if r == 0:
                on[g] = sum(int(n[i]) for i in items)
            if not items:
                ov[r, g], of[r, g], oa[r, g] = QNAN, EMPTY, -1
                continue
            of[r, g] = np.bitwise_or.reduce(f[r, items])
            bad = [i for i in items if f[r, i] & (NAN | CAP) or np.isnan(v[r, i])]
            if bad:
                ov[r, g], oa[r, g] = QNAN, bad[0] - a
                continue
            best = items[0]
            for i in items[1:]:
                if v[r, i] > v[r, best]:  # float comparison: -0.0 == +0.0, the earlier one stays
                    best = i
            ov[r, g], oa[r, g] = bits[r, best], best - a
    return ov, on, of, oa


def make_inputs(rows, seed):
    """Groups of SIZES, then hand-made groups for every rule; returns goffs, v, n, f and the
    hand-made groups' indices by name."""
    rng = np.random.default_rng(seed)
    groups, names = [], {}

    def add(name, vals, flags=None, counts=None):
        vals = np.asarray(vals, dtype=np.float64)
        names[name] = len(groups)
        groups.append((vals, np.zeros(vals.size, dtype=np.uint32) if flags is None else np.asarray(flags, np.uint32),
                       rng.integers(1, 5000, vals.size) if counts is None else np.asarray(counts, np.int64)))

    for size in SIZES:  # few distinct values: ties everywhere
        add(f"size{size}", rng.integers(-3, 4, size).astype(np.float64) * 0.25)
    base = -1.0 - rng.random(200)
    t = base.copy()
    t[[5, 70]] = 7.5                      # equal maxima in different lanes
    add("tie_lanes", t[:130])
    t = base.copy()
    t[[3, 67, 131]] = 7.5                 # equal maxima in different strides of lane 3
    add("tie_strides", t)
    t = base[:80].copy()
    t[2], t[9] = -0.0, 0.0                # -0.0 before +0.0: the earlier one's bits
    add("neg_zero_first", t)
    t = base[:80].copy()
    t[2], t[9] = 0.0, -0.0
    add("pos_zero_first", t)
    t = base[:80].copy()
    t[66], t[1] = 0.0, -0.0               # the same across a stride (lanes 2 and 1)
    add("zero_strides", t)
    t = rng.random(150)
    fl = np.zeros(150, dtype=np.uint32)
    for i in (0, 1, 77, 148, 149):        # EMPTY at the start, in the middle and at the end
        fl[i], t[i] = EMPTY, 1e300        # a skipped item's value must not win
    cn = rng.integers(1, 5000, 150)
    cn[[0, 77, 149]] = 0
    add("empty_edges", t, fl, cn)
    add("all_empty", np.full(70, np.nan), np.full(70, EMPTY, dtype=np.uint32), np.zeros(70, dtype=np.int64))
    t, fl = rng.random(100), np.zeros(100, dtype=np.uint32)
    fl[40] = NAN
    t[40] = np.nan
    add("nan_flag", t, fl)
    t = rng.random(100)
    t[[90, 12]] = np.nan                  # NaN values without a flag: the first one is the index
    add("nan_value", t)
    t, fl = rng.random(100), np.zeros(100, dtype=np.uint32)
    fl[64] = CAP | (0x37 << 8)            # CAPACITY with a reason in bits 8..15
    fl[3] = 0x1200                        # reason bits of a clean item are OR-ed in too
    add("capacity", t, fl)
    add("infs", [1.0, np.inf, -np.inf, np.inf, 2.0])
    add("neg_inf_only", [-np.inf, -np.inf])

    v1 = np.concatenate([g[0] for g in groups])
    f1 = np.concatenate([g[1] for g in groups])
    n = np.concatenate([g[2] for g in groups]).astype(np.int64)
    goffs = np.concatenate([[0], np.cumsum([g[0].size for g in groups])]).astype(np.int64)
    v = np.stack([v1] + [np.where(f1 & EMPTY, v1, rng.integers(-2, 3, v1.size) * 0.5) for _ in range(rows - 1)])
    f = np.stack([f1] * rows)
    if rows > 1:  # a later row's own bad item
        i = int(goffs[names["size129"]]) + 100
        f[rows - 1, i] = NAN
    return goffs, np.ascontiguousarray(v), n, np.ascontiguousarray(f), names


def run(gpu, goffs, v, n, f, records=False, arg=True):
    import torch

    ctx, dev = gpu
    R, G = v.shape[0], goffs.size - 1
    shape = (R, G) if R > 1 else (G,)
    ov = torch.full(shape, -777.0, dtype=torch.float64, device=dev)
    on = torch.full((G,), -7, dtype=torch.int64, device=dev)
    of = torch.full(shape, -1, dtype=torch.int32, device=dev)
    oa = torch.full(shape, -99, dtype=torch.int64, device=dev) if arg else None
    rec = torch.full((G, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) if records else None
    iv = torch.from_numpy(v if R > 1 else v[0]).to(dev)
    fl = torch.from_numpy((f if R > 1 else f[0]).view(np.int32)).to(dev)
    ctx.group_max(torch.from_numpy(goffs).to(dev), iv, torch.from_numpy(n).to(dev), fl, ov, on, of, oa, records=rec)
    torch.cuda.synchronize()
    return (ov.cpu().numpy().reshape(R, G).view(np.uint64), on.cpu().numpy(),
            of.cpu().numpy().reshape(R, G).view(np.uint32), oa.cpu().numpy().reshape(R, G) if arg else None,
            rec.cpu().numpy() if records else None)


@pytest.mark.parametrize("rows", [1, 2, 4])
def test_group_max_matches_the_rules(gpu, rows):
    goffs, v, n, f, names = make_inputs(rows, 100 + rows)
    wv, wn, wf, wa = fold(goffs, v, n, f)
    gv, gn, gf, ga, _ = run(gpu, goffs, v, n, f)
    bad = np.argwhere(gv != wv)
    assert bad.size == 0, (bad[:5], [k for k, g in names.items() if g in bad[:, 1]])
    assert np.array_equal(gn, wn)
    assert np.array_equal(gf, wf)
    assert np.array_equal(ga, wa)
    # the restatement itself says what the hand-made groups are there for
    g = names
    assert wa[0, g["tie_lanes"]] == 5 and wa[0, g["tie_strides"]] == 3
    assert wv[0, g["neg_zero_first"]] == np.uint64(1) << np.uint64(63) and wa[0, g["neg_zero_first"]] == 2
    assert wv[0, g["pos_zero_first"]] == 0 and wa[0, g["pos_zero_first"]] == 2
    assert wv[0, g["zero_strides"]] == np.uint64(1) << np.uint64(63) and wa[0, g["zero_strides"]] == 1
    assert wf[0, g["all_empty"]] == EMPTY and wa[0, g["all_empty"]] == -1 and wn[g["all_empty"]] == 0
    assert wf[0, g["size0"]] == EMPTY and wv[0, g["size0"]] == QNAN
    assert wf[0, g["empty_edges"]] == 0 and wv[0, g["empty_edges"]] != np.float64(1e300).view(np.uint64)
    assert wv[0, g["nan_flag"]] == QNAN and wa[0, g["nan_flag"]] == 40 and wf[0, g["nan_flag"]] == NAN
    assert wv[0, g["nan_value"]] == QNAN and wa[0, g["nan_value"]] == 12 and wf[0, g["nan_value"]] == 0
    assert wf[0, g["capacity"]] == CAP | 0x3700 | 0x1200 and wa[0, g["capacity"]] == 64
    assert wa[0, g["infs"]] == 1 and wa[0, g["neg_inf_only"]] == 0


def test_records_get_the_cpu_half_only(gpu):
    goffs, v, n, f, _ = make_inputs(1, 7)
    gv, gn, gf, _, rec = run(gpu, goffs, v, n, f, records=True, arg=False)  # out_arg NULL
    wv, wn, wf, _ = fold(goffs, v, n, f)
    assert np.array_equal(gv, wv) and np.array_equal(gn, wn) and np.array_equal(gf, wf)
    assert np.array_equal(rec[:, 0].view(np.uint64), gv[0])
    assert np.array_equal(rec[:, 2], gn | (gf[0].astype(np.int64) << 48))
    assert (rec[:, 1] == 0x5A5A5A5A5A5A5A5A).all() and (rec[:, 3] == 0x5A5A5A5A5A5A5A5A).all()


def test_no_groups_writes_nothing_and_many_groups_stride(gpu):
    import torch

    from krr_amd import _native

    ctx, dev = gpu
    ov = torch.full((3,), -777.0, dtype=torch.float64, device=dev)
    on = torch.full((3,), -7, dtype=torch.int64, device=dev)
    of = torch.full((3,), -1, dtype=torch.int32, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.group_max(z, torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                  torch.zeros(0, dtype=torch.int32, device=dev), ov, on, of)
    torch.cuda.synchronize()
    assert (ov == -777.0).all() and (on == -7).all() and (of == -1).all()
    # records with more than one row, and a row count out of range: KRR_E_INVALID
    with pytest.raises(_native.NativeError) as e:
        ctx.group_max(torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros((2, 0), dtype=torch.float64, device=dev),
                      torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((2, 0), dtype=torch.int32, device=dev),
                      torch.zeros((2, 1), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                      torch.zeros((2, 1), dtype=torch.int32, device=dev),
                      records=torch.zeros((1, 4), dtype=torch.int64, device=dev))
    assert e.value.code == _native.KRR_E_INVALID
    # more groups than the launch has waves: the grid strides over them
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 4, 70_000)
    goffs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(goffs[-1])
    v = rng.integers(-3, 4, N).astype(np.float64)[None]
    f = np.where(rng.random(N) < 0.1, EMPTY, 0).astype(np.uint32)[None]
    n = rng.integers(0, 100, N).astype(np.int64)
    gv, gn, gf, ga, _ = run((ctx, dev), goffs, v, n, f)
    # vectorised restatement for this size: per group the first maximum among the non-EMPTY items
    wv, wn, wf, wa = fold(goffs[:2001], v, n, f)
    assert np.array_equal(gv[:, :2000], wv) and np.array_equal(gn[:2000], wn)
    assert np.array_equal(gf[:, :2000], wf) and np.array_equal(ga[:, :2000], wa)
    tail = slice(68_000, 70_000)
    goffs_t = goffs[68_000:] - goffs[68_000]
    a, b = int(goffs[68_000]), int(goffs[-1])
    wv, wn, wf, wa = fold(goffs_t, v[:, a:b], n[a:b], f[:, a:b])
    assert np.array_equal(gv[:, tail], wv) and np.array_equal(gn[tail], wn)
    assert np.array_equal(gf[:, tail], wf) and np.array_equal(ga[:, tail], wa)
    assert not (gn == -7).any() and not (ga == -99).any()

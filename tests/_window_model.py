"""The exact part of the window export / merge (include/krr_amd.h, "window export"; config 5),
restated in plain numpy: no GPU, no torch.  tests/test_window_model.py pins the model against the
oracle, tests/test_gpu_window_lattice.py holds the kernels to it.

A header is one row of HDR_WORDS int64 words, as _native.KrrWindowHdr lays it out: lo and hi as
key bits, below, n, cnt | flags << 32.  A key row is int64 too (uint64 key bit patterns); rows
and headers a kernel is to fill start as SENTINEL, which is no present sample's key (it lies above
the key of +inf), so an unwritten word shows.

What is pinned is what the header promises: n, below, cnt and the row are exact counts of the
slice's samples against [lo, hi], whichever window the export chose, and the merge decides hit or
miss from those counts alone.  How a window is chosen (z, keep limits, bins) is left free.
"""
import numpy as np

CHUNK = 1024
HDR_WORDS = 5
SENTINEL = -777
FLAG_NAN, FLAG_EMPTY, FLAG_WINDOW_MISS = 1, 4, 16  # KRR_FLAG_*
WIN_FAIL, WIN_POINT = 0x100, 0x200                 # KRR_WIN_*
SORTED_LOWER, LINEAR = 1, 2                        # KRR_PCT_*
WEXP_Z = 6.0                                       # KRR_WEXP_Z
SIGN = np.uint64(1 << 63)
KEY_NEG_INF = np.uint64(0x000FFFFFFFFFFFFF)        # okey(-inf)
KEY_POS_INF = np.uint64(0xFFF0000000000000)        # okey(+inf)
KEY_NEG_ZERO = np.uint64(0x7FFFFFFFFFFFFFFF)       # okey(-0.0)
KEY_POS_ZERO = np.uint64(0x8000000000000000)       # okey(+0.0)


def okey(x) -> np.ndarray:
    """The order-preserving uint64 key of krr_kernels.hip: a negative has every bit flipped, any
    other value has the sign bit set, so -0 < +0 and the keys sort as the numbers do."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def okey_inv(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ SIGN, ~k).view(np.float64)


def sorted_keys(x) -> np.ndarray:
    """The ascending keys of the present (non-NaN) samples of x."""
    x = np.asarray(x, dtype=np.float64)
    k = okey(x[~np.isnan(x)])
    k.sort()
    return k


def pack_header(lo, hi, below, n, cnt, flags) -> np.ndarray:
    h = np.empty(HDR_WORDS, dtype=np.uint64)
    for i, w in enumerate((lo, hi, below, n, int(cnt) | int(flags) << 32)):
        h[i] = np.uint64(int(w) % 2**64)
    return h.view(np.int64)


def unpack_header(hdr):
    """lo, hi (Python ints, unsigned), below, n, cnt, flags."""
    h = np.asarray(hdr, dtype=np.int64)
    last = int(h[4]) % 2**64
    return int(h[0]) % 2**64, int(h[1]) % 2**64, int(h[2]), int(h[3]), last & 0xFFFFFFFF, last >> 32


def key_cap_for(max_slice_len: int, ext: int, q: float) -> int:
    """krr_window_key_cap written out: 2 ceil(z sigma + 4) + 2 ranks and 64 keys of room for
    keys equal to the bounds, in 64-key steps."""
    L, U = float(max_slice_len), float(ext)
    sig = np.sqrt(q * (1.0 - q) * L * U / (L + U)) if L > 0 and U > 0 else 0.0
    keys = 2 * int(np.ceil(WEXP_Z * sig + 4.0)) + 2 + 64
    return (keys + 63) // 64 * 64


def check_header(x, gaps, hdr, row, key_cap, sentinel=SENTINEL, keys=None) -> list:
    """The promise of krr_window_hdr for the slice with samples x: a list of violations (short
    strings), empty when the header and its row keep it.  keys: sorted_keys(x), if the caller has
    them already."""
    x = np.asarray(x, dtype=np.float64)
    row = np.asarray(row, dtype=np.int64)
    lo, hi, below, n, cnt, flags = unpack_header(hdr)
    has_nan = bool(np.isnan(x).any())
    out = []
    if not gaps and has_nan:  # the compact layout propagates a NaN sample: nothing else is promised
        if not flags & FLAG_NAN:
            out.append("flags: a compact slice with a NaN sample lacks KRR_FLAG_NAN")
        if n != x.size:
            out.append(f"n: {n}, a compact slice of {x.size} slots")
        return out
    if flags & FLAG_NAN:
        out.append("flags: KRR_FLAG_NAN on a slice without a NaN sample" if not gaps else
                   "flags: KRR_FLAG_NAN in the gapped layout")
    untouched = bool((row == sentinel).all())
    if flags & WIN_FAIL:  # the counts mean nothing; no keys were stored
        if not untouched:
            out.append("row: written under KRR_WIN_FAIL")
        return out
    if keys is None:
        keys = sorted_keys(x)
    if n != keys.size:
        out.append(f"n: {n}, present samples {keys.size} of {x.size} slots")
    if lo > hi:
        out.append(f"lo > hi: {lo:#x} > {hi:#x}")
        return out
    b = int(np.searchsorted(keys, np.uint64(lo), "left"))
    e = int(np.searchsorted(keys, np.uint64(hi), "right"))
    if below != b:
        out.append(f"below: {below}, present keys < lo {b}")
    if cnt != e - b:
        out.append(f"cnt: {cnt}, present keys in [lo, hi] {e - b}")
    if flags & WIN_POINT:
        if lo != hi:
            out.append(f"POINT with lo != hi: {lo:#x}, {hi:#x}")
        if not untouched:
            out.append("row: written under KRR_WIN_POINT")
        return out
    if cnt > key_cap:
        out.append(f"cnt: {cnt} keys in a row of {key_cap} without KRR_WIN_FAIL")
    c = min(cnt, row.size)
    got = np.sort(row[:c].view(np.uint64))
    if not np.array_equal(got, keys[b:e]):
        out.append(f"row: its first {c} keys are not the {e - b} keys of the slice in [lo, hi]")
    if not (row[c:] == sentinel).all():
        out.append(f"row: written past its first {c} keys")
    return out


def ranks_for(mode, n, p_num, p_den, q):
    """ranks_for of krr_kernels.hip among n present samples: r0, r1, gamma."""
    if mode == SORTED_LOWER:
        r = (n - 1) * p_num // (100 * p_den)
        return r, r, 0.0
    vidx = float(n - 1) * q
    if vidx >= float(n - 1):
        return n - 1, n - 1, vidx + 1.0  # numpy subtracts the clipped index -1
    fl = float(np.floor(vidx))
    return int(fl), int(fl) + 1, vidx - fl


def np_lerp(a, b, t):
    """numpy's _lerp, every operation rounded by itself."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    with np.errstate(invalid="ignore"):
        d = b - a
        return b - d * (np.float64(1.0) - t) if t >= 0.5 else a + d * t


def _merge(hdrs, rows):
    """The slices' common window: any_nan, any_fail, n, Lk, Hk, cb (present samples below Lk),
    the ascending in-range keys (POINT copies included)."""
    h = np.asarray(hdrs, dtype=np.int64).reshape(-1, HDR_WORDS)
    R = np.asarray(rows, dtype=np.int64).reshape(h.shape[0], -1).view(np.uint64)
    key_cap = R.shape[1]
    lo, hi = h[:, 0].view(np.uint64), h[:, 1].view(np.uint64)
    last = h[:, 4].view(np.uint64)
    cnt = (last & np.uint64(0xFFFFFFFF)).astype(np.int64)
    flags = (last >> np.uint64(32)).astype(np.int64)
    point = (flags & WIN_POINT) != 0
    any_nan = bool(((flags & FLAG_NAN) != 0).any())
    # a row longer than key_cap cannot come from the export: no window
    any_fail = bool((((flags & WIN_FAIL) != 0) | (~point & (cnt > key_cap))).any())
    n = int(h[:, 3].sum())
    Lk, Hk = lo.max(), hi.min()
    if any_nan or any_fail or Lk > Hk:
        return any_nan, any_fail, n, Lk, Hk, 0, np.empty(0, dtype=np.uint64)
    valid = (np.arange(key_cap)[None, :] < cnt[:, None]) & ~point[:, None]
    inr = valid & (R >= Lk) & (R <= Hk)
    cb = int(h[:, 2].sum()) + int((valid & (R < Lk)).sum()) + int(cnt[point & (lo < Lk)].sum())
    pts = point & (lo >= Lk) & (lo <= Hk)  # cnt copies of lo each
    merged = np.concatenate([R[inr], np.repeat(lo[pts], cnt[pts])])
    merged.sort()
    return any_nan, any_fail, n, Lk, Hk, cb, merged


def merge_keys(hdrs, rows, r0, r1):
    """The keys at ranks r0 and r1 of the series, selected from the merged rows of a hit."""
    _, _, _, _, _, cb, merged = _merge(hdrs, rows)
    return merged[r0 - cb], merged[r1 - cb]


def merge_model(hdrs, rows, mode, p_num, p_den, q):
    """k_window_merge for one series from its W headers [W, HDR_WORDS] and rows [W, key_cap]:
    ("nan" | "empty" | "miss:fail" | "miss:disjoint" | "miss:ranks" | "miss:zero" | "hit", n, r0, r1),
    n the summed count as the kernel writes it, the ranks -1 where none is taken."""
    any_nan, any_fail, n, Lk, Hk, cb, merged = _merge(hdrs, rows)
    if any_nan:
        return "nan", n, -1, -1
    if n == 0:
        return "empty", n, -1, -1
    r0, r1, _ = ranks_for(mode, n, p_num, p_den, q)
    if any_fail:
        return "miss:fail", n, r0, r1
    if Lk > Hk:
        return "miss:disjoint", n, r0, r1
    if not (cb <= r0 and r1 < cb + merged.size):
        return "miss:ranks", n, r0, r1
    # a zero's sign under SORTED_LOWER is decided by position in the whole series, not by keys
    if mode == SORTED_LOWER and merged[r0 - cb] in (KEY_NEG_ZERO, KEY_POS_ZERO):
        return "miss:zero", n, r0, r1
    return "hit", n, r0, r1


def compose(lattices, rot):
    """The time-sharded series over W slice lattices (each the values, offsets, index of
    _lattice.build with one layout: the same index, other seeds and offsets).  Series
    (content, LENGTHS_c[t], parity) has, as its j-th slice, slice lattice j's segment
    (content, LENGTHS_c[(t + j rot) % len(LENGTHS_c)], parity), LENGTHS_c being the content's
    lengths in ascending order; filler i has filler i of every lattice.  Series are numbered as
    the segments of one lattice are.

    Returns perms [W, S] (perms[j, i]: the segment of lattice j that is slice j of series i) and
    the composed series (values, offsets), each the concatenation of its slices in time order."""
    index = lattices[0][2]
    S = lattices[0][1].size - 1
    lengths = {}
    for content, n, _ in index:
        if n not in lengths.setdefault(content, []):
            lengths[content].append(n)
    perms = np.tile(np.arange(S, dtype=np.int64), (len(lattices), 1))
    for j, (_, offs, idx) in enumerate(lattices):
        assert idx == index and offs.size - 1 == S
        for (content, n, parity), s in index.items():
            ls = lengths[content]
            perms[j, s] = index[(content, ls[(ls.index(n) + j * rot) % len(ls)], parity)]
    pieces = []
    for i in range(S):
        for j, (vals, offs, _) in enumerate(lattices):
            s = perms[j, i]
            pieces.append(vals[offs[s]:offs[s + 1]])
    sizes = np.array([p.size for p in pieces], dtype=np.int64).reshape(S, len(lattices)).sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return perms, np.concatenate(pieces), offsets


def numpy_export(x, gaps, q, ext, key_cap, sentinel=SENTINEL):
    """A deliberately simple exporter (the CPU tests' stand-in for krr_window_export): header and
    row of the slice x.  The window is every key when they fit the row, else exact bounds at the
    ranks floor(c - w) and ceil(c + w) + 1 with c = q (n - 1), w = 6 sigma + 4 and sigma as in
    export_shrink (a rank at or past an end of the slice leaves that side open); a row longer than
    key_cap is a FAIL."""
    x = np.asarray(x, dtype=np.float64)
    row = np.full(key_cap, sentinel, dtype=np.int64)
    if not gaps and np.isnan(x).any():
        return pack_header(KEY_NEG_INF, KEY_POS_INF, 0, x.size, 0, FLAG_NAN), row
    keys = sorted_keys(x)
    n = keys.size
    lo, hi, b, e = KEY_NEG_INF, KEY_POS_INF, 0, n
    if n > key_cap:
        S, U = float(n), float(ext)
        c = q * (S - 1.0)
        sig = np.sqrt(q * (1.0 - q) * S * U / (S + U)) if U > 0.0 else 0.0
        w = WEXP_Z * sig + 4.0
        ilo = min(max(int(np.floor(c - w)), 0), n - 1)
        ihi = min(max(int(np.ceil(c + w)) + 1, 0), n - 1)
        # a rank past either end leaves that bound open, as export_shrink does
        lo = keys[ilo] if ilo > 0 else lo
        hi = keys[ihi] if ihi < n - 1 else hi
        b = int(np.searchsorted(keys, lo, "left"))
        e = int(np.searchsorted(keys, hi, "right"))
    if e - b > key_cap:
        return pack_header(lo, hi, b, n, e - b, WIN_FAIL), row
    row[:e - b] = keys[b:e].view(np.int64)
    return pack_header(lo, hi, b, n, e - b, 0), row

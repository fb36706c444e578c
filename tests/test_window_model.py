"""CPU: tests/_window_model.py against the oracle, over the edge-geometry lattice cut into time
slices (_window_model.compose).  Three things are pinned, so that the GPU tests
(tests/test_gpu_window_lattice.py) can hold the kernels to the model:

  * merge_model over headers that keep the promise of krr_window_hdr (here: numpy_export's)
    never calls a series a hit whose merged rows do not hold the oracle's result;
  * its miss conditions fire only where the data give the reason: never on the distinct-valued
    contents, on the zeros contents only as a zero SORTED_LOWER result, and a failed export only
    on the contents that repeat keys;
  * check_header reports each way a header or its row can break the promise.
"""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lattice  # noqa: E402
import _window_model as wm  # noqa: E402

W = 3
MODES = {"sorted_lower": wm.SORTED_LOWER, "linear": wm.LINEAR}
PCT = {"100": (100, 1), "99": (99, 1), "95": (95, 1), "50": (50, 1), "5": (5, 1), "0.1": (1, 10)}
MAXLEN = 7 * 1024 + 1
# contents whose values are distinct (a NaN sample or absent slots change nothing in that)
DISTINCT = {"distinct", "edge_hi", "edge_lo", "absent0", "absentL", "absent0L", "absent_all", "nan0", "nanL",
            "nanmid", "filler"}
ZEROS = {"zeros", "zeros_swap"}
REPEATS = {"ties", "const"}


def _q(p):
    p_num, p_den = PCT[p]
    return float(p_num) / float(p_den) / 100.0


@functools.lru_cache(maxsize=None)
def _lattices(gaps):
    """Slice j: seed 31 (compact) / 32 (gapped) + 10 j, the fillers shifted on the odd slices."""
    out = [_lattice.build(gaps, (32 if gaps else 31) + 10 * j, shift=j % 2) for j in range(W)]
    for vals, offs, _ in out:
        vals.flags.writeable = offs.flags.writeable = False
        assert int(np.diff(offs).max()) == MAXLEN
    return out


@functools.lru_cache(maxsize=None)
def _composed(gaps, rot):
    lat = _lattices(gaps)
    perms, vals, offs = wm.compose(lat, rot)
    return perms, vals, offs, _lattice.names(lat[0][1], lat[0][2])


@functools.lru_cache(maxsize=None)
def _exports(gaps, p, ext):
    """numpy_export of every segment of every slice lattice: per slice, headers [S, 5] and rows."""
    q = _q(p)
    key_cap = wm.key_cap_for(MAXLEN, ext, q)
    out = []
    for vals, offs, _ in _lattices(gaps):
        S = offs.size - 1
        hdr = np.empty((S, wm.HDR_WORDS), dtype=np.int64)
        rows = np.empty((S, key_cap), dtype=np.int64)
        for s in range(S):
            hdr[s], rows[s] = wm.numpy_export(vals[offs[s]:offs[s + 1]], gaps, q, ext, key_cap)
        out.append((hdr, rows))
    return key_cap, out


@functools.lru_cache(maxsize=None)
def _outcomes(gaps, rot, mode, p):
    """Per series: merge_model's outcome over the numpy exports, and the headers and rows it saw."""
    perms, _, _, _ = _composed(gaps, rot)
    _, exp = _exports(gaps, p, (W - 1) * MAXLEN)
    p_num, p_den = PCT[p]
    out = []
    for i in range(perms.shape[1]):
        hdrs = np.stack([exp[j][0][perms[j, i]] for j in range(W)])
        rows = np.stack([exp[j][1][perms[j, i]] for j in range(W)])
        out.append((wm.merge_model(hdrs, rows, MODES[mode], p_num, p_den, _q(p)), hdrs, rows))
    return out


def test_compose_cuts_unequal_slices():
    """rot = 0: every slice of a series has its length; rot = 1 and 5: series of 0, 1 and 2 slots
    and of 1,023, 4,097 and 65 slots exist, and odd and even slice offsets meet in one series."""
    for gaps in (False, True):
        lat = _lattices(gaps)
        assert all(l[2] == lat[0][2] for l in lat) and (lat[0][1][1:] != lat[1][1][1:]).all()
        for rot in (0, 1, 5):
            perms, vals, offs, names = _composed(gaps, rot)
            lens = np.stack([np.diff(lat[j][1])[perms[j]] for j in range(W)])  # [W, S]
            assert np.array_equal(lens.sum(axis=0), np.diff(offs)) and offs[-1] == vals.size
            assert np.array_equal(perms[0], np.arange(perms.shape[1]))
            for j in range(W):
                assert np.array_equal(np.sort(perms[j]), np.arange(perms.shape[1]))
            case = np.array([n[0] != "filler" for n in names])
            assert (perms[:, ~case] == np.flatnonzero(~case)).all()
            if rot == 0:
                assert (lens[:, case] == lens[0, case]).all()
            else:
                shapes = {tuple(int(n) for n in lens[:, i]) for i in np.flatnonzero(case)}
                want = [(0, 1, 2), (2049, 3071, 3072)] if rot == 1 else [(0, 64, 1023), (1023, 2048, 4095)]
                assert all(w in shapes for w in want), (rot, sorted(shapes)[:8])
                # slices shorter than a chunk and of several chunks in one series
                assert any(min(s) < wm.CHUNK and max(s) > 4 * wm.CHUNK for s in shapes)


@pytest.mark.parametrize("p", list(PCT))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rot", [0, 1, 5])
@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_model_hits_equal_oracle(gaps, rot, mode, p):
    _, vals, offs, names = _composed(gaps, rot)
    p_num, p_den = PCT[p]
    ov, on, of = oracle.percentile(vals, offs, MODES[mode], p_num, p_den, _q(p), gaps)
    bad, hits = [], 0
    for i, ((what, n, r0, r1), hdrs, rows) in enumerate(_outcomes(gaps, rot, mode, p)):
        where = f"{names[i]} rot={rot} mode={mode} p={p}: {what}"
        if n != on[i]:
            bad.append(f"{where}: n {n}, oracle {on[i]}")
        if (what == "nan") != bool(of[i] & wm.FLAG_NAN) or (what == "empty") != bool(of[i] & wm.FLAG_EMPTY):
            bad.append(f"{where}: oracle flags {of[i]}")
        if what != "hit":
            continue
        hits += 1
        k0, k1 = wm.merge_keys(hdrs, rows, r0, r1)
        a, b = wm.okey_inv(k0), wm.okey_inv(k1)
        got = a if mode == "sorted_lower" else wm.np_lerp(a, b, wm.ranks_for(MODES[mode], n, p_num, p_den, _q(p))[2])
        same = np.float64(got).view(np.uint64) == ov[i].view(np.uint64)
        if mode == "linear":  # the sign of a zero LINEAR result is unspecified
            same |= got == 0 and ov[i] == 0
        if not same or of[i] != 0:
            bad.append(f"{where}: got {got!r}, oracle {ov[i]!r} flags {of[i]}")
    assert not bad, f"{len(bad)} series differ:\n" + "\n".join(bad[:8])
    assert hits > len(names) // 2


@pytest.mark.parametrize("p", list(PCT))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rot", [0, 1, 5])
@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_model_misses_have_reasons(gaps, rot, mode, p):
    """The miss conditions for the reference alone (a failure is a bug of the model)."""
    _, _, _, names = _composed(gaps, rot)
    bad = []
    for i, ((what, _, _, _), _, _) in enumerate(_outcomes(gaps, rot, mode, p)):
        content = names[i][0]
        assert content in DISTINCT | ZEROS | REPEATS
        if not what.startswith("miss"):
            continue
        ok = content in REPEATS or (content in ZEROS and what == "miss:zero" and mode == "sorted_lower")
        if what == "miss:fail":
            ok = content in REPEATS
        if not ok:
            bad.append(f"{names[i]} rot={rot} mode={mode} p={p}: {what}")
    assert not bad, "\n".join(bad[:8])


# ---- the checker bites -------------------------------------------------------------------

def _mut_below_up(x, gaps, h, row, kc):
    lo, hi, below, n, cnt, flags = wm.unpack_header(h)
    return wm.pack_header(lo, hi, below + 1, n, cnt, flags), row


def _mut_below_down(x, gaps, h, row, kc):
    lo, hi, below, n, cnt, flags = wm.unpack_header(h)
    return wm.pack_header(lo, hi, below - 1, n, cnt, flags), row


def _mut_n_padded(x, gaps, h, row, kc):
    """n counting the NaN padding of the partial chunk."""
    lo, hi, below, n, cnt, flags = wm.unpack_header(h)
    pad = -x.size % wm.CHUNK
    return (wm.pack_header(lo, hi, below, n + pad, cnt, flags), row) if pad else None


def _mut_key_dropped(x, gaps, h, row, kc):
    cnt = wm.unpack_header(h)[4]
    if cnt == 0:
        return None
    row = row.copy()
    row[cnt - 1] = wm.SENTINEL
    return h, row


def _mut_key_duplicated(x, gaps, h, row, kc):
    cnt = wm.unpack_header(h)[4]
    if cnt < 2 or row[cnt - 1] == row[cnt - 2]:
        return None
    row = row.copy()
    row[cnt - 1] = row[cnt - 2]
    return h, row


def _mut_lo_nudged(x, gaps, h, row, kc):
    """lo moved to the next key of the slice; below and cnt stay."""
    lo, hi, below, n, cnt, flags = wm.unpack_header(h)
    keys = wm.sorted_keys(x)
    above = keys[(keys > np.uint64(lo)) & (keys <= np.uint64(hi))]
    if above.size == 0 or below + cnt != np.searchsorted(keys, np.uint64(hi), "right") or not (keys == np.uint64(lo)).any():
        return None
    return wm.pack_header(above[0], hi, below, n, cnt, flags), row


def _mut_key_past_cnt(x, gaps, h, row, kc):
    cnt = wm.unpack_header(h)[4]
    if cnt >= kc:
        return None
    row = row.copy()
    row[cnt] = wm.okey(np.array([0.25])).view(np.int64)[0]
    return h, row


MUTATIONS = {"below+1": _mut_below_up, "below-1": _mut_below_down, "n_padded": _mut_n_padded,
             "key_dropped": _mut_key_dropped, "key_duplicated": _mut_key_duplicated, "lo_nudged": _mut_lo_nudged,
             "key_past_cnt": _mut_key_past_cnt}


def _slices(gaps):
    """Every segment of slice lattice 0 with its p50 export at ext = 2 maxlen."""
    vals, offs, index = _lattices(gaps)[0]
    kc, exp = _exports(gaps, "50", (W - 1) * MAXLEN)
    hdr, rows = exp[0]
    names = _lattice.names(offs, index)
    for s in range(offs.size - 1):
        yield names[s], vals[offs[s]:offs[s + 1]], hdr[s], rows[s], kc


@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_numpy_export_keeps_the_promise(gaps):
    bad = [(name, v) for name, x, h, row, kc in _slices(gaps) if (v := wm.check_header(x, gaps, h, row, kc))]
    assert not bad, bad[:4]
    flags = {name: wm.unpack_header(h)[5] for name, x, h, row, kc in _slices(gaps)}
    assert any(f & wm.WIN_FAIL for f in flags.values())  # the long const slices
    assert all(not f & wm.WIN_FAIL for name, f in flags.items() if name[0] in DISTINCT)
    assert {name[0] for name, f in flags.items() if f & wm.FLAG_NAN} == (set() if gaps else {"nan0", "nanL", "nanmid"})


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_checker_reports_mutation(gaps, mutation):
    """Every slice the mutation applies to (a window with counts: no FAIL, no compact NaN) is
    reported, and it applies to slices of every shape: shorter than a chunk and longer, with a
    narrowed window and with the whole one."""
    applied, missed = [], []
    for name, x, h, row, kc in _slices(gaps):
        flags = wm.unpack_header(h)[5]
        if flags & (wm.WIN_FAIL | wm.FLAG_NAN):
            continue
        mutated = MUTATIONS[mutation](x, gaps, h, row, kc)
        if mutated is None:
            continue
        applied.append(name)
        if not wm.check_header(x, gaps, mutated[0], mutated[1], kc):
            missed.append(name)
    assert not missed, (mutation, missed[:8])
    assert any(n < wm.CHUNK for _, n, _ in applied) and any(n > 2 * wm.CHUNK for _, n, _ in applied), mutation
    assert len(applied) >= 50, (mutation, len(applied))


@pytest.mark.parametrize("gaps", [False, True], ids=["compact", "gapped"])
def test_checker_reports_point_rows(gaps):
    """A POINT header of a const slice: lo == hi its key, cnt copies, the row untouched.  A key in
    the row, or a window of two keys, is reported."""
    seen = 0
    for name, x, h, row, kc in _slices(gaps):
        keys = wm.sorted_keys(x)
        if name[0] != "const" or keys.size == 0:
            continue
        seen += 1
        point = wm.pack_header(keys[0], keys[0], 0, keys.size, keys.size, wm.WIN_POINT)
        blank = np.full(kc, wm.SENTINEL, dtype=np.int64)
        assert wm.check_header(x, gaps, point, blank, kc) == [], name
        written = blank.copy()
        written[0] = keys[0].view(np.int64)
        assert wm.check_header(x, gaps, point, written, kc), name
        wide = wm.pack_header(keys[0], int(keys[0]) + 1, 0, keys.size, keys.size, wm.WIN_POINT)
        assert wm.check_header(x, gaps, wide, blank, kc), name
        short = wm.pack_header(keys[0], keys[0], 0, keys.size, keys.size - 1, wm.WIN_POINT)
        assert wm.check_header(x, gaps, short, blank, kc), name
    assert seen >= 40

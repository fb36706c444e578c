"""The streaming layout of a segment (krr_amd/csrc/krr_geom.h: seg_geom, SegGeom's position
functions, SegCursor), compiled for the host (tests/native/geom_check.cpp) and checked on the CPU
against a model written here from the contract's words — it never calls the header:

  a segment is L slots; an odd start leaves slot 0 in front of the 16-byte aligned body, an odd
  end leaves slot L - 1 behind it; the body goes out two slots per lane, 64 lanes per row, 8 rows
  per chunk, in slot order; the last chunk is partial when body slots remain or there is a head or
  a tail, and lane 63 of its last row holds (slot 0, slot L - 1) for them; the rest is padding.

Every start parity (beg 0..3) and every L in 0..2200: none, one and two full chunks of 1,024
slots, with and without a partial one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import kll_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LANES, ROWS, CHUNK = 64, 8, 1024  # lanes per row, rows per chunk, slots per chunk
EDGE_X = CHUNK - 2                 # lane 63 of row 7, .x; .y follows
BEGS, LENGTHS = range(4), range(2201)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gc") / "libgeomcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "krr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "geom_check.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    L.geom_check_geom.argtypes = [i64, i64, vp]
    L.geom_check_geom.restype = None
    L.geom_check_layout.argtypes = [i64, i64, vp, i64]
    L.geom_check_layout.restype = i64
    L.geom_check_cursor.argtypes = [i64, i64, ctypes.c_int, vp, vp, vp]
    L.geom_check_cursor.restype = None
    return L


def model(beg: int, L: int) -> np.ndarray:
    """What every (chunk, row, lane, half) holds, [chunks, 1024] in that order: a slot or -1."""
    head = L > 0 and beg % 2 == 1
    body = L - (1 if head else 0)          # slots from the first even address on
    tail = body % 2 == 1                   # ... the last of which has no partner
    units = body // 2
    full, rem = divmod(units, ROWS * LANES)
    chunks = full + (1 if rem or head or tail else 0)
    lay = np.full((chunks, CHUNK), -1, dtype=np.int64)
    first = 1 if head else 0
    lay.reshape(-1)[: 2 * units] = np.arange(first, first + 2 * units)  # chunk, row, lane, half: slot order
    if head:
        lay[-1, EDGE_X] = 0
    if tail:
        lay[-1, EDGE_X + 1] = L - 1
    return lay


def header_layout(lib, beg: int, L: int, buf: np.ndarray):
    nch = lib.geom_check_layout(beg, beg + L, buf.ctypes.data, buf.size)
    assert nch >= 0
    return buf[: nch * CHUNK].reshape(nch, CHUNK)


def test_layout_properties_and_model(lib):
    buf = np.empty(4 * CHUNK, dtype=np.int64)
    g = np.empty(12, dtype=np.int64)
    for beg in BEGS:
        for L in LENGTHS:
            end = beg + L
            lay = header_layout(lib, beg, L, buf)
            lib.geom_check_geom(beg, end, g.ctypes.data)
            partial, nch, padding = bool(g[9]), int(g[10]), int(g[11])
            where = (beg, L)
            flat = lay.reshape(-1)
            # every slot of [0, L) is held exactly once
            assert np.array_equal(np.sort(flat[flat >= 0]), np.arange(L)), where
            # body slots ascend in (chunk, row, lane, half) order
            body = flat.copy()
            if partial:
                body[-2:] = -1  # the edge unit
            assert np.all(np.diff(body[body >= 0]) > 0), where
            # slot 0 / slot L - 1 sit in the edge unit exactly when beg / end is odd
            assert (partial and lay[-1, EDGE_X] == 0) == (L > 0 and beg % 2 == 1), where
            assert (partial and lay[-1, EDGE_X + 1] == L - 1) == (L > 0 and end % 2 == 1), where
            if partial:
                assert lay[-1, EDGE_X] in (0, -1) and lay[-1, EDGE_X + 1] in (L - 1, -1), where
            # everything else is padding, and padding() counts it
            assert int((flat < 0).sum()) == padding == nch * CHUNK - L, where
            # the model, position by position, and its chunk count
            want = model(beg, L)
            assert nch == want.shape[0] == lay.shape[0], where
            assert np.array_equal(lay, want), where


def test_nch_against_the_kll_oracle(lib):
    """oracle/kll_ref.chunks restates the skeleton for the KLL rows: as many chunks, holding the same
    slots (values = slot indices, NaN = padding)."""
    buf = np.empty(4 * CHUNK, dtype=np.int64)
    for beg in BEGS:
        vals = np.arange(-beg, 2201, dtype=np.float64)  # vals[beg + i] = i
        for L in LENGTHS:
            lay = header_layout(lib, beg, L, buf)
            ref = list(kll_ref.chunks(vals, beg, beg + L))
            assert len(ref) == lay.shape[0], (beg, L)
            if ref:
                got = np.where(lay < 0, np.nan, lay.astype(np.float64))
                assert np.array_equal(got, np.stack(ref), equal_nan=True), (beg, L)


def test_seg_geom_fields(lib):
    g = np.empty(12, dtype=np.int64)
    for beg in BEGS:
        for L in LENGTHS:
            end = beg + L
            lib.geom_check_geom(beg, end, g.ctypes.data)
            a0, a1, s0, i0, nunits, nfull, rem, head, tail, partial, nch, padding = (int(x) for x in g)
            where = (beg, L)
            assert head == (L > 0 and beg % 2 == 1) and tail == (L > 0 and end % 2 == 1), where
            assert a0 == beg + head and a1 == end - tail and s0 == head, where
            assert a0 % 2 == 0 or a0 == a1, where  # 16-byte aligned unless the body is empty
            assert i0 * 2 == a0 - a0 % 2 and nunits * 2 == a1 - a0, where
            assert nunits == nfull * ROWS * LANES + rem and 0 <= rem < ROWS * LANES, where
            assert partial == (rem > 0 or head or tail) and nch == nfull + partial, where
            assert padding == nch * CHUNK - L, where


def test_cursor_follows_the_layout(lib):
    """A SegCursor counts its chunks into the same positions: row_base(u) is the slot lane 0 holds in
    row u, edge_row / edge name the partial chunk's last row and its lane 63, nowhere else."""
    buf = np.empty(4 * CHUNK, dtype=np.int64)
    rb = np.empty(4 * ROWS, dtype=np.int64)
    er, ed = np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)
    g = np.empty(12, dtype=np.int64)
    for beg in BEGS:
        for L in (0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 2200):
            lay = header_layout(lib, beg, L, buf).reshape(-1, ROWS, LANES, 2)
            lib.geom_check_geom(beg, beg + L, g.ctypes.data)
            partial, nch = bool(g[9]), int(g[10])
            for lane in (0, 1, 62, 63):
                lib.geom_check_cursor(beg, beg + L, lane, rb.ctypes.data, er.ctypes.data, ed.ctypes.data)
                for ci in range(nch):
                    last = partial and ci == nch - 1
                    assert er[ci] == (1 << (ROWS - 1) if last else 0), (beg, L, lane, ci)
                    assert ed[ci] == (1 << (ROWS - 1) if last and lane == LANES - 1 else 0), (beg, L, lane, ci)
                    for u in range(ROWS):
                        held = lay[ci, u, lane]
                        if held[0] >= 0 and not (ed[ci] >> u) & 1:
                            assert held[0] == rb[ci * ROWS + u] + 2 * lane and held[1] == held[0] + 1, (beg, L, lane, ci, u)

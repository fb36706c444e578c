"""What tests/_lattice.py covers, pinned on the CPU: tests/test_gpu_lattice.py runs the kernels over
that lattice, and would lose coverage silently if someone trimmed its length list.

The geometry model restates krr_amd/csrc/krr_geom.h seg_geom from the contract's words (the header
itself is checked against such a model in tests/test_segment_geom.py): an odd start leaves a head
slot, an odd end a tail slot, the rest is double2 units, 512 of them to a full chunk.

The expected classes are written out, not derived from the builder.  A class is (head, tail, full
chunks, units in the partial chunk).  Of the partial-chunk sizes 0, 1, 63, 64, 65 and 511 units
the length list reaches all but 65 (130..133 slots are not in it); it reaches 8, 31 and 32 as well.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lattice  # noqa: E402

UNITS = 512  # double2 units per chunk


def geom(beg: int, n: int):
    """(head, tail, full chunks, units of the partial chunk) of values[beg, beg + n)."""
    head = 1 if n > 0 and beg % 2 == 1 else 0
    tail = 1 if n - head > 0 and (beg + n) % 2 == 1 else 0
    units = (n - head - tail) // 2
    return head, tail, units // UNITS, units % UNITS


# every length of _lattice.LENGTHS at both start parities, by hand
FULL = {
    (0, 0, 0, 0),                                              # 0
    (0, 1, 0, 0), (1, 0, 0, 0),                                # 1
    (0, 0, 0, 1), (1, 1, 0, 0),                                # 2
    (0, 1, 0, 1), (1, 0, 0, 1),                                # 3
    (0, 1, 0, 31), (1, 0, 0, 31),                              # 63
    (0, 0, 0, 32), (1, 1, 0, 31),                              # 64
    (0, 1, 0, 32), (1, 0, 0, 32),                              # 65
    (0, 1, 0, 63), (1, 0, 0, 63),                              # 127
    (0, 0, 0, 64), (1, 1, 0, 63),                              # 128
    (0, 1, 0, 64), (1, 0, 0, 64),                              # 129
    (0, 1, 0, 511), (1, 0, 0, 511),                            # 1023
    (0, 0, 1, 0), (1, 1, 0, 511),                              # 1024
    (0, 1, 1, 0), (1, 0, 1, 0),                                # 1025
    (0, 0, 1, 1), (1, 1, 1, 0),                                # 1026
    (0, 1, 1, 511), (1, 0, 1, 511),                            # 2047
    (0, 0, 2, 0), (1, 1, 1, 511),                              # 2048
    (0, 1, 2, 0), (1, 0, 2, 0),                                # 2049
    (0, 1, 2, 511), (1, 0, 2, 511),                            # 3071
    (0, 0, 3, 0), (1, 1, 2, 511),                              # 3072
    (0, 1, 3, 0), (1, 0, 3, 0),                                # 3073
    (0, 1, 3, 511), (1, 0, 3, 511),                            # 4095
    (0, 1, 4, 0), (1, 0, 4, 0),                                # 4097
    (0, 1, 5, 8), (1, 0, 5, 8),                                # 5 * 1024 + 17
    (0, 0, 6, 0), (1, 1, 5, 511),                              # 6 * 1024
    (0, 1, 7, 0), (1, 0, 7, 0),                                # 7 * 1024 + 1
}
# the variants' lengths: up to 2,049 slots, and 3,073
SHORT = {c for c in FULL if c[2] <= 1 or c in {(0, 0, 2, 0), (0, 1, 2, 0), (1, 0, 2, 0), (0, 1, 3, 0), (1, 0, 3, 0)}}
# classes only lengths 0, 1 and 2 reach: a content that needs more slots cannot have them
ONLY_LEN = {0: {(0, 0, 0, 0)}, 1: {(0, 1, 0, 0), (1, 0, 0, 0)}, 2: {(0, 0, 0, 1), (1, 1, 0, 0)}}
MIN_LEN = {"distinct": 0, "ties": 1, "const": 1, "edge_hi": 2, "edge_lo": 2, "zeros": 2, "zeros_swap": 2,
           "absent0": 1, "absentL": 1, "absent0L": 2, "absent_all": 1, "nan0": 1, "nanL": 1, "nanmid": 3}
FULL_CONTENTS = {"distinct", "ties", "edge_hi", "edge_lo", "zeros", "const"}
CONTENTS = {False: FULL_CONTENTS | {"zeros_swap", "nan0", "nanL", "nanmid"},
            True: FULL_CONTENTS | {"zeros_swap", "absent0", "absentL", "absent0L", "absent_all"}}


def expected(content):
    want = set(FULL if content in FULL_CONTENTS else SHORT)
    for n in range(MIN_LEN[content]):
        want -= ONLY_LEN[n]
    return want


@pytest.fixture(scope="module", params=[(False, 0), (True, 0), (False, 1), (True, 1)],
                ids=["compact", "gapped", "compact_shifted", "gapped_shifted"])
def lattice(request):
    gaps, shift = request.param
    vals, offs, index = _lattice.build(gaps, seed=7 + shift, shift=shift)
    return gaps, shift, vals, offs, index


def test_expected_classes_span_the_loop_forms():
    """The written-out set itself: both head and both tail forms, 0..7 full chunks, the
    partial-chunk sizes of the module docstring; all four head/tail forms with 0, 1 and 2 full
    chunks, and a tail without a head on exactly three."""
    assert {c[0] for c in FULL} == {0, 1} and {c[1] for c in FULL} == {0, 1}
    assert {c[2] for c in FULL} == set(range(8))
    assert {c[3] for c in FULL} == {0, 1, 8, 31, 32, 63, 64, 511}
    for nfull in (0, 1):
        assert {(h, t) for h, t, f, _ in FULL if f == nfull} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(h, t) for h, t, f, _ in FULL if f == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (0, 1, 3, 0) in FULL and (1, 0, 3, 0) in FULL and (0, 0, 3, 0) in FULL
    # chunks streamed, the partial one included: each residue of the period-3 loop and of the
    # depth-2 ring twice (1..6), and 8
    chunks = {f + (1 if r or h or t else 0) for h, t, f, r in FULL}
    assert chunks == {0, 1, 2, 3, 4, 5, 6, 8}


def test_every_content_has_every_class(lattice):
    gaps, _, _, offs, index = lattice
    assert {c for c, _, _ in index} == CONTENTS[gaps]
    got = {}
    for (content, n, parity), s in index.items():
        assert offs[s + 1] - offs[s] == n, (content, n, parity)
        got.setdefault(content, set()).add(geom(int(offs[s]), n))
    for content in CONTENTS[gaps]:
        assert got[content] == expected(content), (content, got[content] ^ expected(content))


def test_both_parities_of_every_case(lattice):
    _, _, _, offs, index = lattice
    for (content, n, parity), s in index.items():
        assert offs[s] % 2 == parity, (content, n, parity)
        assert (content, n, 1 - parity) in index
    lengths = {}
    for content, n, _ in index:
        lengths.setdefault(content, set()).add(n)
    for content, have in lengths.items():
        base = _lattice.LENGTHS if content in FULL_CONTENTS else _lattice.SHORT_LENGTHS
        assert have == {n for n in base if n >= MIN_LEN[content]}, content
    assert _lattice.LENGTHS == [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1026, 2047, 2048, 2049,
                                3071, 3072, 3073, 4095, 4097, 5137, 6144, 7169]


def test_fillers_are_poison_never_nan(lattice):
    """One filler before every case and one after the last; +1e300 and -1e300 in turn; case values
    lie strictly between.  So each case has +1e300 on one side and -1e300 on the other, and the
    shifted lattice has them the other way round."""
    _, shift, vals, offs, index = lattice
    S = offs.size - 1
    case = np.zeros(S, dtype=bool)
    case[list(index.values())] = True
    assert S == 2 * len(index) + 1 and not case[0::2].any() and case[1::2].all()
    for f, s in enumerate(range(0, S, 2)):
        x = vals[offs[s]:offs[s + 1]]
        assert x.size in (1 + 2 * shift, 2 + 2 * shift)
        assert not np.isnan(x).any() and (x == (_lattice.HI if (f + shift) % 2 == 0 else _lattice.LO)).all()
    for s in index.values():
        x = vals[offs[s]:offs[s + 1]]
        assert not (np.abs(x[~np.isnan(x)]) >= 1e299).any()
    assert vals.size < 1_000_000


def test_contents_are_what_they_say(lattice):
    gaps, _, vals, offs, index = lattice
    for (content, n, parity), s in index.items():
        x = vals[offs[s]:offs[s + 1]]
        pres = x[~np.isnan(x)]
        where = (content, n, parity)
        if content in ("edge_hi", "edge_lo"):
            sign = 1.0 if content == "edge_hi" else -1.0
            order = np.sort(sign * pres)  # ascending: the two extreme values come last
            assert np.array_equal(order[-2:], np.sort(sign * np.array([x[0], x[-1]]))), where
            assert order[-2] != order[-1] and (order.size == 2 or order[-3] < order[-2]), where
        elif content in ("zeros", "zeros_swap"):
            assert (pres <= 0).all() and np.flatnonzero(x == 0).tolist() == [0, n - 1], where
            assert np.signbit(x[0]) == (content == "zeros_swap") and np.signbit(x[-1]) == (content == "zeros"), where
        elif content == "const":
            assert np.unique(pres).size == 1, where
        elif content == "ties":
            assert set(np.unique(pres).tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}, where
        elif content == "absent_all":
            assert pres.size == 0, where
        if content in ("absent0", "absent0L", "nan0"):
            assert np.isnan(x[0]), where
        if content in ("absentL", "absent0L", "nanL"):
            assert np.isnan(x[-1]), where
        if content in ("nan0", "nanL", "nanmid"):
            assert np.isnan(x).sum() == 1, where
        if content == "nanmid":
            assert not np.isnan(x[0]) and not np.isnan(x[-1]), where
        if gaps and content in FULL_CONTENTS | {"zeros_swap"} and n:
            assert not np.isnan(x[0]) and not np.isnan(x[-1]), where
        if not gaps and content in FULL_CONTENTS | {"zeros_swap"}:
            assert pres.size == n, where
    if gaps:  # a fifth of the slots of the long cases are absent
        s = index[("distinct", 7169, 0)]
        share = np.isnan(vals[offs[s]:offs[s + 1]]).mean()
        assert 0.17 < share < 0.23


def test_two_lattices_pair_up(lattice):
    """A lattice and its shifted twin have the same segments in the same order (a fused launch
    takes one CPU and one memory segment per object) at different offsets."""
    gaps, shift, vals, offs, index = lattice
    if shift:
        return
    _, offs1, index1 = _lattice.build(gaps, seed=99, shift=1)
    assert index1 == index and offs1.size == offs.size
    assert np.array_equal(np.diff(offs1)[1::2], np.diff(offs)[1::2])
    assert (offs1[1:] != offs[1:]).all()
    assert _lattice.names(offs, index)[0][0] == "filler" and _lattice.names(offs, index)[1] == ("distinct", 0, 0)

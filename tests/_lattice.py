"""The edge-geometry lattice: one series that holds, for every content, every length at which
the streaming skeleton (krr_amd/csrc/krr_geom.h, stream_segment) changes shape, each at an even
and at an odd start offset.  Plain numpy, no GPU; tests/test_lattice_layout.py pins what it
covers, tests/test_gpu_lattice.py runs the kernels over it.

A chunk is 1,024 slots.  An odd start leaves slot 0 (head) and an odd end slot L - 1 (tail)
outside the 16-byte aligned body; both travel in the last unit of the padded partial chunk.  The
lengths are the smallest around 0..3 slots, one row (128 slots), and 1..7 chunks: every residue of
the period-3 loop and of the depth-2 ring twice, with and without a partial chunk.

Every case is preceded by exactly one filler segment (and the last one followed by one), so the
segment count does not depend on the arguments: two lattices pair up in a fused launch.  A filler
is never NaN: fillers alternate between +1e300 and -1e300, above and below every case value, so a
kernel that reads one slot past either end of a case changes that case's max, a low percentile or
its present count.  Fillers are segments like any other (1..4 slots) and are compared as well.
"""
import numpy as np

CHUNK = 1024
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129,
           1023, 1024, 1025, 1026, 2047, 2048, 2049,
           3071, 3072, 3073, 4095, 4097,
           5 * 1024 + 17, 6 * 1024, 7 * 1024 + 1]
# the variants of a content (absent edge slots, a NaN sample, the swapped zeros): up to two chunks
# with every head / tail form, and one three-chunk length (period 3 of the multi-site loop)
SHORT_LENGTHS = [n for n in LENGTHS if n <= 2049] + [3073]
HI, LO = 1e300, -1e300

# content -> (smallest length it can be built at, its lengths)
FULL_CONTENTS = {"distinct": 0, "ties": 1, "edge_hi": 2, "edge_lo": 2, "zeros": 2, "const": 1}
SHORT_CONTENTS_ANY = {"zeros_swap": 2}
SHORT_CONTENTS_GAPS = {"absent0": 1, "absentL": 1, "absent0L": 2, "absent_all": 1}
SHORT_CONTENTS_COMPACT = {"nan0": 1, "nanL": 1, "nanmid": 3}


def contents(gaps: bool) -> dict:
    """content -> the lengths it appears at."""
    out = {c: [n for n in LENGTHS if n >= lo] for c, lo in FULL_CONTENTS.items()}
    short = dict(SHORT_CONTENTS_ANY)
    short.update(SHORT_CONTENTS_GAPS if gaps else SHORT_CONTENTS_COMPACT)
    out.update({c: [n for n in SHORT_LENGTHS if n >= lo] for c, lo in short.items()})
    return out


def _case(content: str, n: int, gaps: bool, rng) -> np.ndarray:
    x = rng.normal(size=n)
    if content == "ties":
        x = rng.integers(-2, 3, size=n) * 0.5
        x[(x == 0) & (rng.random(n) < 0.5)] = -0.0
    elif content in ("edge_hi", "edge_lo"):
        sign = 1.0 if content == "edge_hi" else -1.0
        first, last = (10.0, 9.0) if rng.random() < 0.5 else (9.0, 10.0)
        x[0], x[n - 1] = sign * first, sign * last
    elif content in ("zeros", "zeros_swap"):
        x = -(np.abs(x) + 1e-3)
        x[0], x[n - 1] = (0.0, -0.0) if content == "zeros" else (-0.0, 0.0)
    elif content == "const":
        x = np.full(n, float(rng.normal()))
    if gaps and n:
        holes = rng.random(n) < 0.2
        holes[0] = holes[n - 1] = False  # the edge slots stay: their absence has contents of its own
        x[holes] = np.nan
    if content in ("absent0", "absent0L", "nan0"):
        x[0] = np.nan
    if content in ("absentL", "absent0L", "nanL"):
        x[n - 1] = np.nan
    if content == "absent_all":
        x[:] = np.nan
    if content == "nanmid":
        x[min(max(n // 2 + 37, 1), n - 2)] = np.nan  # inside a chunk, neither edge slot
    return x


def build(gaps: bool, seed, shift: int = 0):
    """values, offsets, index: index[(content, length, parity)] is the segment whose start offset
    has that parity.  gaps: a fifth of every case's slots are NaN (absent), plus the absent-edge
    contents; else a few contents hold one NaN sample.  shift = 1: every filler is two slots
    longer and the fillers' signs are swapped, so the offsets differ from shift = 0 at every
    segment while the segment numbers and parities stay."""
    rng = np.random.default_rng(seed)
    by_content = contents(gaps)
    segs, index, pos, fillers = [], {}, 0, 0

    def filler(parity):
        nonlocal pos, fillers
        n = (1 if (pos + 1) % 2 == parity else 2) + 2 * shift
        segs.append(np.full(n, HI if (fillers + shift) % 2 == 0 else LO))
        pos += n
        fillers += 1

    for n in LENGTHS:
        for content, lengths in by_content.items():
            if n not in lengths:
                continue
            for parity in (0, 1):
                filler(parity)
                index[(content, n, parity)] = len(segs)
                x = _case(content, n, gaps, rng)
                assert not (np.abs(x) >= HI).any()
                segs.append(x)
                pos += n
    filler(0)
    offsets = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    return np.concatenate(segs), offsets, index


def names(offsets: np.ndarray, index: dict) -> list:
    """Segment number -> (content, length, parity), the fillers included."""
    out = [("filler", int(offsets[s + 1] - offsets[s]), int(offsets[s] % 2)) for s in range(offsets.size - 1)]
    for key, s in index.items():
        out[s] = key
    return out

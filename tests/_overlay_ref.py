"""krr_pods_overlay restated in plain Python, for the tests of the kernel and of the layers above
it.  Nothing here comes from the code under test.

Object g owns pod segments groups[g] .. groups[g+1] of a pod series; pod p has Lp slots and the
object Lg = max Lp (0 without pods).  Pod slot i falls on object slot i ("start") or on
i + (Lg - Lp) ("end").  Per object slot, P = the pods that reach it, in pod order, with ``gaps``
only those whose sample there is not NaN:

    active = |P|
    sum    = ((+0.0 + x1) + x2) + ... in pod order, Python floats (IEEE double, one rounding per
             add); a NaN sum is the quiet NaN 0x7FF8000000000000
    max / min = the FIRST extremal sample in pod order under float comparison, its own bits (an
             update only on a strict > / <); the quiet NaN when P is empty

and a NaN sample that reaches a slot in the compact layout counts in active and makes the slot's
sum, max and min the quiet NaN (the object gets NAN).  Every expectation is bit-exact: there is one
order of additions, so there is no tolerance."""
import struct

import numpy as np

EMPTY, NAN, CAPACITY = 4, 1, 2
START, END = 0, 1
QNAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


def slot_one(xs: list, gaps: bool) -> tuple:
    """(active, sum, max, min, nan) of one object slot from the samples of the pods that reach it,
    in pod order (Python floats)."""
    active, total, hi, lo, bad = 0, 0.0, None, None, False
    for v in xs:
        if v != v:
            if gaps:
                continue
            bad = True
        active += 1
        total = total + v
        if hi is None or v > hi:
            hi = v
        if lo is None or v < lo:
            lo = v
    if bad:
        return active, QNAN, QNAN, QNAN, True
    if total != total:
        total = QNAN
    if hi is None:
        hi = lo = QNAN
    return active, total, hi, lo, False


def overlay_one(pods: list, align: int, gaps: bool) -> list:
    """The slots of one object from the list of its pods' sample arrays, oldest slot first."""
    pods = [np.asarray(p, dtype=np.float64).tolist() for p in pods]
    Lg = max((len(p) for p in pods), default=0)
    out = []
    for j in range(Lg):
        xs = []
        for p in pods:
            i = j - (Lg - len(p) if align == END else 0)
            if 0 <= i < len(p):
                xs.append(p[i])
        out.append(slot_one(xs, gaps))
    return out


def np_overlay(vals, pod_offs, groups, align: int, gaps: bool = False, out_offsets=None) -> dict:
    """The whole entry point as numpy arrays: ``offsets`` (the exclusive cumulative sum of Lg, or
    the caller's), ``slots`` (Lg) and ``pods`` [S], flat ``active`` (uint32) / ``sum`` / ``max`` /
    ``min``, ``written`` (False where no slot is written), and ``count`` / ``flags`` [S] by the
    header's rules (CAPACITY: the caller's span is too small, no slot of that object is written)."""
    vals = np.asarray(vals, dtype=np.float64)
    pod_offs, groups = np.asarray(pod_offs, dtype=np.int64), np.asarray(groups, dtype=np.int64)
    S = groups.size - 1
    lens = np.diff(pod_offs)
    Lg = np.array([lens[groups[g]:groups[g + 1]].max(initial=0) for g in range(S)], dtype=np.int64)
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(Lg)]).astype(np.int64)
    out_offsets = np.asarray(out_offsets, dtype=np.int64)
    n = int(out_offsets.max()) if out_offsets.size else 0
    out = dict(offsets=out_offsets, slots=Lg, pods=np.diff(groups), active=np.zeros(n, np.uint32), sum=np.zeros(n),
               max=np.full(n, QNAN), min=np.full(n, QNAN), written=np.zeros(n, bool),
               count=np.zeros(S, np.int64), flags=np.zeros(S, np.uint32))
    for g in range(S):
        pods = [vals[pod_offs[p]:pod_offs[p + 1]] for p in range(groups[g], groups[g + 1])]
        slots = overlay_one(pods, align, gaps)
        out["count"][g] = sum(e[0] for e in slots)
        if out["count"][g] == 0:
            out["flags"][g] = EMPTY
        elif any(e[4] for e in slots):
            out["flags"][g] = NAN
        if out_offsets[g + 1] - out_offsets[g] < Lg[g]:
            out["flags"][g] |= CAPACITY
            continue
        for j, e in enumerate(slots):
            i = int(out_offsets[g]) + j
            out["active"][i], out["sum"][i], out["max"][i], out["min"][i] = e[0], e[1], e[2], e[3]
            out["written"][i] = True
    return out


def brute_slot(pods: list, j: int, align: int) -> list:
    """The (pod, pod slot) pairs that fall on object slot j, found by walking every pod slot:
    "end" counts slots back from each pod's last."""
    Lg = max((len(p) for p in pods), default=0)
    hits = []
    for k, p in enumerate(pods):
        for i in range(len(p)):
            at = i if align == START else (Lg - 1) - (len(p) - 1 - i)
            if at == j:
                hits.append((k, i))
    return hits

"""What tests/_json_numbers.py and tests/_json_lattice.py cover, pinned on the CPU from the computed
positions: tests/test_gpu_json_lattice.py runs both on the device and would lose coverage silently
if someone trimmed a list.  Every lattice and corpus body is also parsed here by the g++ build of
the device logic (tests/native/json_check.cpp) and by the host packer, both against float()'s bits,
so a failure of the GPU test isolates the device build or the wave geometry.
"""
import os
import re
import sys
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _json_lattice as L  # noqa: E402
import _json_numbers as N  # noqa: E402
from test_json_device_logic import JSON_DROPPED, JSON_OK, _check_body, _grouped, lib  # noqa: E402,F401

from krr_amd.core.prom_native import pack_query_range_bodies  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Obj:
    def __init__(self, ns, c, pods):
        self.namespace, self.container, self.pods = ns, c, pods


def make_plan():
    """One object per grouped lattice series (series 0: the filler), a few bodies."""
    from krr_amd.core.fleet_query import FleetQueryPlan

    n = len(L.grouped_specs()) + 1
    plan = FleetQueryPlan([Obj("ns", "app", [L.pod_name(k)]) for k in range(n)], max_query_chars=1200)
    assert len(plan.groups) > 2 and [p for g in plan.groups for p in g.pods] == [L.pod_name(k) for k in range(n)]
    return plan


# ---- the number corpus ----

@pytest.fixture(scope="module")
def corpus():
    return {"shortest": N.shortest_repr_values(), "midpoints": N.midpoint_cases(),
            "constructed": N.constructed_values()}


def test_corpus_groups_are_accepted(corpus):
    assert len(corpus["shortest"]) == 50013 and len(corpus["midpoints"]) > 80000 and len(corpus["constructed"]) > 900
    left_out = [s for g in corpus.values() for s in g if not N.acceptable(s)]
    assert len(left_out) == 0, left_out[:5]
    assert not [s for s in N.TIMESTAMPS if not N.acceptable(s, value_form=False)]
    assert len(N.value_corpus()) == sum(len(g) for g in corpus.values())
    for s in ("0", "-0", "0.5", "1.7e9", "1700000000.781"):
        assert s in N.TIMESTAMPS
    assert sum(len(re.sub(r"[-.]|e.*", "", s).strip("0")) == 19 for s in N.TIMESTAMPS) >= 5
    for s in N.TIMESTAMPS:  # inside the JSON grammar
        assert not s.startswith("+") and "N" not in s and "I" not in s and not re.match(r"-?0[0-9]", s), s


def test_handover_strings_are_not_accepted():
    assert not [s for s in N.HANDOVER if N.acceptable(s)]
    assert set(N.OTHER_SPELLINGS) < set(N.HANDOVER)
    twenty = [s for s in N.HANDOVER if re.fullmatch(r"[0-9]{20}", s) and s[19] != "0"]
    seven = [s for s in N.HANDOVER if re.fullmatch(r"[0-9]e-?[0-9]{7}", s)]
    assert twenty and seven


def test_second_multiply_strings():
    """At least 200 strings, spread over q in [-342, 308], whose first product leaves the rounding
    bits unsure — by the table of krr_pow5.inc itself."""
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", open(
        os.path.join(ROOT, "krr_amd", "csrc", "krr_pow5.inc")).read())]
    assert len(words) == 2 * 651
    assert all(N.pow5_high(q) == words[2 * (q + 342)] for q in range(-342, 309))
    got = N.second_multiply_strings()
    qs = []
    for s in got:
        w, q = s.split("e")
        assert len(w) <= 19 and N.first_product_unsure(int(w), int(q)), s
        qs.append(int(q))
    assert len(got) >= 200 and qs == list(range(-342, 309))
    ts = [s for s in N.TIMESTAMPS if re.fullmatch(r"[0-9]+e-?[0-9]+", s) and
          N.first_product_unsure(int(s.split("e")[0]), int(s.split("e")[1]))]
    assert len(ts) >= 20


def test_halfway_cases_are_halfway():
    """For every q in [-4, 23] a value exactly between two doubles whose lower neighbour is odd, and
    one where it is even (5^23 is the only 54-bit odd multiple of 5^23: even only)."""
    seen = set()
    for q, odd, s in N.halfway_cases():
        v = Fraction(Decimal(s))
        x = float(s)
        lo = x if Fraction(x) < v else float(np.nextafter(x, 0.0))
        hi = float(np.nextafter(lo, np.inf))
        assert Fraction(lo) + Fraction(hi) == 2 * v, s
        assert (N.bits(lo) & 1) == (1 if odd else 0), s
        assert N.bits(x) & 1 == 0  # ties to even
        digits = re.sub(r"e.*", "", s).replace(".", "").strip("0")
        assert len(digits) <= 19
        seen.add((q, odd))
    assert seen == {(q, odd) for q in range(-4, 24) for odd in (True, False)} - {(23, True)}
    assert sum(1 for s in N.TIMESTAMPS if s in {h[2] for h in N.halfway_cases()}) >= 20


def test_edges_and_spellings_present(corpus):
    c = set(corpus["constructed"])
    for s in ("2.2250738585072009e-308", "2.2250738585072014e-308", "2.2250738585072008e-308",
              "2.2250738585072015e-308", "4.9406564584124654e-324", "2.470328229206232720e-324",
              "2.470328229206232721e-324", "9999999999999999999e-342", "9999999999999999999e-343",
              "1.7976931348623157e308", "1.7976931348623158e308", "1.797693134862315808e308", "1e309",
              "1E5", "2e+7", "25e-3", "1e007", "0001.5", "+1.5", "-0.0", "0e0", "0.000", "+Inf", "-NaN"):
        assert s in c, s
    # the edges decide what they are meant to decide
    assert float("2.470328229206232720e-324") == 0.0 and float("2.470328229206232721e-324") == 5e-324
    assert float("1.797693134862315807e308") < float("inf") == float("1.797693134862315808e308")
    assert float("7.410984687618698162e-324") == 5e-324 and float("7.410984687618698163e-324") == 1e-323


@pytest.mark.parametrize("rotate", [0, 7])
def test_corpus_bodies_parse_to_float_bits_on_the_cpu(lib, rotate):
    """The bodies the GPU test packs: the host-compiled device logic and the host packer both give
    float()'s bits for every value and timestamp."""
    bodies, vals, ts = N.corpus_bodies(N.value_corpus(), rotate)
    assert max(b.count(b'"],[') + 1 for b in bodies) == 2000 and len(bodies) == -(-len(vals) // 2000)
    want_v, want_t = N.expected_bits(vals), N.expected_bits(ts)
    a = 0
    for b in bodies:
        rc, v, t = _check_body(lib, b, want_ts=1)
        assert rc == JSON_OK
        bad = np.flatnonzero((v.view(np.uint64) != want_v[a:a + v.size]) | (t.view(np.uint64) != want_t[a:a + v.size]))
        assert bad.size == 0, (vals[a + bad[0]], ts[a + bad[0]])
        a += v.size
    assert a == len(vals)
    ps, pt = pack_query_range_bodies([[b] for b in bodies], want_timestamps=True)
    assert np.array_equal(ps.values.view(np.uint64), want_v)
    assert np.array_equal(pt.view(np.uint64), want_t)


# ---- the lattice ----

@pytest.fixture(scope="module")
def lattice():
    return L.per_body()


def _by_line(cases, line):
    return [c for c in cases if c.line == line]


def _rel(c, off):
    return off - (c.vs & ~(L.LANE - 1))


def test_positions_are_the_bytes(lattice):
    """The bookkeeping against the bytes: bodies back to back, vs at the first element's '[', every
    start a '[', `end` at "]]"; the counts per lattice line."""
    bodies, cases = lattice
    buf = b"".join(bodies)
    off = 0
    for b, c in zip(bodies, cases):
        assert c.off == off and c.body == b
        off += len(b)
        if c.kind == "empty_result":
            continue
        assert buf[c.vs - 1:c.vs] == b"["
        if c.kind == "empty_values":
            assert buf[c.vs:c.vs + 1] == b"]" and not c.starts
            continue
        assert c.starts[0] == c.vs and all(buf[s] == ord("[") for s in c.starts)
        assert buf[c.end:c.end + 3] == b"]]}" and buf.count(b"[", c.vs, c.end) == len(c.starts)
        assert len(c.starts) == len(c.vals) == len(c.ts)
        assert all(b - a >= 8 for a, b in zip(c.starts, c.starts[1:]))
    counts = {}
    for c in cases:
        counts[c.line] = counts.get(c.line, 0) + 1
    assert counts == {"array_start": 32, "array_end": 47, "dense": 64, "element_length": 177, "edge_start": 6,
                      "back_to_back": 16, "empty": 12}
    assert len({c.name for c in cases}) == len(cases)


def test_array_start_residues(lattice):
    assert {c.vs % L.LANE for c in _by_line(lattice[1], "array_start")} == set(range(L.LANE))


def test_array_end_residues_and_straddles(lattice):
    ends = _by_line(lattice[1], "array_end")
    assert {c.end % L.LANE for c in ends if c.tag[0] == "res"} == set(range(L.LANE))
    by = {c.tag: c for c in ends if c.tag[0] != "res"}
    for what, size, rs in (("lane", L.LANE, (0,)), ("block", L.BLOCK, (0,)), ("stage", L.STAGE, (0,)),
                           ("part", L.PART, (0, 17))):
        for r in rs:
            before, straddle, after = (by[(what, side, r)] for side in ("before", "straddle", "after"))
            assert before.vs % L.LANE == straddle.vs % L.LANE == after.vs % L.LANE == r
            # the pair's first ']' on the last byte before the boundary, the second on the first after
            assert _rel(straddle, straddle.end) % size == size - 1 and _rel(straddle, straddle.end) // size == \
                (4 if what == "lane" else 0)
            assert _rel(before, before.end) % size == size - 2   # both brackets before it
            assert _rel(after, after.end) % size == 0            # the first ']' on the first byte after it
            assert _rel(after, after.end) // size == (5 if what == "lane" else 1)
    # a lane straddle that is no block straddle, a block straddle (lane 63 bit 31), the part's at both
    # alignments of the array's start
    assert L.phase(by[("lane", "straddle", 0)].end, by[("lane", "straddle", 0)].vs) == (0, 4, 31)
    assert L.phase(by[("block", "straddle", 0)].end, by[("block", "straddle", 0)].vs) == (0, 63, 31)
    for r in (0, 17):
        c = by[("part", "straddle", r)]
        assert L.phase(c.end, c.vs) == (7, 63, 31) and c.vs % L.LANE == r
        c = by[("part", "after", r)]  # the second part holds no element start
        assert all(_rel(c, s) < L.PART for s in c.starts) and _rel(c, c.end) == L.PART


def test_dense_elements_fill_every_lane(lattice):
    dense = _by_line(lattice[1], "dense")
    assert {c.tag for c in dense} == {(n, s) for n in L.DENSE_N for s in range(8)}
    for c in dense:
        n, s = c.tag
        assert len(c.starts) == n and c.vs % L.LANE == s
        assert all(b - a == 8 for a, b in zip(c.starts, c.starts[1:])) and c.end - c.starts[-1] == 6
        per_lane = np.bincount(np.array([_rel(c, x) // L.LANE for x in c.starts]))
        assert per_lane.max() <= L.MAX_PER_LANE
        assert (per_lane[:-1] == L.MAX_PER_LANE).all()  # every lane but the array's last one is full
        assert (per_lane == L.MAX_PER_LANE).sum() == n // 4
        if n >= 257:
            assert (per_lane[:64] == L.MAX_PER_LANE).all()  # a whole block of full lanes
    digits = {tuple(c.vals[:40]) for c in dense if len(c.vals) >= 40}
    assert len(digits) > 20 and all(len(set(d)) >= 8 for d in digits)  # the digits vary


def test_element_length_classes(lattice):
    cases = _by_line(lattice[1], "element_length")
    want = {(n, f, p) for n in L.ELEMENT_LENGTHS for f in (("plain",) if n == 8 else L.FORMS) if n >= L.FORM_MIN[f]
            for p in L.POSITIONS}
    assert {c.tag for c in cases} == want
    # only 9 bytes cannot be reached by a fraction (".0" takes two)
    assert {(n, f) for n in L.ELEMENT_LENGTHS for f in L.FORMS} - {t[:2] for t in want} == \
        {(8, f) for f in L.FORMS} | {(9, "vfrac0"), (9, "tfrac0")}
    empty_block, past_stage, empty_part = set(), set(), set()
    for c in cases:
        n, form, pos = c.tag
        k = {"first": 0, "middle": 3, "last": 5}[pos]
        nxt = c.starts[k + 1] if k + 1 < len(c.starts) else c.end + 2
        assert nxt - c.starts[k] == n and len(c.starts) == 6  # the length, its separator counted
        text = c.body[c.starts[k] - c.off:nxt - c.off]
        assert {"plain": True, "lead0": b'"00' in text or n == 9, "vfrac0": b'0"' in text, "tfrac0": b"0," in text,
                "blanks": b" " in text}[form]
        blocks = {_rel(c, s) // L.BLOCK for s in c.starts}
        if set(range(_rel(c, c.end) // L.BLOCK + 1)) - blocks:
            empty_block.add(n)
        if c.starts[k] + n > (c.vs & ~31) + _rel(c, c.starts[k]) // L.BLOCK * L.BLOCK + L.STAGE:
            past_stage.add(c.tag)
        parts = {_rel(c, s) // L.PART for s in c.starts}
        if set(range(_rel(c, c.end + 1) // L.PART + 1)) - parts:
            empty_part.add(c.tag)
    # blocks without an element start, elements read partly from global memory, parts without a start
    assert {4097, 16385, 40 * 1024 + 7} <= empty_block and 4096 in empty_block
    assert {t for t in want if t[0] >= 4097} <= past_stage
    assert {t for t in want if t[0] > 2 * L.PART} <= empty_part and {t[0] for t in empty_part} >= {16385}


def test_edge_starts(lattice):
    by = {c.tag: c for c in _by_line(lattice[1], "edge_start")}
    assert set(by) == {(w, s) for w in ("lane", "block", "part") for s in ("short", "long")}
    for (what, size), c in by.items():
        unit = {"lane": L.LANE, "block": L.BLOCK, "part": L.PART}[what]
        hit = [k for k, s in enumerate(c.starts) if _rel(c, s) % unit == unit - 1]
        assert len(hit) == 1
        k = hit[0]
        assert _rel(c, c.starts[k]) == (4 * L.LANE if what == "lane" else unit) - 1
        length = c.starts[k + 1] - c.starts[k]
        assert length == 8 if size == "short" else length > L.STAGE
        assert len(c.starts) == k + 4


def test_back_to_back_and_empty_bodies(lattice):
    bodies, cases = lattice
    pairs = _by_line(cases, "back_to_back")
    firsts = [c for c in pairs if c.tag[1] == 0]
    assert sorted(len(c.body) % 8 for c in firsts) == list(range(8))
    for c in firsts:
        nxt = cases[cases.index(c) + 1]
        assert nxt.tag == (c.tag[0], 1) and nxt.off == c.off + len(c.body) and len(nxt.starts) == 40
        # the first body's slots (offset / 8 + element) end below the second's
        assert (c.off >> 3) + len(c.starts) <= nxt.off >> 3
    kinds = [c.kind for c in cases]
    assert kinds.count("empty_values") == 6 and kinds.count("empty_result") == 6
    for i, c in enumerate(cases):
        if c.kind != "array":
            assert 0 < i < len(cases) - 1 or c.kind == "empty_result"
    assert any(a.kind == "empty_result" and b.kind == "array" for a, b in zip(cases, cases[1:]))


@pytest.mark.parametrize("front", [0, 13])
def test_front_filler_shifts_every_case(lattice, front):
    bodies, cases = L.per_body(front)
    if front == 0:
        assert bodies == lattice[0]
        return
    assert len(bodies[0]) % L.LANE == front and bodies[1:] == lattice[0]
    buf = b"".join(bodies)
    for c, c0 in zip(cases, lattice[1]):
        assert c.off == c0.off + len(bodies[0]) and c.body == c0.body
        assert all(buf[s] == ord("[") for s in c.starts)
        if c.kind == "array":
            assert c.vs % L.LANE == (c0.vs + front) % L.LANE and buf[c.end:c.end + 2] == b"]]"


def test_lattice_bodies_parse_to_float_bits_on_the_cpu(lib, lattice):
    """json_check_body (the device logic, g++) gives JSON_OK and float()'s bits for every lattice
    body, and so does the host packer."""
    bodies, cases = lattice
    ps, pt, counts = pack_query_range_bodies([[b] for b in bodies], want_timestamps=True, return_pod_counts=True)
    offs = ps.offsets
    for i, (b, c) in enumerate(zip(bodies, cases)):
        rc, v, t = _check_body(lib, b, want_ts=1)
        if c.kind == "empty_result":
            assert rc == JSON_DROPPED and counts[i] < 0
            continue
        assert rc == JSON_OK, c.name
        want_v, want_t = N.expected_bits(c.vals), N.expected_bits(c.ts)
        assert np.array_equal(v.view(np.uint64), want_v), c.name
        assert np.array_equal(t.view(np.uint64), want_t), c.name
        assert np.array_equal(ps.values[offs[i]:offs[i + 1]].view(np.uint64), want_v), c.name
        assert np.array_equal(pt[offs[i]:offs[i + 1]].view(np.uint64), want_t), c.name
        rc, v, _ = _check_body(lib, b, want_ts=0)
        assert rc == JSON_OK and np.array_equal(v.view(np.uint64), want_v), c.name


@pytest.mark.parametrize("front", [0, 21])
def test_grouped_lattice_on_the_cpu(lib, front):
    """The same series in grouped bodies: positions from the bytes, the same geometry classes as
    the per-body lattice, json_check_grouped and plan.pack with float()'s bits."""
    plan = make_plan()
    bodies, cases = L.grouped([len(g.pods) for g in plan.groups], front)
    per = {c.name: c for c in L.per_body()[1]}
    buf = b"".join(bodies)
    for c in cases:
        p = per[c.name]
        assert buf[c.off:c.off + 10] == b'{"metric":' and buf[c.vs - 1:c.vs] == b"["
        if c.kind == "array":
            assert all(buf[s] == ord("[") for s in c.starts) and buf[c.end:c.end + 3] == b"]]}"
            # the same array at the same residue (shifted by the front pad): the same geometry
            if c.tag[1:] == (0,) and c.line == "back_to_back":  # placed by the series' length mod 8
                assert (c.vs - front) % L.LANE < 8
            else:
                assert (c.vs - front) % L.LANE == p.vs % L.LANE
            assert [s - c.vs for s in c.starts] == [s - p.vs for s in p.starts] and c.end - c.vs == p.end - p.vs
            assert c.vals == p.vals and c.ts == p.ts
    firsts = [c for c in cases if c.line == "back_to_back" and c.tag[1] == 0]
    assert sorted(len(c.body) % 8 for c in firsts) == list(range(8))
    want_v = np.concatenate([[N.want_bits("2")]] + [N.expected_bits(c.vals) for c in cases]).astype(np.uint64)
    want_t = np.concatenate([[N.want_bits("1")]] + [N.expected_bits(c.ts) for c in cases]).astype(np.uint64)
    k = 0
    for b in bodies:
        rc, got, v, t = _grouped(lib, b)
        assert rc == JSON_OK
        n = sum(g[1] for g in got)
        assert np.array_equal(v[:n].view(np.uint64), want_v[k:k + n])
        assert np.array_equal(t[:n].view(np.uint64), want_t[k:k + n])
        k += n
    assert k == want_v.size
    ps, pt, counts = plan.pack(bodies, want_timestamps=True, return_pod_counts=True)
    assert np.array_equal(ps.values.view(np.uint64), want_v) and np.array_equal(pt.view(np.uint64), want_t)
    assert np.array_equal(np.diff(ps.offsets), [1] + [len(c.vals) for c in cases])

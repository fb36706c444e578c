"""The byte-phase lattice of the device packer's wave-parallel values parse (krr_amd/csrc/krr_json.h
values_array / values_scan / values_part): response bodies built so that every edge of that
geometry is met on purpose, each case in a body (or, grouped, a series) of its own, with the value
and timestamp strings of every element and, computed from the bytes, where the array starts, where
every element starts and where its closing `]]` lies.  numpy and the standard library only; the CPU
test tests/test_json_lattice_layout.py pins what is covered, tests/test_gpu_json_lattice.py runs it
on the device.

The geometry (krr_json.h): the bodies lie back to back in one buffer; a values array whose first
element's '[' is at absolute offset vs is cut from blk0 = vs & ~31 into 2-KiB blocks of 64 lanes x
32 bytes (`phase`), the wave stages 4 KiB from the block's start in LDS and reads what an element
holds beyond it from global memory, a lane takes at most 4 element starts, and the split parse of
grouped bodies cuts the array into 16-KiB parts from blk0.  So every case is fixed by vs mod 32
(set by the length of a metric label value) and by the bytes of the array; a filler body in front
shifts all of them together.

Long elements are made only from forms the host packer and the device accept alike: leading zeros
of the value, trailing fraction zeros of the value or of the timestamp, JSON blanks between tokens.
"""
from dataclasses import dataclass, field
from typing import Optional

LANE, BLOCK, STAGE, PART = 32, 2048, 4096, 16384
MAX_PER_LANE = 4

HEAD = b'{"status":"success","data":{"resultType":"matrix","result":[{"metric":{"pod":"'
MID = b'"},"values":['
TAIL = b']}]}}'
EMPTY_RESULT = b'{"status":"success","data":{"resultType":"matrix","result":[]}}'
GHEAD = b'{"status":"success","data":{"resultType":"matrix","result":['
GTAIL = b']}}'

DENSE_N = (1, 3, 4, 5, 255, 256, 257, 1000)
ELEMENT_LENGTHS = (8, 9, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 16385, 40 * 1024 + 7)
FORMS = ("lead0", "vfrac0", "tfrac0", "blanks")
FORM_MIN = {"plain": 8, "digits": 9, "lead0": 9, "vfrac0": 10, "tfrac0": 10, "blanks": 9}  # shortest element of each
POSITIONS = ("first", "middle", "last")


def phase(off: int, vs: int):
    """(block, lane, bit) of absolute offset ``off`` in the array starting at ``vs``."""
    rel = off - (vs & ~(LANE - 1))
    return rel // BLOCK, rel % BLOCK // LANE, rel % LANE


# ---- elements: (timestamp string, value string, bytes without the separator after it) ----

def _digit(i: int, salt: int) -> str:
    return str(((i + salt) * 2654435761 >> 7) % 10)


def short(i: int):
    """`[d,"d"]`: with its separator the 8 bytes no element is shorter than."""
    t, v = _digit(i, 1), _digit(i, 5)
    return t, v, f'[{t},"{v}"]'.encode()


def stretched(i: int, length: int, form: str):
    """An element of ``length`` bytes, its separator counted, lengthened by ``form``."""
    n = length - 8  # bytes more than `[d,"d"]` + separator
    t, v = _digit(i, 2) if _digit(i, 2) != "0" else "7", _digit(i, 3) if _digit(i, 3) != "0" else "4"
    if n < 0 or length < FORM_MIN[form]:
        raise ValueError((length, form))
    if form == "plain":
        return short(i)
    if form == "digits":   # a longer integer value, for fillers of 9 to 15 bytes
        v = "123456789"[:n + 1]
        return t, v, f'[{t},"{v}"]'.encode()
    if form == "lead0":
        v = "0" * n + v
        return t, v, f'[{t},"{v}"]'.encode()
    if form == "vfrac0":
        v = v + ".25" + "0" * (n - 3) if n >= 3 else v + ".0"
        return t, v, f'[{t},"{v}"]'.encode()
    if form == "tfrac0":
        t = t + ".75" + "0" * (n - 3) if n >= 3 else t + ".0"
        return t, v, f'[{t},"{v}"]'.encode()
    if form == "blanks":
        ws = (" \n\t\r" * (n // 4 + 1))[:n]
        a = ws[:n // 2]
        b = ws[n // 2:]
        return t, v, f'[{a}{t},{b}"{v}"]'.encode()
    raise ValueError(form)


def fill(i0: int, nbytes: int) -> list:
    """Elements that take exactly ``nbytes`` with their separators: `[d,"d"],` throughout and
    one of 8 to 15 bytes at the end."""
    if nbytes < 8:
        raise ValueError(nbytes)
    k = nbytes // 8 - 1
    out = [short(i0 + j) for j in range(k)]
    rest = nbytes - 8 * k
    out.append(short(i0 + k) if rest == 8 else stretched(i0 + k, rest, "digits"))
    return out


@dataclass
class Spec:
    line: str                 # the lattice line the case belongs to
    name: str
    r: Optional[int]          # vs mod 32 (None: chosen so that the body's length is len_mod8 mod 8)
    elems: list               # [] with kind != "array"
    len_mod8: Optional[int] = None
    kind: str = "array"       # "array", "empty_values", "empty_result"
    tag: tuple = ()           # what the case was built for (the layout test checks it from the bytes)


def array_ending_at(i0: int, r: int, rel_end: int) -> list:
    """Elements whose array, started at r in its first lane, has the first ']' of its closing
    "]]" at ``rel_end`` bytes from blk0."""
    return fill(i0, rel_end - r + 2)


def specs() -> list:
    out = []

    def empties(k):
        out.append(Spec("empty", f"empty_values_{k}", (5 * k) % LANE, [], kind="empty_values"))
        out.append(Spec("empty", f"empty_result_{k}", None, [], kind="empty_result"))

    # array start: the first '[' at each residue
    for r in range(LANE):
        out.append(Spec("array_start", f"start_r{r}", r,
                        [short(r), stretched(r + 1, 10, "digits"), short(r + 2), stretched(r + 3, 13, "lead0"),
                         short(r + 4)], tag=(r,)))
    empties(0)
    # array end: the first ']' of "]]" at each residue; the pair across a lane, a block, the stage's
    # and a part's end (the part at both alignments of the array's start: on and off blk0), and
    # wholly on either side of each
    for res in range(LANE):
        out.append(Spec("array_end", f"end_res{res}", 0, array_ending_at(res, 0, 2 * LANE + res), tag=("res", res)))
    for what, edge, rs in (("lane", 5 * LANE, (0,)), ("block", BLOCK, (0,)), ("stage", STAGE, (0,)),
                           ("part", PART, (0, 17))):
        for r in rs:
            for side, d in (("before", -2), ("straddle", -1), ("after", 0)):
                out.append(Spec("array_end", f"end_{what}_{side}_r{r}", r, array_ending_at(d + 2, r, edge + d),
                                tag=(what, side, r)))
    empties(1)
    # dense minimal elements: four starts in every lane, and the same shifted by 1..7 bytes
    for n in DENSE_N:
        for s in range(8):
            out.append(Spec("dense", f"dense_n{n}_s{s}", s, [short(3 * n + s + j) for j in range(n)], tag=(n, s)))
    empties(2)
    # element length: each length first, in the middle and last among short elements, by each form
    k = 0
    for length in ELEMENT_LENGTHS:
        for form in (("plain",) if length == 8 else FORMS):
            if length < FORM_MIN[form]:
                continue
            for pos in POSITIONS:
                at = {"first": 0, "middle": 3, "last": 5}[pos]
                elems = [short(k + j) for j in range(6)]
                elems[at] = stretched(k + at, length, form)
                out.append(Spec("element_length", f"len{length}_{form}_{pos}", (7 * k) % LANE, elems,
                                tag=(length, form, pos)))
                k += 1
    empties(3)
    # an element start on the last byte of a lane, a block, a part: a short element, and one longer
    # than the stage
    for what, edge in (("lane", 4 * LANE), ("block", BLOCK), ("part", PART)):
        for size, length in (("short", 8), ("long", STAGE + 104)):
            r = 5
            elems = fill(length, edge - 1 - r)
            elems.append(short(1) if size == "short" else stretched(2, length, "lead0"))
            elems += [short(7 + j) for j in range(3)]
            out.append(Spec("edge_start", f"edge_{what}_{size}", r, elems, tag=(what, size)))
    empties(4)
    # back to back: the first body's length at every residue mod 8 (the scratch slot is offset >> 3)
    for m in range(8):
        out.append(Spec("back_to_back", f"pair{m}_first", None, [short(m + j) for j in range(40)], len_mod8=m,
                        tag=(m, 0)))
        out.append(Spec("back_to_back", f"pair{m}_second", 0, [short(2 * m + j) for j in range(40)], tag=(m, 1)))
    empties(5)
    return out


@dataclass
class Case:
    line: str
    name: str
    tag: tuple
    kind: str
    body: bytes               # the body (per-body path) or the series object (grouped path)
    off: int                  # its absolute offset, the bodies back to back from 0
    vs: int                   # absolute offset of the first element's '[' (of the array's ']' when empty)
    starts: list = field(default_factory=list)   # absolute offset of every element's '['
    end: int = -1             # absolute offset of the first ']' of the closing "]]"
    ts: list = field(default_factory=list)       # timestamp strings
    vals: list = field(default_factory=list)     # value strings

    def shifted(self, by: int) -> "Case":
        return Case(self.line, self.name, self.tag, self.kind, self.body, self.off + by, self.vs + by,
                    [s + by for s in self.starts], self.end + by if self.end >= 0 else -1, self.ts, self.vals)

    def where(self, k: int) -> str:
        """Element k's place, for a failure message."""
        off = self.starts[k]
        blk, lane, bit = phase(off, self.vs)
        return (f"case {self.name} element {k} of {len(self.starts)} at byte {off} "
                f"(lane {off % BLOCK // LANE} bit {off % LANE} of the buffer; block {blk} lane {lane} bit {bit} "
                f"of its array, vs = {self.vs})")


def _place(spec: Spec, off: int, head: bytes, mid: bytes, tail: bytes) -> Case:
    """The case's bytes at absolute offset ``off``: the pad between head and mid puts vs at the
    wanted residue."""
    if spec.kind == "empty_result":
        return Case(spec.line, spec.name, spec.tag, spec.kind, EMPTY_RESULT, off, -1)
    array = b",".join(e[2] for e in spec.elems)
    r = spec.r
    if r is None:  # the body's length fixed mod 8: pad = r - (off + head + mid) mod 32
        r = (spec.len_mod8 - len(array) - len(tail) + off) % 8
    pad = (r - (off + len(head) + len(mid))) % LANE
    body = head + b"x" * pad + mid + array + tail
    vs = off + len(head) + pad + len(mid)
    assert vs % LANE == r and (spec.len_mod8 is None or len(body) % 8 == spec.len_mod8)
    c = Case(spec.line, spec.name, spec.tag, spec.kind, body, off, vs)
    if spec.kind == "array":
        at = vs
        for t, v, text in spec.elems:
            c.starts.append(at)
            at += len(text) + 1
        c.end = vs + len(array) - 1
        c.ts = [e[0] for e in spec.elems]
        c.vals = [e[1] for e in spec.elems]
    return c


def per_body(front: int = 0):
    """(bodies, cases): one body per case, back to back in this order.  ``front`` > 0 puts a
    filler body in front whose length is ``front`` mod 32: the same bodies at shifted phases."""
    cases, off = [], 0
    for spec in specs():
        c = _place(spec, off, HEAD, MID, TAIL)
        cases.append(c)
        off += len(c.body)
    bodies = [c.body for c in cases]
    if front:
        f = filler(front)
        return [f] + bodies, [c.shifted(len(f)) for c in cases]
    return bodies, cases


def filler(front: int) -> bytes:
    """A one-sample body whose length is ``front`` mod 32."""
    base = len(HEAD) + len(MID) + len(b'[1,"2"]') + len(TAIL)
    return HEAD + b"f" * ((front - base) % LANE) + MID + b'[1,"2"]' + TAIL


def pod_name(k: int) -> str:
    return f"pod-{k:04d}"


def grouped_specs() -> list:
    return [s for s in specs() if s.kind != "empty_result"]


def grouped(group_sizes, front: int = 0):
    """(bodies, cases): the same series contents as `{"metric":{"pod":...,"z":pad},"values":[...]}`
    series of grouped bodies, ``group_sizes[g]`` series in body g; series k's pod is pod_name(k).
    Series 0 is a one-sample filler whose pad is ``front`` bytes long (the shift); cases[k - 1] is
    series k."""
    sp = grouped_specs()
    assert sum(group_sizes) == len(sp) + 1, (sum(group_sizes), len(sp) + 1)
    bodies, cases, off, k = [], [], 0, 0
    for n in group_sizes:
        parts = [GHEAD]
        off += len(GHEAD)
        for j in range(n):
            if j:
                parts.append(b",")
                off += 1
            head = f'{{"metric":{{"pod":"{pod_name(k)}","z":"'.encode()
            if k == 0:
                ser = head + b"f" * front + MID + b'[1,"2"]' + b"]}"
            else:
                c = _place(sp[k - 1], off, head, MID, b"]}")
                cases.append(c)
                ser = c.body
            parts.append(ser)
            off += len(ser) - (front if k == 0 else 0)  # placed as without the shift: the same bytes
            k += 1
        parts.append(GTAIL)
        off += len(GTAIL)
        bodies.append(b"".join(parts))
    return bodies, [c.shifted(front) for c in cases]

"""The number corpus of the device packer's decimal -> binary64 conversion (krr_json_parse.h
scan_number / eisel_lemire): one list of strings read by the CPU logic test
(tests/test_json_device_logic.py, a g++ build of the header) and by the GPU test
(tests/test_gpu_json_lattice.py, the device build).  numpy and the standard library only.

Three groups of sample VALUE strings:
  * shortest_repr_values()   Prometheus' 'f'-format shortest reprs of every magnitude;
  * midpoint_cases()         random 1-19 digit significands over every exponent and decimal
                             strings of exact binary midpoints;
  * constructed_values()     built, not drawn: significands whose first 64-bit product leaves
                             the rounding bits unsure (the second multiply), exact halfway cases
                             for every q in [-4, 23], the subnormal, underflow and overflow
                             edges, and the accepted spellings.
TIMESTAMPS holds JSON-number literals of the same kinds (the sample's time, JSON grammar only),
HANDOVER the strings the device must leave to the host packer.  The reference for every accepted
string is Python's float() — correctly rounded — bit for bit (want_bits: NaN by SPECIAL_BITS).
"""
import re
from decimal import Decimal

import numpy as np

MASK64 = (1 << 64) - 1

# tests/test_json_device_logic.py test_special_spellings' table
SPECIAL_BITS = {"NaN": 0x7FF8000000000000, "-NaN": 0xFFF8000000000000, "+NaN": 0x7FF8000000000000,
                "+Inf": 0x7FF0000000000000, "-Inf": 0xFFF0000000000000, "Inf": 0x7FF0000000000000,
                "-0": 0x8000000000000000, "0": 0, "1e400": 0x7FF0000000000000, "-1e-400": 0x8000000000000000}


def bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def want_bits(s: str) -> int:
    """The binary64 an accepted string stands for: float() (correctly rounded); NaN's sign and
    payload from SPECIAL_BITS."""
    if s in SPECIAL_BITS:
        return SPECIAL_BITS[s]
    return bits(float(s))


def go_format(x: float) -> str:
    from krr_amd.utils.prom_decimal import prom_format

    return prom_format(x)


# ---- group 1 and 2: the generators of the CPU logic test, seeds and strings unchanged ----

def shortest_repr_values() -> list:
    rng = np.random.default_rng(7)
    xs = np.concatenate([
        rng.gamma(2.0, 0.05, 20000),
        np.floor(rng.normal(2e8, 2e7, 5000)),
        np.exp(rng.uniform(-744, 709, 20000)),                       # every exponent, subnormals included
        rng.integers(0, 2**63, 2000).astype(np.float64) * 2.0 ** rng.integers(0, 900, 2000),
        np.array([5e-324, 2.2250738585072014e-308, 2.2250738585072009e-308, 1.7976931348623157e308, 0.0, 1.0,
                  0.1, 0.2, 0.3, 1e22, 1e23, 9007199254740993.0, 123456789012345678.0]),
    ])
    xs = np.concatenate([xs, -xs[:3000]])
    return [go_format(float(x)) for x in xs]


def midpoint_cases() -> list:
    """1-19 digit significands with exponents over the whole range, plus decimal strings
    built from exact binary midpoints (the halfway cases the round-to-even branch decides)."""
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(40000):
        nd = int(rng.integers(1, 20))
        digits = str(int(rng.integers(1, 10))) + "".join(str(int(d)) for d in rng.integers(0, 10, nd - 1))
        e = int(rng.integers(-360, 320))
        cases.append(f"{digits}e{e}")
        cases.append(f"0.{digits}")
    for _ in range(6000):  # midpoints between adjacent doubles, written exactly when short enough
        x = float(np.exp(rng.uniform(-50, 50)))
        lo = Decimal(x)
        hi = Decimal(float(np.nextafter(x, np.inf)))
        mid = (lo + hi) / 2
        s = format(mid, "f")
        if len(s.replace(".", "").lstrip("0")) <= 19:
            cases.append(s)
    return cases


# ---- the acceptance rule (krr_json_parse.h header comment and scan_number's) ----

_VALUE = re.compile(r"[+-]?(?:NaN|Inf|(?P<i>[0-9]+)(?:\.(?P<f>[0-9]+))?(?:[eE][+-]?(?P<e>[0-9]+))?)\Z")
_JSON = re.compile(r"-?(?P<i>0|[1-9][0-9]*)(?:\.(?P<f>[0-9]+))?(?:[eE][+-]?(?P<e>[0-9]+))?\Z")


def acceptable(s: str, value_form: bool = True) -> bool:
    """Does the device parse ``s`` itself?  The grammar (a sample value string: an optional sign,
    then digits with an optional fraction and exponent, or NaN / Inf; a timestamp: a JSON number),
    at most 19 significant digits after the leading zeros, trailing zeros not counted, and at
    most 6 exponent digits."""
    m = (_VALUE if value_form else _JSON).match(s)
    if not m:
        return False
    if m.group("i") is None:
        return True  # NaN / Inf
    digits = (m.group("i") + (m.group("f") or "")).lstrip("0").rstrip("0")
    return len(digits) <= 19 and len(m.group("e") or "") <= 6


# ---- group 3: constructed ----

def pow5_high(q: int) -> int:
    """The high 64-bit word of the 128-bit power of five Eisel-Lemire multiplies by for 10^q
    (the published table: floor(2^b / 5^-q) + 1 for q < 0, the leading bits of 5^q otherwise)."""
    if q < 0:
        p5 = 5 ** -q
        z = (p5 - 1).bit_length()
        if q >= -27:
            c = (1 << (z + 127)) // p5 + 1
        else:
            c = (1 << (2 * z + 128)) // p5 + 1
            while c >= (1 << 128):
                c //= 2
    else:
        c = 5 ** q
        c = c << (128 - c.bit_length()) if c.bit_length() <= 128 else c >> (c.bit_length() - 128)
    return c >> 64


def first_product_unsure(w: int, q: int) -> bool:
    """eisel_lemire's `(hi & 0x1FF) == 0x1FF` for the significand w and the exponent q: the
    high word of (w normalised) x (the table's high word) ends in nine one bits."""
    wn = (w << (64 - w.bit_length())) & MASK64
    return ((wn * pow5_high(q)) >> 64) & 0x1FF == 0x1FF


def second_multiply_strings(step: int = 1) -> list:
    """One `<w>e<q>` per q in [-342, 308] (every ``step``-th) whose first product is unsure: w
    walks a fixed sequence of 15 to 19 digit integers (the digit count and the start depend on
    q) until the condition holds — one in 512 does, except where the table word has few bits
    (q near 0: only the longest significands reach the low nine bits), so the search moves on
    to more digits after 4,096 misses."""
    out = []
    for q in range(-342, 309, step):
        hi_word = pow5_high(q)
        found = None
        for nd in list(range(15 + (q % 5), 20)) + list(range(15, 15 + (q % 5))):
            lo, span = 10 ** (nd - 1), 9 * 10 ** (nd - 1)
            for k in range(4096):
                x = ((q + 343) * 4096 + k + 1) * 11_400_714_819_323_198_485 & MASK64
                x ^= x >> 29
                x = x * 7_046_029_254_386_353_131 & MASK64
                w = lo + x % span
                wn = (w << (64 - w.bit_length())) & MASK64
                if ((wn * hi_word) >> 64) & 0x1FF == 0x1FF:
                    found = w
                    break
            if found:
                break
        assert found, q
        out.append(f"{found}e{q}")
    return out


def halfway_cases() -> list:
    """[(q, lower neighbour odd?, string)]: w x 10^q exactly between two adjacent normal doubles,
    w < 10^19.  Such a value is M x 2^k with M odd and 54 bits wide; w = M / 5^q x 2^j (q >= 0,
    so 5^q divides M) or M x 5^-q x 2^j (q < 0).  For every q the smallest M of each class
    (M mod 4 == 3: odd lower neighbour, rounds up; == 1: even, rounds down) is written with the
    exponent and as a plain decimal.  5^23 itself is the only M for q = 23: an even neighbour."""
    out = []
    for q in range(-4, 24):
        p = 5 ** abs(q)
        for odd in (True, False):
            if q >= 0:
                k = -(-(1 << 53) // p) | 1
                while (k * p) % 4 != (3 if odd else 1) and k * p < (1 << 54):
                    k += 2
                M = k * p
                w = k
            else:
                M = (1 << 53) + (3 if odd else 1)
                w = M * p
            if not ((1 << 53) <= M < (1 << 54)):
                continue
            assert w < 10 ** 19 and M % 2 == 1
            for j in (0, 3):
                if (w << j) >= 10 ** 19:
                    continue
                out.append((q, odd, f"{w << j}e{q}"))
                plain = format(Decimal(w << j).scaleb(q), "f")
                out.append((q, odd, plain))
    return out


SUBNORMAL_EDGES = [
    # the largest subnormal and the smallest normal, +- one unit in the 17th digit
    "2.2250738585072008e-308", "2.2250738585072009e-308", "2.2250738585072010e-308",
    "2.2250738585072013e-308", "2.2250738585072014e-308", "2.2250738585072015e-308",
    # the smallest subnormal 2^-1074, its half (the underflow threshold: ...27208828 exactly) and
    # one and a half of it, from below and from above, in at most 19 digits
    "4.9406564584124654e-324", "4.940656458412465441e-324", "4.940656458412465442e-324",
    "2.4703282292062327e-324", "2.4703282292062328e-324", "2.470328229206232720e-324",
    "2.470328229206232721e-324", "7.410984687618698162e-324", "7.410984687618698163e-324",
    "9.8813129168249309e-324", "5e-324", "3e-324", "2e-324",
    # q = -342 is the table's first entry, q = -343 is zero without a lookup
    "9999999999999999999e-342", "9999999999999999999e-343", "2470328229206232720e-342",
    "2470328229206232721e-342", "4940656458412465442e-342", "7410984687618698162e-342",
    "7410984687618698163e-342", "1e-342", "1e-343", "24703282292062327210e-343", "1000000000000000000e-342",
    "0.0000000000000000001e-323", "0.000000000000000000247032822920623272e-305",
]
OVERFLOW_EDGES = ["1.7976931348623157e308", "1.7976931348623158e308", "1.797693134862315808e308", "1e309",
                  "1.797693134862315807e308", "17976931348623157e292", "1797693134862315708e290",
                  "1797693134862315809e290", "9999999999999999999e308", "1e308", "1e400", "-1e-400"]
SPELLINGS = ["1E5", "1.5E+3", "2e+7", "25e-3", "1e007", "1E+2", "0001.5", "000", "00.5e1", "+1.5", "+0", "-0.0",
             "-0", "0e0", "0.000", "-0e-5", "0e999999", "1e000308", "+Inf", "-Inf", "Inf", "NaN", "+NaN", "-NaN",
             "12345678901234567890000", "0.00000000000000000001234567890123456789", "1.2345678901234567890000"]


def constructed_values() -> list:
    return (second_multiply_strings() + [s for _, _, s in halfway_cases()] + SUBNORMAL_EDGES + OVERFLOW_EDGES
            + SPELLINGS)


def value_corpus() -> list:
    """Every accepted value string, the three groups in order."""
    return shortest_repr_values() + midpoint_cases() + constructed_values()


def _json_halfway() -> list:
    out = []
    for _, _, s in halfway_cases():
        if acceptable(s, value_form=False) and 1e-3 < float(s) < 1e30:
            out.append(s)
    return out


# JSON-number timestamp literals: no '+', no leading zeros, no NaN / Inf
TIMESTAMPS = ["0", "-0", "0.5", "1.7e9", "1700000000.781", "1700000000", "1.70000006e9", "1700000060.5",
              "-1.5", "-0.0", "0e0", "0.000", "1E+2", "1e-7", "2.5E-3", "1e007", "10", "0.1",
              # 19 significant digits
              "1700000000.123456789", "1234567890123456789", "0.1234567890123456789", "1.700000000123456789e9",
              "9223372036854775807", "9999999999999999999", "1700000000123.456789",
              "-1700000000.123456789", "1700000000.1234567890000",
              # unsure first products and exact halfway cases, as JSON numbers
              ] + [s for s in second_multiply_strings(step=20) if 1e-300 < float(s) < 1e300] + _json_halfway()

_HEAD = b'{"status":"success","data":{"resultType":"matrix","result":[{"metric":{"pod":"c"},"values":['
_TAIL = b']}]}}'


def corpus_bodies(values, rotate: int = 0, per_body: int = 2000):
    """(bodies, value strings, timestamp strings): ``values`` rotated by ``rotate`` elements and
    cut into bodies of at most ``per_body`` samples, value i paired with timestamp literal i
    modulo TIMESTAMPS."""
    vals = list(values[rotate:]) + list(values[:rotate])
    ts = [TIMESTAMPS[i % len(TIMESTAMPS)] for i in range(len(vals))]
    bodies = []
    for a in range(0, len(vals), per_body):
        bodies.append(_HEAD + ",".join(f'[{t},"{v}"]' for t, v in zip(ts[a:a + per_body], vals[a:a + per_body])).encode()
                      + _TAIL)
    return bodies, vals, ts


def expected_bits(strings) -> np.ndarray:
    return np.array([want_bits(s) for s in strings], dtype=np.uint64)


# what the device must hand to the host packer (test_other_spellings_go_to_the_host's list, a
# 20-digit significand with a nonzero 20th digit and a 7-digit exponent)
OTHER_SPELLINGS = ["nan", "inf", "Infinity", ".5", "5.", "1e", "1e+", "--1", "+-1", "1.2.3", "0x10",
                   "12345678901234567890123", "1" * 25 + ".5", "1e1234567", " 1", "1 ", ""]
HANDOVER = OTHER_SPELLINGS + ["12345678901234567891", "1.2345678901234567891", "1e0000001", "1e-1000000"]

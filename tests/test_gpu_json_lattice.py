"""The device packer (krr_amd/csrc/krr_json.h, krr_json_parse.h) on the GPU, over the number corpus
of tests/_json_numbers.py and the byte-phase lattice of tests/_json_lattice.py.

* Numbers: the device build of scan_number / eisel_lemire (its own multiply-high, count-leading-zeros
  and powers-of-five table) against Python's float() — correctly rounded — bit for bit, on every
  magnitude, 18 and 19 digit significands, exponent spellings, the second multiply, exact halfway
  cases, subnormals, underflow and overflow; what it must not decide goes to the host.
* Lattice: the wave geometry of values_array, values_scan and values_part — lanes, blocks, the LDS
  stage and the global-memory leg past it, the split parse's parts, `]]` across every boundary,
  four starts in every lane, blocks and parts without a start — each case in a body of its own.

tests/test_json_lattice_layout.py pins what both cover and checks every body on the CPU (the same
header compiled by g++, and the host packer), so a failure here is the device build's or the wave
geometry's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _json_lattice as L  # noqa: E402
import _json_numbers as N  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def packer():
    from krr_amd import _native
    from krr_amd.core.device_pack import DevicePacker

    ctx = _native.Context(0)
    yield DevicePacker(ctx, chunk_bytes=1 << 20)
    ctx.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _host(per_obj, want_ts=True):
    from krr_amd.core.prom_native import pack_query_range_bodies

    return pack_query_range_bodies(per_obj, want_timestamps=want_ts, return_pod_counts=True)


def _same_layout(dp, host_series, host_counts):
    assert np.array_equal(_np(dp.series.offsets), host_series.offsets)
    assert dp.series.max_len == host_series.max_len
    assert np.array_equal(_np(dp.pod_counts), host_counts)


# ---- numbers ----

@pytest.fixture(scope="module")
def corpus():
    return tuple(N.value_corpus())


@pytest.mark.parametrize("rotate", [0, 1, 7, 13])
def test_number_corpus_on_the_device(packer, corpus, rotate):
    """Every corpus string as a sample value (and the timestamp literals beside them), in bodies
    of 2,000 samples: parsed on the device, float()'s bits.  The rotations move every string to
    other lanes and blocks."""
    bodies, vals, ts = N.corpus_bodies(corpus, rotate)
    per_obj = [[b] for b in bodies]
    dp = packer.pack(per_obj, want_timestamps=True, return_pod_counts=True)
    assert dp.via == "device" and dp.host_bodies == 0
    hs, _, hc = _host(per_obj)
    _same_layout(dp, hs, hc)
    for what, got, strings in (("value", _np(dp.series.values), vals), ("timestamp", _np(dp.timestamps), ts)):
        want = N.expected_bits(strings)
        got = got.view(np.uint64)
        assert got.size == want.size
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{bad.size} {what}s differ; first: {strings[bad[0]]!r} (sample {bad[0] % 2000} of body "
                               f"{bad[0] // 2000}) gave {int(got[bad[0]]):#018x}, float() {int(want[bad[0]]):#018x}")


@pytest.mark.parametrize("s", N.HANDOVER)
def test_other_spellings_make_the_batch_the_hosts(packer, s):
    """A value string the device does not decide, in the middle of an otherwise canonical body of a
    small batch: the batch goes to the host packer, whose result or error stands."""
    from krr_amd.core.prom_native import PrometheusResponseError

    def body(vals):
        return (L.HEAD + b"p" + L.MID + ",".join(f'[{1700000000 + 15 * i},"{v}"]' for i, v in enumerate(vals)).encode()
                + L.TAIL)

    plain = ["0.25", "1", "17.5", "3e2", "NaN", "0.001"]
    per_obj = [[body(plain)], [body(plain[:3] + [s] + plain[3:]), body(plain)], [body(plain[::-1])]]
    try:
        hs, ht, hc = _host(per_obj)
    except PrometheusResponseError as host_err:
        with pytest.raises(PrometheusResponseError) as dev_err:
            packer.pack(per_obj, want_timestamps=True, return_pod_counts=True)
        assert str(dev_err.value) == str(host_err) and dev_err.value.code == host_err.code
        return
    dp = packer.pack(per_obj, want_timestamps=True, return_pod_counts=True)
    assert dp.via == "host" and dp.host_bodies == 1
    _same_layout(dp, hs, hc)
    assert np.array_equal(_np(dp.series.values).view(np.uint64), hs.values.view(np.uint64))
    assert np.array_equal(_np(dp.timestamps).view(np.uint64), ht.view(np.uint64))


# ---- the lattice, per-body path ----

def _check_cases(cases, offsets, values, timestamps=None, first=0):
    """Segment first + k of the CSR is cases[k]: float()'s bits of its strings, element by element."""
    offsets = np.asarray(offsets)
    for k, c in enumerate(cases):
        a, b = int(offsets[first + k]), int(offsets[first + k + 1])
        assert b - a == len(c.vals), f"case {c.name}: {b - a} samples, {len(c.vals)} expected"
        for what, arr, strings in (("value", values, c.vals), ("timestamp", timestamps, c.ts)):
            if arr is None or not strings:
                continue
            want = N.expected_bits(strings)
            got = arr[a:b].view(np.uint64)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"{what} of {c.where(int(bad[0]))}: {strings[bad[0]][:40]!r} gave "
                                   f"{int(got[bad[0]]):#018x}, float() {int(want[bad[0]]):#018x}")


@pytest.mark.parametrize("front", range(L.LANE))
def test_lattice_per_body(packer, front):
    """All lattice bodies in one call, with timestamps and — through a packer that does not strip,
    so the positions hold — without; then the same bodies behind a filler body whose length is
    1 to 31 mod 32: every case at every other absolute phase as well."""
    from krr_amd.core.device_pack import DevicePacker

    bodies, cases = L.per_body(front)
    per_obj = [[b] for b in bodies]
    skip = 1 if front else 0
    hs, ht, hc = _host(per_obj)
    dp = packer.pack(per_obj, want_timestamps=True, return_pod_counts=True)
    assert dp.via == "device" and dp.host_bodies == 0
    _check_cases(cases, _np(dp.series.offsets), _np(dp.series.values), _np(dp.timestamps), first=skip)
    _same_layout(dp, hs, hc)
    plain = DevicePacker(packer.ctx, chunk_bytes=1 << 20, strip=False)
    dq = plain.pack(per_obj, want_timestamps=False, return_pod_counts=True)
    assert dq.via == "device" and plain.last_upload["bytes_sent"] == plain.last_upload["bytes"]
    _check_cases(cases, _np(dq.series.offsets), _np(dq.series.values), first=skip)
    _same_layout(dq, hs, hc)


def test_lattice_stripped(packer):
    """The default packer without timestamps stages the bodies with their timestamps cut, so the
    positions move: only the result is asserted, the host packer's bit for bit."""
    bodies, cases = L.per_body()
    per_obj = [[b] for b in bodies]
    assert packer.strip
    dp = packer.pack(per_obj, want_timestamps=False, return_pod_counts=True)
    hs, hc = _host(per_obj, want_ts=False)
    assert dp.via == "device"
    _same_layout(dp, hs, hc)
    assert np.array_equal(_np(dp.series.values).view(np.uint64), hs.values.view(np.uint64))


# ---- the lattice, grouped path ----

@pytest.fixture(params=[("chunk", True), ("end", True), ("chunk", False)], ids=["chunk-split", "end-split",
                                                                                   "chunk-wave"])
def route_mode(request, packer):
    """tests/test_gpu_json.py's routings: chunk by chunk or once at the end, the values arrays
    parsed in 16-KiB parts (values_scan / values_part) or one wave per series (values_array)."""
    was = packer.grouped_route, packer.grouped_split_parse
    packer.grouped_route, packer.grouped_split_parse = request.param
    yield request.param
    packer.grouped_route, packer.grouped_split_parse = was


@pytest.mark.parametrize("front", [0, 1, 8, 13, 31])
def test_lattice_grouped(packer, route_mode, front):
    """The same series contents as series of grouped bodies (one object per series, series 0 a
    filler whose label shifts the rest): float()'s bits and plan.pack's CSR.  With timestamps the
    bodies are staged whole, so the positions hold."""
    from test_json_lattice_layout import make_plan

    plan = make_plan()
    bodies, cases = L.grouped([len(g.pods) for g in plan.groups], front)
    want, want_ts, want_counts = plan.pack(bodies, want_timestamps=True, return_pod_counts=True)
    dp = packer.pack_grouped(plan, bodies, want_timestamps=True, return_pod_counts=True)
    assert dp.via == "device"
    _check_cases(cases, _np(dp.series.offsets), _np(dp.series.values), _np(dp.timestamps), first=1)
    assert np.array_equal(_np(dp.series.offsets), want.offsets)
    assert np.array_equal(_np(dp.series.values).view(np.uint64), want.values.view(np.uint64))
    assert np.array_equal(_np(dp.timestamps).view(np.uint64), want_ts.view(np.uint64))
    assert np.array_equal(np.asarray(dp.pod_counts), want_counts)
    assert dp.series.max_len == want.max_len

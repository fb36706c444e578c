"""The device packer's pod boundaries (include/krr_amd.h krr_json_pod_bounds,
krr_amd/csrc/krr_json.h k_json_pod_bounds) against the host packer's: ``pod_offsets``,
``pod_groups`` and ``pod_max_len`` of ``DevicePacker.pack`` / ``pack_many`` equal, element for
element, what ``pack_query_range_bodies`` puts on the same bodies.

The kernel runs one wave per object over its bodies in blocks of 64, so the hand-made layouts
sit on both sides of a block (1, 63, 64, 65 and 130 bodies) with dropped bodies at a block's
first and last place; objects without bodies, objects whose every body is dropped and a batch
without any kept pod exercise the empty ranges."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = b'{"status":"success","data":{"resultType":"matrix","result":[]}}'
# (strip, want_timestamps): the stripped staging copy, the plain one, and the plain one with
# timestamps (timestamps are never stripped)
CONFIGS = [(True, False), (False, False), (True, True)]


def _body(xs, t0=1700000000) -> bytes:
    from krr_amd.utils.prom_decimal import prom_format

    vals = ",".join(f'[{t0 + 60 * i},"{prom_format(float(x))}"]' for i, x in enumerate(xs))
    return ('{"status":"success","data":{"resultType":"matrix","result":[{"metric":{"pod":"p"},"values":[' + vals +
            ']}]}}').encode()


def _layout(objects, seed=0):
    """objects[o] = samples per body (-1: a dropped body, ``"result":[]``; 0: no samples)."""
    rng = np.random.default_rng(seed)
    return [[EMPTY if n < 0 else _body(rng.gamma(2.0, 0.05, n)) for n in bodies] for bodies in objects]


def _block_edges():
    """Objects of 1, 63, 64, 65 and 130 bodies: all kept, then with bodies 0, 63, 64 and the last
    dropped (as far as the object has them).  Mostly one-sample bodies; the kept 130-body object
    holds 500 samples per body so that the batch spans several 1-MiB parse launches."""
    objs = []
    for size in (1, 63, 64, 65, 130):
        kept = [1 + (i % 3 == 2) for i in range(size)]
        objs.append([500] * size if size == 130 else kept)
        holes = list(kept)
        for i in (0, 63, 64, size - 1):
            if i < size:
                holes[i] = -1 if i % 2 == 0 else 0
        objs.append(holes)
    return objs


def _fleet(seed, n_obj=60, max_samples=1200):
    """tests/test_gpu_json.py's generator shape: 0-4 bodies per object, dropped bodies, bodies
    without samples, NaN / Inf / 300-digit values, a second series that is ignored."""
    from krr_amd.utils.prom_decimal import prom_format

    rng = np.random.default_rng(seed)
    per_obj = []
    for o in range(n_obj):
        pods = []
        for p in range(int(rng.integers(0, 5))):
            if rng.random() < 0.12:
                pods.append(EMPTY)
                continue
            n = int(rng.integers(0, max_samples))
            xs = rng.gamma(2.0, 0.05, n)
            sp = rng.random(n)
            xs[sp < 0.01] = np.nan
            xs[(sp >= 0.01) & (sp < 0.015)] = np.inf
            m = (sp >= 0.02) & (sp < 0.1)
            xs[m] = np.floor(rng.normal(2e8, 2e7, int(m.sum())))
            m = (sp >= 0.105) & (sp < 0.11)
            xs[m] = 1e300 * rng.random(int(m.sum()))
            ts = 1.7e9 + 60.0 * np.arange(n) + 0.781
            res = [{"metric": {"pod": f"p{o}-{p}", "container": "c"},
                    "values": [[float(t), prom_format(float(x))] for t, x in zip(ts, xs)]}]
            if rng.random() < 0.3:
                res.append({"metric": {"pod": "x"}, "values": [[1.0, "7"]]})
            pods.append(json.dumps({"status": "success", "data": {"resultType": "matrix", "result": res}},
                                   separators=(",", ":")).encode())
        per_obj.append(pods)
    return per_obj


LAYOUTS = {
    "single_object": lambda: _layout([[5, 3]]),
    "objects_without_bodies": lambda: _layout([[], [2, 1], [], [4], []]),
    "every_body_dropped": lambda: _layout([[3], [-1, -1, -1], [2, 1]]),
    "no_kept_pod": lambda: _layout([[-1], [], [-1, 0]]),
    "one_sample_bodies": lambda: _layout([[1], [1, 1, 1], [1, -1, 1]]),
    "block_edges": lambda: _layout(_block_edges()),
    "fleet": lambda: _fleet(11),
}


@pytest.fixture(scope="module")
def cases():
    """name -> (bodies, the host packer's series), built once."""
    from krr_amd.core.prom_native import pack_query_range_bodies

    out = {}
    for name, make in LAYOUTS.items():
        bodies = make()
        out[name] = (bodies, pack_query_range_bodies(bodies))
    return out


@pytest.fixture(scope="module")
def packers():
    from krr_amd import _native
    from krr_amd.core.device_pack import DevicePacker

    ctx = _native.Context(0)
    yield {strip: DevicePacker(ctx, chunk_bytes=1 << 20, strip=strip) for strip in (True, False)}
    ctx.close()


def _same(series, want):
    """Values, offsets and the three pod fields of a device-packed series against the host's."""
    import torch

    assert np.array_equal(series.offsets.cpu().numpy(), want.offsets)
    assert np.array_equal(series.values.cpu().numpy().view(np.uint64), want.values.view(np.uint64))
    for got, ref in ((series.pod_offsets, want.pod_offsets), (series.pod_groups, want.pod_groups)):
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), ref)
    assert series.n_pods == want.n_pods
    assert series.pod_max_len == int(np.diff(want.pod_offsets).max(initial=0))


@pytest.mark.parametrize("strip,want_ts", CONFIGS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pod_fields_equal_the_host_packers(packers, cases, name, strip, want_ts):
    bodies, want = cases[name]
    dp = packers[strip].pack(bodies, want_timestamps=want_ts)
    assert dp.via == "device" and dp.host_bodies == 0
    _same(dp.series, want)
    if name == "no_kept_pod":
        assert dp.series.n_pods == 0 and dp.series.pod_max_len == 0
    if name == "block_edges":
        per_object = np.diff(want.pod_groups)
        assert {1, 63, 64, 65, 130} <= set(per_object.tolist()) and 0 in per_object


def test_parse_spans_several_launches(packers, cases):
    """The 1-MiB chunks cut the larger batches into several parse launches (what the cases above
    run under): the boundaries come from the whole batch's counts."""
    for name in ("block_edges", "fleet"):
        assert sum(len(b) for bodies in cases[name][0] for b in bodies) > 3 << 19  # > 1.5 chunks


@pytest.mark.parametrize("strip,want_ts", CONFIGS)
@pytest.mark.parametrize("pair", [("fleet", "block_edges"), ("no_kept_pod", "objects_without_bodies"),
                                  ("every_body_dropped", "no_kept_pod")])
def test_pack_many_rebases_each_resource(packers, cases, pair, strip, want_ts):
    """Two resources through one pipeline: each one's groups start at 0 and its offsets at 0."""
    got = packers[strip].pack_many([cases[n][0] for n in pair], want_timestamps=want_ts)
    for dp, n in zip(got, pair):
        assert dp.via == "device"
        _same(dp.series, cases[n][1])


@pytest.mark.parametrize("strip", [True, False])
def test_empty_batches(packers, strip):
    for bodies in ([], [[], [], []]):
        dp = packers[strip].pack(bodies)
        assert dp.via == "device"
        assert dp.series.pod_offsets.cpu().tolist() == [0]
        assert dp.series.pod_groups.cpu().tolist() == [0] * (len(bodies) + 1)
        assert dp.series.pod_max_len == 0 and dp.series.n_pods == 0


def test_host_fallback_keeps_the_host_packers_fields(packers, cases):
    """A body the device does not decide (an escaped key): that resource is the host packer's,
    numpy fields included; the other resource of the same batch stays on the device."""
    from krr_amd.core.prom_native import pack_query_range_bodies

    bodies = [list(b) for b in cases["every_body_dropped"][0]]
    bodies[0].append(_body([1.0, 2.0]).replace(b'"status"', b'"st\\u0061tus"'))
    want = pack_query_range_bodies(bodies)
    other, other_want = cases["objects_without_bodies"]
    host, dev = packers[True].pack_many([bodies, other])
    assert host.via == "host" and host.host_bodies == 1
    for got, ref in ((host.series.pod_offsets, want.pod_offsets), (host.series.pod_groups, want.pod_groups)):
        assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    assert dev.via == "device"
    _same(dev.series, other_want)


def test_null_and_negative_arguments_are_refused_before_any_launch():
    """KRR_E_INVALID from the host-side checks (nothing is launched)."""
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    lib = _native.load_library()
    z = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    s = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    p = z.data_ptr()
    bad = [
        (ctx._h, -1, p, 1, p, s.data_ptr(), p, None, p, p, None, None),   # negative objects
        (ctx._h, 1, p, -1, p, s.data_ptr(), p, None, p, p, None, None),   # negative bodies
        (ctx._h, 1, None, 1, p, s.data_ptr(), p, None, p, p, None, None),  # no body table
        (ctx._h, 1, p, 1, None, s.data_ptr(), p, None, p, p, None, None),  # no counts
        (ctx._h, 1, p, 1, p, s.data_ptr(), p, p, p, p, None, None),       # pod_groups without pod_offsets
        (ctx._h, 1, p, 1, p, s.data_ptr(), p, None, p, p, p, None),       # pod_offsets without pod_groups
        (ctx._h, 1, p, 1, p, s.data_ptr(), p, None, None, None, None, None),  # no output
    ]
    for args in bad:
        assert lib.krr_json_pod_bounds(*args) == _native.KRR_E_INVALID, args[1:4]
    assert lib.krr_json_pod_bounds(None, 1, p, 1, p, s.data_ptr(), p, None, p, p, None, None) == _native.KRR_E_INVALID
    ctx.close()

"""Pod boundaries through the packers (cpu_aggregation = "pods_max"): every host packer writes
``PackedSeries.pod_offsets`` / ``pod_groups`` with pod_offsets[pod_groups[s]] == offsets[s],
``slice_fleet`` carries and rebases them, the settings field validates, and the two new ABI
entries refuse null arguments.  No GPU."""
import ctypes
from decimal import Decimal

import numpy as np
import pytest

from krr_amd.core.models.allocations import ResourceType

# per object: the pods' sample lists in pod order (an empty list = a pod without data)
FLEET = [
    [],                                            # an object without pods
    [[], []],                                      # every pod empty: all dropped
    [[1.0, 2.0], [], [3.0]],                       # an empty pod between two pods with data
    [[0.5]],                                       # one pod
    [[1.0], [2.0, 2.5], [3.0, 3.5, 4.0], [5.0], [6.0, 7.0]],  # five pods
    [[9.0, 8.0, 7.0]],
]
KEPT = [[len(p) for p in pods if p] for pods in FLEET]


def check_invariant(ps, kept=KEPT):
    assert ps.pod_offsets is not None and ps.pod_groups is not None
    po, pg, offs = (np.asarray(a) for a in (ps.pod_offsets, ps.pod_groups, ps.offsets))
    assert po.dtype == np.int64 and pg.dtype == np.int64
    assert pg.size == offs.size and po.size == pg[-1] + 1 == ps.n_pods + 1
    assert pg[0] == 0 and po[0] == 0 and po[-1] == offs[-1]
    assert np.array_equal(po[pg], offs)  # the invariant, the last entry included
    assert np.array_equal(np.diff(pg), [len(k) for k in kept])
    assert np.array_equal(np.diff(po), [n for k in kept for n in k])


def histories():
    return [{ResourceType.CPU: {f"p{i}": [Decimal(repr(x)) for x in pod] for i, pod in enumerate(pods)},
             ResourceType.Memory: {f"p{i}": [Decimal(int(x * 1000)) for x in pod] for i, pod in enumerate(pods)}}
            for pods in FLEET]


def test_pack_histories_native_and_python_paths(monkeypatch):
    from krr_amd.core import packing

    fleet = packing.pack_histories(histories())
    check_invariant(fleet.cpu)
    monkeypatch.setattr(packing, "_PYDEC", None)  # the pure-Python walk
    fleet_py = packing.pack_histories(histories())
    check_invariant(fleet_py.cpu)
    assert np.array_equal(fleet.cpu.values, fleet_py.cpu.values)
    assert np.array_equal(fleet.cpu.pod_offsets, fleet_py.cpu.pod_offsets)
    # an exact (class >= 1) history keeps its pod lists, one per pod segment
    hs = histories()
    hs[2][ResourceType.CPU]["p0"][0] = Decimal("1.00")
    ps = packing.pack_resource(hs, ResourceType.CPU)
    check_invariant(ps)
    view = packing.pod_view(ps)
    assert view.n_segments == ps.n_pods and view.exact is not None
    j = int(ps.pod_groups[2])
    assert view.exact[j] and view.sources[j] == (hs[2][ResourceType.CPU]["p0"],)
    assert view.sources[j + 1] == (hs[2][ResourceType.CPU]["p2"],)


def prom_result(pod):
    return [{"metric": {}, "values": [[1700000000 + 60 * i, repr(x)] for i, x in enumerate(pod)]}] if pod else []


def test_pack_prometheus():
    from krr_amd.core.packing import pack_prometheus

    check_invariant(pack_prometheus([[prom_result(p) for p in pods] for pods in FLEET]))


def test_pack_dense_grid_pods_are_slots():
    from krr_amd.core.packing import pack_dense_grid

    slots = 6
    per_object = [[(np.arange(len(p), dtype=np.float64) * 60.0, np.asarray(p, dtype=np.float64)) for p in pods]
                  for pods in FLEET]
    ps = pack_dense_grid(per_object, 0.0, 60.0, slots)
    # every pod is a pod segment of `slots` slots, present samples or not
    check_invariant(ps, [[slots] * len(pods) for pods in FLEET])
    assert ps.gaps_are_nan


def body(pod):
    vals = ",".join(f'[{1700000000 + 60 * i},"{float(x)!r}"]' for i, x in enumerate(pod))
    series = '{"metric":{},"values":[' + vals + ']}' if pod else ""
    return ('{"status":"success","data":{"resultType":"matrix","result":[' + series + ']}}').encode()


def test_pack_query_range_bodies():
    from krr_amd.core.prom_native import pack_query_range_bodies

    bodies = [[body(p) for p in pods] for pods in FLEET]
    ps, counts = pack_query_range_bodies(bodies, return_pod_counts=True)
    check_invariant(ps)
    assert counts.tolist() == [len(p) if p else -1 for pods in FLEET for p in pods]
    check_invariant(pack_query_range_bodies(bodies))  # without the counts returned, too


def test_slice_fleet_rebases_pod_fields():
    from krr_amd.core.distributed import slice_fleet
    from krr_amd.core.packing import pack_histories

    fleet = pack_histories(histories())
    assert fleet.n_objects == 6
    whole = np.diff(fleet.cpu.pod_offsets)
    for cuts in ([0, 2, 3, 6], [0, 1, 5, 6], [0, 6], [0, 0, 4, 4, 6]):
        lens = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = slice_fleet(fleet, lo, hi)
            check_invariant(part.cpu, KEPT[lo:hi])
            lens.append(np.diff(part.cpu.pod_offsets))
            for j in range(part.cpu.n_pods):  # the same samples under the rebased offsets
                a, b = part.cpu.pod_offsets[j:j + 2]
                g = int(fleet.cpu.pod_groups[lo]) + j
                assert np.array_equal(part.cpu.values[a:b],
                                      fleet.cpu.values[fleet.cpu.pod_offsets[g]:fleet.cpu.pod_offsets[g + 1]])
        assert np.array_equal(np.concatenate(lens), whole)


def test_pod_view_names_the_packer_without_pod_fields():
    from krr_amd.core.packing import PackedSeries, pod_view

    ps = PackedSeries(np.zeros(3), np.array([0, 3], dtype=np.int64), 3)  # positional, as before
    assert ps.pod_offsets is None and ps.pod_groups is None and ps.n_pods == 0
    with pytest.raises(ValueError, match="device packer"):
        pod_view(ps)


def test_settings_field():
    import pydantic.v1 as pd

    from krr_amd.strategies.simple import CpuAggregation, SimpleStrategySettings
    from krr_amd.strategies.simple_limit import SimpleLimitStrategySettings

    assert SimpleStrategySettings().cpu_aggregation == CpuAggregation.CONCAT == "concat"
    assert SimpleStrategySettings().aggregation() == "concat"
    st = SimpleStrategySettings(cpu_aggregation="pods_max")
    assert st.cpu_aggregation is CpuAggregation.PODS_MAX and st.aggregation() == "pods_max"
    with pytest.raises(pd.ValidationError):
        SimpleStrategySettings(cpu_aggregation="pods_mean")
    assert SimpleLimitStrategySettings().simple_settings().aggregation() == "concat"


def test_new_entry_points_refuse_null_arguments():
    from krr_amd import _native

    lib = _native.load_library(require_torch=False)
    assert "krr_group_max" in _native.EXPORTED_SYMBOLS and "krr_simple_run_pods" in _native.EXPORTED_SYMBOLS
    assert lib.krr_group_max(None, 0, None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert lib.krr_simple_run_pods(None, None, None, None, None, None, None, None, None, None, None, None, None,
                                   None, None, None, None) == -1
    assert lib.krr_abi_version() == 3 and ctypes.sizeof(_native.KrrSeries) == 48

"""krr_multi_plan (host only): which path a multi-percentile launch takes, and its argument checks.

The shared rows were worked out from krr_plan.h's rules (plan_side per percentile, the max of the
tops / bottoms, capacity_for, single_pass_ok) by hand before the code existed; they pin the rule,
not the implementation.  No GPU: krr_multi_plan needs no device and no ctx."""
import ctypes
from decimal import Decimal

import pytest


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g

    g.build()
    from krr_amd import _native

    _native.load_library()
    return _native


def _params(ps, mode):
    from krr_amd.core.engine import percentile_params

    return [percentile_params(Decimal(str(p)), mode) for p in ps]


@pytest.mark.parametrize("L,ps,tkeep,cap,bottom", [
    (6000, (95, 99), 303, 1088, 0),
    (6000, (1, 5), 303, 1088, 1),
    (1345, (5, 95), 1280, 1920, 0),
    (4035, (66, 96), 1375, 2048, 0),
    (70000, (97, 99), 2103, 2752, 0),
    (20160, (95, 99), 1011, 1664, 0),
])
def test_shared_plans(native, L, ps, tkeep, cap, bottom):
    info = native.multi_plan(L, _params(ps, "sorted_lower"))
    assert (info.shared, info.tkeep, info.cap_keys, info.bottom) == (1, tkeep, cap, bottom)
    assert info.lds_bytes == 1536 + 8 * cap
    # the order of the set does not matter, and a duplicate changes nothing
    again = native.multi_plan(L, _params(tuple(reversed(ps)) + (ps[0],), "sorted_lower"))
    assert (again.shared, again.tkeep, again.cap_keys, again.bottom) == (1, tkeep, cap, bottom)


@pytest.mark.parametrize("L,ps", [(70000, (95, 99)), (70000, (50, 99)), (10080, (66, 96)), (5380, (66, 96))])
def test_sets_that_fall_back(native, L, ps):
    info = native.multi_plan(L, _params(ps, "sorted_lower"))
    assert (info.shared, info.tkeep, info.cap_keys, info.lds_bytes) == (0, 0, 0, 0)


def test_shared_buffer_is_the_innermost_percentiles(native):
    """The set's buffer is the single plan of its innermost percentile (top side: the lowest)."""
    for L, ps in ((6000, (95, 99)), (20160, (95, 97, 99, 100)), (6000, (1, 5))):
        multi = native.multi_plan(L, _params(ps, "linear"))
        inner = min(ps) if not multi.bottom else max(ps)
        one = native.select_plan(L, _params((inner,), "linear")[0])
        assert multi.shared == 1 and (multi.tkeep, multi.bottom) == (one.tkeep, one.bottom)


def test_index_table_widens_the_plan(native):
    plain = native.multi_plan(6000, _params((95, 99), "sorted_lower"))
    tabled = native.multi_plan(6000, _params(("99.99999999999999999999999999", 95), "sorted_lower"))
    assert tabled.shared == 1 and tabled.tkeep == plain.tkeep  # p95 is the innermost: no table there
    # alone, the tabled percentile keeps plan_side's two extra keys: k(L) is L - 2 or L - 1 (p within
    # 1e-15 of 100), so L - k + 2 + 2 is 5 or 6, against 3 or 4 without the table's margin
    lone = native.multi_plan(6000, _params(("99.99999999999999999999999999",), "sorted_lower"))
    one = native.select_plan(6000, _params(("99.99999999999999999999999999",), "sorted_lower")[0])
    assert lone.shared == 1 and lone.tkeep == one.tkeep and lone.tkeep in (5, 6)


@pytest.mark.parametrize("L", [1, 1440, 10080, 70000, 500000])
def test_ref_index_always_shares(native, L):
    for ps in ((66, 96), (50, 99), (1, 50, 99, 100)):
        info = native.multi_plan(L, _params(ps, "ref_index"))
        assert (info.shared, info.cap_keys, info.lds_bytes) == (1, 0, 0)


def test_argument_checks(native):
    with pytest.raises(native.NativeError) as ei:
        native.multi_plan(6000, [])
    assert ei.value.code == native.KRR_E_INVALID
    with pytest.raises(native.NativeError) as ei:
        native.multi_plan(6000, _params((90, 95, 97, 99, 100), "linear"))
    assert ei.value.code == native.KRR_E_INVALID
    mixed = _params((95,), "linear") + _params((99,), "sorted_lower")
    with pytest.raises(native.NativeError) as ei:
        native.multi_plan(6000, mixed)
    assert ei.value.code == native.KRR_E_INVALID
    lib = native.load_library()
    info = native.KrrMultiPlanInfo()
    one = _params((99,), "linear")[0]
    assert lib.krr_multi_plan(-1, ctypes.byref(one), 1, ctypes.byref(info)) == native.KRR_E_INVALID
    assert lib.krr_multi_plan(100, None, 1, ctypes.byref(info)) == native.KRR_E_INVALID
    assert lib.krr_multi_plan(100, ctypes.byref(one), 1, None) == native.KRR_E_INVALID
    bad = native.KrrPercentileParams(native.KRR_PCT_LINEAR, 0, 101, 1, 1.01)
    assert lib.krr_multi_plan(100, ctypes.byref(bad), 1, ctypes.byref(info)) == native.KRR_E_INVALID


def test_null_handling_and_layout(native):
    lib = native.load_library()
    assert ctypes.sizeof(native.KrrMultiPlanInfo) == 4 * 2 + 8 * 3
    assert native.KRR_MAX_PERCENTILES == 4
    assert lib.krr_segmented_percentiles(None, None, None, 2, None, None, None, None) == native.KRR_E_INVALID
    assert lib.krr_simple_run_multi(None, None, None, None, 2, None, None, None, None, None, None,
                                    None) == native.KRR_E_INVALID


def test_single_percentile_plan_matches_select_plan(native):
    """P = 1: the same side and keys as krr_select_plan wherever that plan is a single pass."""
    for L, p in ((50400, "99"), (20160, "97"), (10080, "95"), (50400, "1")):
        one = native.select_plan(L, _params((p,), "linear")[0])
        multi = native.multi_plan(L, _params((p,), "linear"))
        assert one.hselect == 0 and multi.shared == 1
        assert (multi.tkeep, multi.bottom, multi.cap_keys, multi.lds_bytes) == \
            (one.tkeep, one.bottom, one.cap_keys, one.lds_bytes)

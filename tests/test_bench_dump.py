"""bench.py --dump-outputs on CPU: the files are float64, small outputs are written whole, and
past the 64 MB budget every array keeps the same seeded rows, run after run."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    v = np.array([0.25, np.nan, -0.0, 3e8])
    bench.dump_outputs(str(tmp_path / "d"), {"value": v, "count": np.array([3, 0, 1, 50400], dtype=np.int64),
                                             "flags": np.array([0, 1, 0, 0], dtype=np.uint32)})
    got = _load(tmp_path / "d")
    assert sorted(got) == ["count", "flags", "value"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["value"].view(np.uint64), v.view(np.uint64))
    assert got["count"].tolist() == [3, 0, 1, 50400] and got["flags"].tolist() == [0, 1, 0, 0]


def test_large_outputs_keep_the_same_seeded_rows(tmp_path):
    n = 1_000_000  # config 4's fleet: 12 arrays x 8 MB is past the budget
    arrays = {f"a{i}": np.arange(n, dtype=np.int64) * (i + 1) for i in range(12)}
    arrays["own"] = np.arange(1000, dtype=np.int64)  # a shorter array under the cap stays whole
    for name in ("x", "y"):
        bench.dump_outputs(str(tmp_path / name), arrays)
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert sorted(x) == sorted(y) == sorted([*arrays, f"rows_{n}"])
    assert all(np.array_equal(x[k], y[k]) for k in x)
    total = sum(os.path.getsize(os.path.join(tmp_path / "x", f)) for f in os.listdir(tmp_path / "x"))
    assert total <= bench.DUMP_BUDGET
    rows = x[f"rows_{n}"]
    assert rows.size < n and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    for i in range(12):
        assert np.array_equal(x[f"a{i}"], rows * (i + 1))
    assert np.array_equal(x["own"], np.arange(1000))

"""Every output bit of the four per-series fleet kernels on one fixed small world, for checking
that a change to their shared scaffolding (krr_geom.h, the SeriesArgs frame) moved none of them:

    python scripts/fleet_bits.py OUT.npz          # run on the GPU, write every output array
    python scripts/fleet_bits.py --compare A B    # byte-compare two such files, array by array

Run it on the parent commit and on the result and compare.  The world: segment lengths
[0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17], each at an even
and at an odd start (one-slot filler segments set the parity), as a compact series (one segment
with a NaN sample) and as a NaN-gapped one, +0.0 and -0.0 samples in both, seed 20.  Floats are
stored as their uint64 bits, so NaN payloads compare too."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17]
WINDOWS = (1, 2, 5, 128, 1440)


def world():
    """(values, offsets): every length at both start parities."""
    lens, at = [], 0
    for L in LENGTHS:
        for parity in (0, 1):
            if at % 2 != parity:
                lens.append(1)
                at += 1
            lens.append(L)
            at += L
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(20)
    vals = rng.gamma(2.0, 0.05, size=int(offs[-1]))
    vals[rng.random(vals.size) < 0.03] = 0.0
    vals[rng.random(vals.size) < 0.03] = -0.0
    return vals, offs


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64) if a.dtype == np.float64 else a


def run(out_path: str) -> None:
    import torch

    from krr_amd import _native
    from krr_amd.core.engine import SimpleEngine
    from krr_amd.core.packing import PackedSeries

    vals, offs = world()
    S, longest = offs.size - 1, int(np.diff(offs).max())
    rng = np.random.default_rng(21)
    compact = vals.copy()
    s_nan = int(np.flatnonzero(np.diff(offs) == 1025)[0])
    compact[offs[s_nan] + 700] = np.nan
    gapped = vals.copy()
    gapped[rng.random(vals.size) < 0.1] = np.nan
    gapped[offs[s_nan]:offs[s_nan + 1]] = np.nan  # a segment of gaps only
    thr = np.stack([np.full(S, q) for q in (0.05, 0.1, 0.2, np.inf)])
    thr[1, ::3] = np.nan
    eng = SimpleEngine(0)
    ctx = eng.context()
    dev = torch.device("cuda", 0)
    res = {}

    def keep(tag, d):
        for k, v in d.items():
            res[f"{tag}.{k}"] = bits(v)

    for name, ps in (("compact", PackedSeries(compact, offs, longest, False)),
                     ("gapped", PackedSeries(gapped, offs, longest, True))):
        keep(f"{name}.stats", eng.stats_series(ps))
        keep(f"{name}.moments", eng.moments_series(ps, trend=True))
        keep(f"{name}.moments_notrend", eng.moments_series(ps, trend=False))
        keep(f"{name}.exceed1", eng.exceed_series(ps, thr[:1]))
        keep(f"{name}.exceed4", eng.exceed_series(ps, thr))
        for W in WINDOWS:
            for aname, align in (("start", _native.KRR_ROLLUP_START), ("end", _native.KRR_ROLLUP_END)):
                keep(f"{name}.rollup{W}{aname}", eng.rollup_series(ps, W, align))
                # without the extrema: the engine always asks for them, so this goes to the entry point
                series = eng._part_series(ctx, ps)
                wo = np.concatenate([[0], np.cumsum(-(-np.diff(offs) // W))]).astype(np.int64)
                o = {"wcount": torch.empty(int(wo[-1]), dtype=torch.int32, device=dev),
                     "sum": torch.empty(int(wo[-1]), dtype=torch.float64, device=dev),
                     "count": torch.empty(S, dtype=torch.int64, device=dev),
                     "flags": torch.empty(S, dtype=torch.int32, device=dev)}
                ctx.segmented_rollup(series, W, align, torch.from_numpy(wo).to(dev), None, None, o["sum"],
                                     o["wcount"], o["count"], o["flags"])
                torch.cuda.synchronize()
                keep(f"{name}.rollup{W}{aname}_nomm", o)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **res)
    print(f"{len(res)} arrays, {sum(v.nbytes for v in res.values())} bytes -> {out_path}")


def compare(a_path: str, b_path: str) -> int:
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    print(f"{len(a.files)} / {len(b.files)} arrays, {len(bad)} differ" + (": " + ", ".join(bad[:10]) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run(sys.argv[1] if len(sys.argv) > 1 else "fleet_bits.npz")

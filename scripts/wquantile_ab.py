"""Same-process A/B of krr_segmented_wquantile (k_wquantile) against krr_segmented_stats (k_stats: ONE
pass over the same bytes, the byte floor of a pass) and, beside it, krr_segmented_percentile
SORTED_LOWER p95 (the flat exact select) on the same buffers.

    python scripts/wquantile_ab.py [--out profiles/wquantile] [--shapes NAME ...] [--iters 10] [--reps 7]
                                   [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/exceed_ab.py: the bench's config-3 memory series
(100,000 compact segments of 1-14 days @1m) and its config-2 CPU series (10,000 NaN-gapped segments
of 50,400 slots).  Tables: decay_weights with a one-day (1,440 slots) and a one-hour (60 slots)
half-life over the longest segment, at p95.  Before timing, every wquantile launch's count / flags
must equal k_stats' bit for bit, two launches must give equal bits, and the unit-weight launch at
p100 must equal k_stats' maximum as a number.  Each leg is warmed up, then timed with HIP events
`--iters` times per repetition, the legs alternating; `--reps` repetitions give each leg's
per-repetition medians, their median and their min-max.  Reported: ms, the ratio of each leg to
k_stats, the mean and the maximum of out_passes and its histogram.  There is no threshold on the
ratios.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)
from pods_ab import SLOTS_7D  # noqa: E402
from stats_ab import same  # noqa: E402

# name -> (length rule, segments, gapped, pod_len, krr_synth_fill kind: 0 CPU, 1 memory)
SHAPES = {
    "config3_memory_compact": ("config3", 100_000, False, 0, 1),
    "config2_cpu_gapped": ("config2", 10_000, True, SLOTS_7D, 0),
}
HALF_LIVES = {"day": 1440, "hour": 60}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/wquantile")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="segments x this (rehearsals)")
    ap.add_argument("--name", default="ab")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from krr_amd import _native
    from krr_amd.api import decay_weights

    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        kind, n, gaps, pod_len, fill = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        vals = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(vals, offs, 1234 if fill == 0 else 1234 ^ 0x5A5A, fill, pod_len, gaps)
        series = ctx.series(vals, offs, Lmax, gaps)

        def table(t):
            return torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)).to(dev)

        def outs():
            return {"value": torch.empty(S, dtype=torch.float64, device=dev),
                    "wsum": torch.empty(S, dtype=torch.int64, device=dev),
                    "passes": torch.empty(S, dtype=torch.int32, device=dev),
                    "count": torch.empty(S, dtype=torch.int64, device=dev),
                    "flags": torch.empty(S, dtype=torch.int32, device=dev)}

        os_ = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("min", torch.float64), ("max", torch.float64), ("sum", torch.float64), ("count", torch.int64),
                ("flags", torch.int32))}
        flat = {"value": torch.empty(S, dtype=torch.float64, device=dev), "count": torch.empty(S, dtype=torch.int64, device=dev),
                "flags": torch.empty(S, dtype=torch.int32, device=dev)}
        p95 = _native.KrrPercentileParams(_native.KRR_PCT_SORTED_LOWER, 0, 95, 1, 0.95)

        def leg_stats():
            ctx.segmented_stats(series, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def leg_flat():
            ctx.segmented_percentile(series, p95, flat["value"], flat["count"], flat["flags"])

        def wq_leg(d_tab, num=95, den=1):
            o = outs()

            def run(o=o):
                ctx.segmented_wquantile(series, d_tab, num, den, o["value"], o["wsum"], o["passes"], o["count"], o["flags"])
            return run, o

        legs, results = {"k_stats": leg_stats, "flat_sorted_lower_p95": leg_flat}, {}
        for hn, h in HALF_LIVES.items():
            legs[f"k_wquantile_{hn}_p95"], results[f"k_wquantile_{hn}_p95"] = wq_leg(table(decay_weights(h, Lmax)))
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        passes = {}
        for k, o in results.items():
            assert same(o["count"], os_["count"]) and same(o["flags"], os_["flags"]), "count / flags differ from k_stats"
            again = outs()
            legs[k](again)
            torch.cuda.synchronize()
            assert all(same(again[f], o[f]) for f in o), "two launches differ"
            p = o["passes"].cpu().numpy()
            passes[k] = {"mean": round(float(p.mean()), 4), "max": int(p.max()), "histogram": np.bincount(p).tolist(),
                         "segments_without_weight": int((o["wsum"] == 0).sum().item())}
        unit_run, unit = wq_leg(table([1]), 100, 1)  # unit weights at p100: the maximum
        unit_run()
        torch.cuda.synchronize()
        live = os_["flags"] == 0
        assert bool((unit["value"][live] == os_["max"][live]).all()), "unit-weight p100 is not the maximum"
        assert same(unit["wsum"], os_["count"] * live), "unit-weight wsum is not the count"
        meds = {k: [] for k in legs}
        for _ in range(args.reps):
            ev = {k: [] for k in legs}
            for _ in range(args.iters):
                for k, f in legs.items():  # alternating legs
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            for k in legs:
                meds[k].append(float(np.median([a.elapsed_time(b) for a, b in ev[k]])))
        med = {k: float(np.median(v)) for k, v in meds.items()}
        row = {"segments": S, "slots": N, "present_samples": int(os_["count"].sum().item()), "gapped": bool(gaps),
               "longest_segment": Lmax, "table_bytes": 8 * Lmax,
               "count_and_flags_equal_k_stats": True, "two_launches_equal_bits": True, "unit_p100_equals_max": True,
               "passes": passes,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"},
               "over_k_stats_per_pass": {k: round(med[k] / med["k_stats"] / passes[k]["mean"], 4) for k in passes}}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("passes", "median_of_medians_ms", "min_max_ms", "over_k_stats",
                                                    "over_k_stats_per_pass")}), flush=True)
        del vals, series, os_, results, legs, flat, unit
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

"""Same-process A/B of krr_segmented_moments (k_moments<true>: with the trend, k_moments<false>:
mean and m2 only) against krr_segmented_stats (k_stats) on the same buffers: all three read every
value once through the same streaming loop; they differ in the arithmetic per slot.

    python scripts/moments_ab.py [--out profiles/moments] [--shapes NAME ...] [--iters 10] [--reps 7]
                                 [--scale 1.0]

Shapes and protocol are scripts/stats_ab.py's: the bench's config-3 memory series (100,000 compact
segments of 1-14 days @1m) and its config-2 memory series (10,000 NaN-gapped segments of 50,400
slots), from krr_synth_fill (seeded).  Before timing, both moments launches' count / flags must
equal k_stats' bit for bit, the launch without the trend must give the full launch's mean and m2
bit for bit, and two full launches must give equal bits in every output.  Each leg is warmed up,
then timed with HIP events `--iters` times per repetition, the legs alternating; `--reps`
repetitions give each leg's per-repetition medians, their median and their min-max.  Reported: ms,
effective bandwidth, and the ratio of each moments leg to k_stats.  There is no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)
from pods_ab import SHAPES  # noqa: E402
from stats_ab import same  # noqa: E402

MOMENTS = ("mean", "m2", "tmean", "t2", "cxt")
# per segment: 8 B offset in; 8 B count + 4 B flags out, plus 8 B per float64 output
OUT_BYTES = {"k_stats": 8 + 12 + 24, "k_moments_trend": 8 + 12 + 40, "k_moments_no_trend": 8 + 12 + 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/moments")
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

    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        kind, n, gaps, pod_len = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        mem = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(mem, offs, 1234 ^ 0x5A5A, 1, pod_len, gaps)
        ms = ctx.series(mem, offs, Lmax, gaps)

        def outs(names):
            return {k: torch.empty(S, dtype={"count": torch.int64, "flags": torch.int32}.get(k, torch.float64),
                                   device=dev) for k in names}

        os_ = outs(("min", "max", "sum", "count", "flags"))
        full, full2, light = (outs(MOMENTS + ("count", "flags")) for _ in range(3))

        def leg_stats():
            ctx.segmented_stats(ms, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def leg_trend(o=full):
            ctx.segmented_moments(ms, o["mean"], o["m2"], o["tmean"], o["t2"], o["cxt"], o["count"], o["flags"])

        def leg_no_trend():
            ctx.segmented_moments(ms, light["mean"], light["m2"], None, None, None, light["count"], light["flags"])

        legs = {"k_stats": leg_stats, "k_moments_trend": leg_trend, "k_moments_no_trend": leg_no_trend}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        leg_trend(full2)
        torch.cuda.synchronize()
        for o in (full, light):
            assert same(o["count"], os_["count"]) and same(o["flags"], os_["flags"]), "count / flags differ from k_stats"
        assert same(light["mean"], full["mean"]) and same(light["m2"], full["m2"]), "no-trend launch differs"
        assert all(same(full[k], full2[k]) for k in full), "two launches differ"
        present = int(os_["count"].sum().item())
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
        row = {"segments": S, "slots": N, "present_samples": present, "gapped": bool(gaps),
               "count_and_flags_equal_k_stats": True, "no_trend_mean_m2_equal_full_launch": True,
               "two_launches_equal_bits": True,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "effective_GBps": {k: round((8 * N + OUT_BYTES[k] * S) / med[k] / 1e6, 1) for k in legs},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"}}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("median_of_medians_ms", "min_max_ms", "effective_GBps",
                                                    "over_k_stats")}), flush=True)
        del mem, ms, os_, full, full2, light
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

"""Same-process A/B of krr_segmented_stats (k_stats) against krr_segmented_max (k_max) on the
same buffers: both read every value once, k_stats also keeps the min and the sum.

    python scripts/stats_ab.py [--out profiles/fleet_stats] [--shapes NAME ...] [--iters 10] [--reps 7]
                               [--scale 1.0]

Shapes: the bench's config-3 memory series (100,000 compact segments of 1-14 days @1m) and its
config-2 memory series (10,000 NaN-gapped segments of 50,400 slots), from krr_synth_fill (seeded).
Before timing, k_stats' max / count / flags must equal k_max's bit for bit, and two k_stats
launches must give equal bits in every output.  Each leg is warmed up, then timed with HIP events
`--iters` times per repetition, the legs alternating; `--reps` repetitions give each leg's
per-repetition medians, their median, and their min-max.  Reported: the ratio stats / max of the
medians, the effective bandwidth of both, and whether k_stats' median lies inside k_max's own
min-max over the repetitions.  There is no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)
from pods_ab import SHAPES  # noqa: E402


def same(a, b):
    import torch

    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                       b.view(torch.int64) if b.dtype == torch.float64 else b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fleet_stats")
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

        om = outs(("value", "count", "flags"))
        os_, os2 = outs(("min", "max", "sum", "count", "flags")), outs(("min", "max", "sum", "count", "flags"))

        def leg_max():
            ctx.segmented_max(ms, om["value"], om["count"], om["flags"])

        def leg_stats(o=os_):
            ctx.segmented_stats(ms, o["min"], o["max"], o["sum"], o["count"], o["flags"])

        legs = {"k_max": leg_max, "k_stats": leg_stats}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        leg_stats(os2)
        torch.cuda.synchronize()
        assert same(os_["max"], om["value"]) and same(os_["count"], om["count"]) and same(os_["flags"], om["flags"])
        assert all(same(os_[k], os2[k]) for k in os_), "two launches differ"
        present = int(om["count"].sum().item())
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
               "max_and_count_and_flags_equal_k_max": True, "two_launches_equal_bits": True,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               # 8 B per slot + 8 B offset per segment in; 20 B (k_max) / 36 B (k_stats) out per segment
               "effective_GBps": {"k_max": round((8 * N + 28 * S) / med["k_max"] / 1e6, 1),
                                  "k_stats": round((8 * N + 44 * S) / med["k_stats"] / 1e6, 1)},
               "stats_over_max": round(med["k_stats"] / med["k_max"], 4),
               "stats_median_inside_k_max_min_max": bool(min(meds["k_max"]) <= med["k_stats"] <= max(meds["k_max"]))}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("median_of_medians_ms", "min_max_ms", "effective_GBps",
                                                    "stats_over_max", "stats_median_inside_k_max_min_max")}), flush=True)
        del mem, ms, om, os_, os2
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

"""Same-process A/B of krr_segmented_slide (k_slide) against krr_segmented_stats (k_stats) and
krr_segmented_rollup (k_rollup) on the same buffers: all three read every value once through the
streaming skeleton; they differ in the work per slot (k_slide: two scan steps and an LDS round
trip per step of at most 64 slots) and in what they write (k_slide: up to 36 bytes per SLOT).

    python scripts/slide_ab.py [--out profiles/slide] [--shapes NAME ...] [--windows 5 60 1440]
                               [--iters 5] [--reps 5] [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/rollup_ab.py: the bench's config-3 memory series
(100,000 compact segments of 1-14 days @1m) and its config-2 CPU series (10,000 NaN-gapped segments
of 50,400 slots).  Legs: k_stats (the yardstick reading the same bytes) and, for every window W,
k_rollup at W (end-aligned, all four outputs), k_slide with the mean only, with all five per-slot
outputs, and with no per-slot output (the peak alone); min_count = ceil(W / 2).  Before timing, on
the buffers: every slide launch's count / flags must equal k_stats' bit for bit, two launches must
give equal bits, and the mean-only and peak-only launches must equal the full one in what they
write.  Each leg is warmed up, then timed with HIP events `--iters` times per repetition, the legs
alternating; `--reps` repetitions give each leg's per-repetition medians, their median and their
min-max.  Reported: ms, effective bandwidth counting the written bytes, the ratio of each leg to
k_stats, and beside it the byte floor (bytes read + bytes written) / bytes read, derived from the
shape: the ratio a kernel at k_stats' bandwidth would have.  There is no threshold on the ratios.
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
SLOT = ("mean", "sum", "max", "min", "wcount")
ROLL = ("min", "max", "sum", "wcount")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/slide")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--windows", nargs="*", type=int, default=[5, 60, 1440])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
        kind, n, gaps, pod_len, fill = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        vals = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(vals, offs, 1234 if fill == 0 else 1234 ^ 0x5A5A, fill, pod_len, gaps)
        series = ctx.series(vals, offs, Lmax, gaps)
        os_ = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("min", torch.float64), ("max", torch.float64), ("sum", torch.float64), ("count", torch.int64),
                ("flags", torch.int32))}

        def leg_stats():
            ctx.segmented_stats(series, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def outs():  # one set serves every leg: the legs run one after the other on one stream
            o = {k: torch.empty(N, dtype=torch.int32 if k == "wcount" else torch.float64, device=dev) for k in SLOT}
            o.update(peak=torch.empty(S, dtype=torch.float64, device=dev),
                     peak_slot=torch.empty(S, dtype=torch.int64, device=dev),
                     count=torch.empty(S, dtype=torch.int64, device=dev),
                     flags=torch.empty(S, dtype=torch.int32, device=dev))
            return o

        a, b = outs(), outs()
        woffs, nwin = {}, {}
        for W in args.windows:
            wo = np.concatenate([[0], np.cumsum(-(-lens.astype(np.int64) // W))]).astype(np.int64)
            woffs[W], nwin[W] = torch.from_numpy(wo).to(dev), int(wo[-1])

        def slide(W, o, want=SLOT):
            ctx.segmented_slide(series, W, -(-W // 2), *(o[k] if k in want else None for k in SLOT), o["peak"],
                                o["peak_slot"], o["count"], o["flags"])

        def rollup(W):  # into the slide's per-slot buffers: a window per W slots fits
            ctx.segmented_rollup(series, W, 1, woffs[W], *(a[k] for k in ROLL), a["count"], a["flags"])

        leg_stats()
        torch.cuda.synchronize()
        legs, io = {"k_stats": leg_stats}, {"k_stats": (8 + 12 + 24) * S}
        for W in args.windows:
            # the checks, on the buffers that are timed
            for o in (a, b):
                for t in o.values():
                    t.fill_(-7)
            slide(W, a)
            slide(W, b)
            torch.cuda.synchronize()
            assert same(a["count"], os_["count"]) and same(a["flags"], os_["flags"]), "count / flags differ from k_stats"
            assert all(same(a[k], b[k]) for k in a), "two launches differ"
            for want in (("mean",), ()):
                for t in b.values():
                    t.fill_(-7)
                slide(W, b, want=want)
                torch.cuda.synchronize()
                assert all(same(a[k], b[k]) for k in want + ("peak", "peak_slot", "count", "flags")), "launch differs"
                assert all(bool((b[k] == -7).all().item()) for k in SLOT if k not in want), "a NULL output was written"
            legs[f"k_rollup_w{W}"] = lambda W=W: rollup(W)
            legs[f"k_slide_w{W}_mean"] = lambda W=W: slide(W, b, want=("mean",))
            legs[f"k_slide_w{W}_all"] = lambda W=W: slide(W, b)
            legs[f"k_slide_w{W}_peak"] = lambda W=W: slide(W, b, want=())
            # per segment: 8 B offset in (+ 16 B window offsets for the rollup), 12 B out (+ 16 B peak and slot);
            # per window 28 B out; per slot 8 B (mean) or 36 B (all five) out
            io[f"k_rollup_w{W}"] = (24 + 12) * S + 28 * nwin[W]
            io[f"k_slide_w{W}_mean"] = (8 + 28) * S + 8 * N
            io[f"k_slide_w{W}_all"] = (8 + 28) * S + 36 * N
            io[f"k_slide_w{W}_peak"] = (8 + 28) * S
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
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
                meds[k].append(float(np.median([x.elapsed_time(y) for x, y in ev[k]])))
        med = {k: float(np.median(v)) for k, v in meds.items()}
        row = {"segments": S, "slots": N, "present_samples": present, "gapped": bool(gaps),
               "windows": {str(W): nwin[W] for W in args.windows},
               "count_and_flags_equal_k_stats": True, "two_launches_equal_bits": True,
               "mean_only_and_peak_only_equal_the_full_launch": True,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "effective_GBps": {k: round((8 * N + io[k]) / med[k] / 1e6, 1) for k in legs},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"},
               "byte_floor": {k: round((8 * N + io[k]) / (8 * N + io["k_stats"]), 4) for k in legs if k != "k_stats"}}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("median_of_medians_ms", "min_max_ms", "effective_GBps",
                                                    "over_k_stats", "byte_floor")}), flush=True)
        del vals, series, os_, legs, a, b, woffs
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

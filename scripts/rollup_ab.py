"""Same-process A/B of krr_segmented_rollup (k_rollup) against krr_segmented_stats (k_stats) on the
same buffers: both read every value once through the streaming skeleton; they differ in the work
per row of 128 slots (a row in which a window closes takes a segmented scan) and in what they
write (one record per window instead of one per segment).

    python scripts/rollup_ab.py [--out profiles/rollup] [--shapes NAME ...] [--windows 5 60 1440]
                                [--iters 10] [--reps 7] [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/exceed_ab.py: the bench's config-3 memory series
(100,000 compact segments of 1-14 days @1m) and its config-2 CPU series (10,000 NaN-gapped segments
of 50,400 slots).  Legs: k_stats, and k_rollup for every window, both alignments, with all four
per-window outputs ("all") and with wsum + wcount only ("sumcnt", what a mean needs).  Before
timing, on the buffers: every rollup launch's count / flags must equal k_stats' bit for bit, two
launches must give equal bits, and the sumcnt launch must equal the full one in what it writes.
Each leg is warmed up, then timed with HIP events `--iters` times per repetition, the legs
alternating; `--reps` repetitions give each leg's per-repetition medians, their median and their
min-max.  Reported: ms, effective bandwidth counting the written bytes, and the ratio of each leg
to k_stats.  There is no threshold on the ratios.
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
STATS = ("min", "max", "sum", "wcount")
ALIGNS = {"start": 0, "end": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rollup")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--windows", nargs="*", type=int, default=[5, 60, 1440])
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

        woffs, nwin = {}, {}
        for W in args.windows:
            wo = np.concatenate([[0], np.cumsum(-(-lens.astype(np.int64) // W))]).astype(np.int64)
            woffs[W], nwin[W] = torch.from_numpy(wo).to(dev), int(wo[-1])
        most = max(nwin.values())

        def outs():  # one set serves every leg: the legs run one after the other on one stream
            o = {k: torch.empty(most, dtype=torch.int32 if k == "wcount" else torch.float64, device=dev) for k in STATS}
            o["count"] = torch.empty(S, dtype=torch.int64, device=dev)
            o["flags"] = torch.empty(S, dtype=torch.int32, device=dev)
            return o

        a, b = outs(), outs()

        def launch(W, align, o, want=STATS):
            ctx.segmented_rollup(series, W, align, woffs[W], *(o[k] if k in want else None for k in STATS),
                                 o["count"], o["flags"])

        leg_stats()
        torch.cuda.synchronize()
        legs, io = {"k_stats": leg_stats}, {"k_stats": (8 + 12 + 24) * S}
        for W in args.windows:
            for an, align in ALIGNS.items():
                # the checks, on the buffers that are timed
                for o in (a, b):
                    for t in o.values():
                        t.fill_(-7)
                launch(W, align, a)
                launch(W, align, b)
                torch.cuda.synchronize()
                assert same(a["count"], os_["count"]) and same(a["flags"], os_["flags"]), "count / flags differ from k_stats"
                assert all(same(a[k][:nwin[W]], b[k][:nwin[W]]) for k in STATS) and same(a["count"], b["count"]), \
                    "two launches differ"
                for t in b.values():
                    t.fill_(-7)
                launch(W, align, b, want=("sum", "wcount"))
                torch.cuda.synchronize()
                assert all(same(a[k][:nwin[W]], b[k][:nwin[W]]) for k in ("sum", "wcount")), "sumcnt launch differs"
                assert all(bool((b[k] == -7).all().item()) for k in ("min", "max")), "a NULL output was written"
                assert same(a["count"], b["count"]) and same(a["flags"], b["flags"])
                legs[f"k_rollup_w{W}_{an}_all"] = lambda W=W, align=align: launch(W, align, a)
                legs[f"k_rollup_w{W}_{an}_sumcnt"] = lambda W=W, align=align: launch(W, align, a, want=("sum", "wcount"))
                # per segment: 8 B offset + 16 B window offsets in, 12 B out; per window 28 B (all) or 12 B out
                io[f"k_rollup_w{W}_{an}_all"] = (24 + 12) * S + 28 * nwin[W]
                io[f"k_rollup_w{W}_{an}_sumcnt"] = (24 + 12) * S + 12 * nwin[W]
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
               "sumcnt_launch_equals_the_full_one": True,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "effective_GBps": {k: round((8 * N + io[k]) / med[k] / 1e6, 1) for k in legs},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"}}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("windows", "median_of_medians_ms", "min_max_ms", "effective_GBps",
                                                    "over_k_stats")}), flush=True)
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

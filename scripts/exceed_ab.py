"""Same-process A/B of krr_segmented_exceed (k_exceed<R>) against krr_segmented_stats (k_stats) on the
same buffers: both read every value once through the streaming skeleton; they differ in the work
per slot and per row of 128 slots.

    python scripts/exceed_ab.py [--out profiles/exceed] [--shapes NAME ...] [--iters 10] [--reps 7]
                                [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/pods_ab.py: the bench's config-3 memory series
(100,000 compact segments of 1-14 days @1m) and its config-2 CPU series (10,000 NaN-gapped segments
of 50,400 slots).  Thresholds: every segment's own p99 (sorted_lower; few samples above, scattered:
most rows of 128 slots hold one or two) and its own p50 (dense alternation: every row takes the
scan), each as one row (R = 1) and as four equal rows (R = 4).  Before timing, every exceed
launch's count / flags must equal k_stats' bit for bit, row 0 of the R = 4 launch must equal the
R = 1 launch bit for bit in all six outputs, and two launches must give equal bits.  Each leg is
warmed up, then timed with HIP events `--iters` times per repetition, the legs alternating; `--reps`
repetitions give each leg's per-repetition medians, their median and their min-max.  Reported: ms,
effective bandwidth, the ratio of each leg to k_stats and the part of the 128-slot rows with a
sample above.  There is no threshold on the ratios.
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
FIELDS = ("above", "excess", "longest", "head", "tail", "last")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/exceed")
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
        kind, n, gaps, pod_len, fill = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        vals = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(vals, offs, 1234 if fill == 0 else 1234 ^ 0x5A5A, fill, pod_len, gaps)
        series = ctx.series(vals, offs, Lmax, gaps)

        def own_percentile(p):  # [S]: every segment's own p-th percentile (an own sample)
            v = torch.empty(S, dtype=torch.float64, device=dev)
            c = torch.empty(S, dtype=torch.int64, device=dev)
            f = torch.empty(S, dtype=torch.int32, device=dev)
            ctx.segmented_percentile(series, _native.KrrPercentileParams(_native.KRR_PCT_SORTED_LOWER, 0, p, 1, p / 100.0),
                                     v, c, f)
            torch.cuda.synchronize()
            assert int((f & _native.KRR_FLAG_CAPACITY).sum().item()) == 0
            return v

        thr = {"p99": own_percentile(99), "p50": own_percentile(50)}

        def outs(rows):
            o = {k: torch.empty(rows * S, dtype=torch.float64 if k == "excess" else torch.int64, device=dev) for k in FIELDS}
            o["count"] = torch.empty(S, dtype=torch.int64, device=dev)
            o["flags"] = torch.empty(S, dtype=torch.int32, device=dev)
            return o

        os_ = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("min", torch.float64), ("max", torch.float64), ("sum", torch.float64), ("count", torch.int64),
                ("flags", torch.int32))}

        def leg_stats():
            ctx.segmented_stats(series, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def exceed_leg(t, rows):
            d_thr = t.repeat(rows).contiguous()
            o = outs(rows)

            def run(o=o):
                ctx.segmented_exceed(series, d_thr, rows, *(o[k] for k in FIELDS), o["count"], o["flags"])
            return run, o

        legs, results = {"k_stats": leg_stats}, {}
        for tn, t in thr.items():
            for rows in (1, 4):
                legs[f"k_exceed_{tn}_r{rows}"], results[f"k_exceed_{tn}_r{rows}"] = exceed_leg(t, rows)
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        rows_hit = {}
        for tn in thr:
            one, four = results[f"k_exceed_{tn}_r1"], results[f"k_exceed_{tn}_r4"]
            for o in (one, four):
                assert same(o["count"], os_["count"]) and same(o["flags"], os_["flags"]), "count / flags differ from k_stats"
            for r in range(4):
                assert all(same(four[k][r * S:(r + 1) * S], one[k]) for k in FIELDS), "a row of R = 4 differs from R = 1"
            again = outs(1)
            legs[f"k_exceed_{tn}_r1"](again)
            torch.cuda.synchronize()
            assert all(same(again[k], one[k]) for k in one), "two launches differ"
            rows_hit[tn] = {"share_of_samples_above": round(float(one["above"].sum().item()) /
                                                            max(int(os_["count"].sum().item()), 1), 5),
                            "mean_longest_run": round(float(one["longest"].double().mean().item()), 2)}
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
        # per segment: 8 B offset in, 8 B count + 4 B flags out; k_stats 24 B of doubles, k_exceed 8 B in + 48 B out per row
        io = {k: 8 + 12 + (24 if k == "k_stats" else 56 * int(k[-1])) for k in legs}
        row = {"segments": S, "slots": N, "present_samples": present, "gapped": bool(gaps),
               "count_and_flags_equal_k_stats": True, "rows_of_r4_equal_r1": True, "two_launches_equal_bits": True,
               "thresholds": rows_hit,
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "effective_GBps": {k: round((8 * N + io[k] * S) / med[k] / 1e6, 1) for k in legs},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"}}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("thresholds", "median_of_medians_ms", "min_max_ms", "effective_GBps",
                                                    "over_k_stats")}), flush=True)
        del vals, series, os_, results, legs, thr
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

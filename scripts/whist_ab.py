"""Same-process A/B of the fleet histogram (krr_segmented_whist + one krr_whist_query of three
percentiles: k_whist, k_whist_query) against krr_segmented_stats (k_stats: ONE pass over the same
bytes) and against krr_segmented_wquantile at p90, launched once and three times (what three
percentiles cost without the histogram).

    python scripts/whist_ab.py [--out profiles/whist] [--shapes NAME ...] [--iters 10] [--reps 7] [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/wquantile_ab.py: the bench's config-3 memory
series (100,000 compact segments of 1-14 days @1m), its config-2 CPU series (10,000 NaN-gapped
segments of 50,400 slots), and the config-3 series rewritten so that EVERY sample of a series falls
into one bin (3e8 plus a jitter far below the bin width): the worst case for the LDS atomics if
lanes did not combine.  Default bins of the resource, decay_weights(1440, longest segment).
Before timing: count / flags equal k_stats' bit for bit, two launches give equal bits, the rows'
sums equal out_wsum, and the p90 answer bin is the bin of krr_segmented_wquantile's p90 value on
every segment with weight.  Legs are warmed up, then timed with HIP events `--iters` times per
repetition, alternating; `--reps` repetitions give per-repetition medians, their median and
min-max.  Reported: ms, each leg over k_stats, whist over one and over three wquantile launches,
and the byte floor (values read once + rows written, over values read; derived, not measured).
There is no threshold on the ratios.
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

# name -> (length rule, segments, gapped, pod_len, krr_synth_fill kind: 0 CPU, 1 memory, resource, one bin)
SHAPES = {
    "config3_memory_compact": ("config3", 100_000, False, 0, 1, "memory", False),
    "config2_cpu_gapped": ("config2", 10_000, True, SLOTS_7D, 0, "cpu", False),
    "config3_one_bin": ("config3", 100_000, False, 0, 1, "memory", True),
}
PERCENTILES = ((50, 1), (90, 1), (95, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/whist")
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
    from krr_amd.api import decay_weights, default_bins

    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        kind, n, gaps, pod_len, fill, resource, one_bin = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        vals = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(vals, offs, 1234 if fill == 0 else 1234 ^ 0x5A5A, fill, pod_len, gaps)
        bins = default_bins(resource)
        if one_bin:
            vals.mul_(1e-12).add_(3e8)  # memory-sized values: a jitter below 1 byte around 3e8
            assert len(set(bins.bin_of(vals[:100000].cpu().numpy()).tolist())) == 1
        series = ctx.series(vals, offs, Lmax, gaps)
        sp, width = bins.params(), bins.width
        d_tab = torch.from_numpy(decay_weights(1440, Lmax).view(np.int64)).to(dev)

        def houts():
            return {"hist": torch.empty((S, width), dtype=torch.int64, device=dev),
                    "wsum": torch.empty(S, dtype=torch.int64, device=dev),
                    "wmin": torch.empty(S, dtype=torch.float64, device=dev),
                    "wmax": torch.empty(S, dtype=torch.float64, device=dev),
                    "count": torch.empty(S, dtype=torch.int64, device=dev),
                    "flags": torch.empty(S, dtype=torch.int32, device=dev),
                    "bin": torch.empty((3, S), dtype=torch.int32, device=dev),
                    "lower": torch.empty((3, S), dtype=torch.float64, device=dev),
                    "upper": torch.empty((3, S), dtype=torch.float64, device=dev),
                    "qflags": torch.empty((3, S), dtype=torch.int32, device=dev)}

        os_ = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("min", torch.float64), ("max", torch.float64), ("sum", torch.float64), ("count", torch.int64),
                ("flags", torch.int32))}
        wq = {"value": torch.empty(S, dtype=torch.float64, device=dev), "wsum": torch.empty(S, dtype=torch.int64, device=dev),
              "passes": torch.empty(S, dtype=torch.int32, device=dev), "count": torch.empty(S, dtype=torch.int64, device=dev),
              "flags": torch.empty(S, dtype=torch.int32, device=dev)}
        h = houts()

        def leg_stats():
            ctx.segmented_stats(series, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def leg_build(o=h):
            ctx.segmented_whist(series, sp, d_tab, None, o["hist"], o["wsum"], o["wmin"], o["wmax"], o["count"], o["flags"])

        def leg_whist(o=h):
            leg_build(o)
            ctx.whist_query(o["hist"], o["wmin"], o["wmax"], sp, PERCENTILES, o["bin"], o["lower"], o["upper"], o["qflags"])

        def leg_wq():
            ctx.segmented_wquantile(series, d_tab, 90, 1, wq["value"], wq["wsum"], wq["passes"], wq["count"], wq["flags"])

        def leg_wq3():
            for _ in range(3):
                leg_wq()

        legs = {"k_stats": leg_stats, "k_whist_build_only": leg_build, "whist_build_and_query3": leg_whist,
                "k_wquantile_p90": leg_wq, "k_wquantile_p90_x3": leg_wq3}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        assert same(h["count"], os_["count"]) and same(h["flags"], os_["flags"]), "count / flags differ from k_stats"
        again = houts()
        leg_whist(again)
        torch.cuda.synchronize()
        assert all(same(again[f], h[f]) for f in h), "two launches differ"
        assert same(h["hist"].sum(dim=1), h["wsum"]), "a row's sum is not out_wsum"
        assert same(h["wsum"], wq["wsum"]), "total weight differs from krr_segmented_wquantile's"
        has = (h["wsum"] != 0).cpu().numpy()
        exact = wq["value"].cpu().numpy()[has]
        assert np.array_equal(h["bin"][1].cpu().numpy()[has], bins.bin_of(exact)), "p90 bin is not the exact answer's"
        up = h["upper"][1].cpu().numpy()[has]
        assert (exact <= up).all(), "p90 bucket end below the exact weighted p90"
        ratio = up[exact > 0] / exact[exact > 0]
        bins_used = int((h["hist"] != 0).sum(dim=1).max().item())
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
               "longest_segment": Lmax, "table_bytes": 8 * Lmax, "row_words": width,
               "bins": [bins.mantissa_bits, bins.min_exponent, bins.octaves],
               "count_and_flags_equal_k_stats": True, "two_launches_equal_bits": True,
               "p90_bin_is_the_exact_answers_bin": True, "segments_without_weight": int((~has).sum()),
               "most_bins_in_use_by_one_series": bins_used,
               "p90_upper_over_exact_max": round(float(ratio.max()), 6) if ratio.size else None,
               "byte_floor_over_one_pass": round((8 * N + 8 * S * width) / (8 * N), 4),
               "median_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
               "median_of_medians_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in meds.items()},
               "over_k_stats": {k: round(med[k] / med["k_stats"], 4) for k in legs if k != "k_stats"},
               "whist_over_wquantile_once": round(med["whist_build_and_query3"] / med["k_wquantile_p90"], 4),
               "whist_over_wquantile_x3": round(med["whist_build_and_query3"] / med["k_wquantile_p90_x3"], 4)}
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("median_of_medians_ms", "min_max_ms", "over_k_stats",
                                                    "whist_over_wquantile_once", "whist_over_wquantile_x3",
                                                    "byte_floor_over_one_pass", "most_bins_in_use_by_one_series")}),
              flush=True)
        del vals, series, os_, wq, h, again, legs
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

"""Same-process A/B of krr_pods_overlay (k_overlay) against krr_segmented_stats (k_stats) reading
the same pod values: both read every value once; k_stats writes one record per object, k_overlay
one record per object SLOT, so its floor is set by the bytes it writes.

    python scripts/overlay_ab.py [--out profiles/overlay] [--shapes NAME ...] [--iters 10] [--reps 7]
                                 [--scale 1.0]

Shapes, from krr_synth_fill (seeded) as in scripts/rollup_ab.py: the bench's config-2 CPU series
(10,000 NaN-gapped objects of 5 pods x 10,080 slots), its config-3 memory series as ONE pod per
object (100,000 compact objects of 1-14 days @1m), and a many-pod shape (1,000 compact objects of
50 pods x 1,440 slots).  Legs: k_stats over the object-level series, and k_overlay (end-aligned)
with all four per-slot outputs ("all"), with sum + active ("sumact") and with the sum alone
("sum").  Before timing, on the buffers: every overlay launch's count / flags must equal k_stats'
bit for bit, two launches must give equal bits, and the partial launches must equal the full one in
what they write and leave the rest alone.  Each leg is warmed up, then timed with HIP events
`--iters` times per repetition, the legs alternating; `--reps` repetitions give each leg's
per-repetition medians, their median and their min-max.  Reported: ms, the ratio of each leg to
k_stats, and beside it the leg's BYTE FLOOR (bytes read + bytes written) / bytes read — derived
from the shape, not measured: the ratio a kernel at k_stats' bandwidth would have.  There is no
threshold on the ratios.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import SLOTS_7D, lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)
from stats_ab import same  # noqa: E402

# name -> (objects, pods per object, pod length rule or slots, gapped, krr_synth_fill kind: 0 CPU, 1 memory)
SHAPES = {
    "config2_cpu_gapped_5pods": (10_000, 5, SLOTS_7D, True, 0),
    "config3_memory_one_pod": (100_000, 1, "config3", False, 1),
    "many_pods_50x1440": (1_000, 50, 1440, False, 0),
}
STATS = ("sum", "max", "min", "active")
VARIANTS = {"all": STATS, "sumact": ("sum", "active"), "sum": ("sum",)}
BYTES = {"sum": 8, "max": 8, "min": 8, "active": 4}
END = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/overlay")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="objects x this (rehearsals)")
    ap.add_argument("--name", default="ab")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from krr_amd import _native

    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        n, k, rule, gaps, fill = SHAPES[name]
        n = max(int(n * args.scale), 8)
        pod_lens = np.repeat(lengths(rule, n), k) if isinstance(rule, str) else np.full(n * k, rule, dtype=np.int64)
        po_np = np.concatenate([[0], np.cumsum(pod_lens)]).astype(np.int64)
        groups_np = np.arange(0, n * k + 1, k, dtype=np.int64)
        obj_np = po_np[groups_np]  # the pod segments tile this object-level series
        lg = pod_lens.reshape(n, k).max(axis=1)
        oo_np = np.concatenate([[0], np.cumsum(lg)]).astype(np.int64)
        G, N, n_slots = n, int(po_np[-1]), int(oo_np[-1])
        po, groups, obj, oo = (torch.from_numpy(a).to(dev) for a in (po_np, groups_np, obj_np, oo_np))
        vals = torch.empty(N, dtype=torch.float64, device=dev)
        # filled per OBJECT, as the bench fills it: pod_len is the grid a gapped object's pods share
        ctx.synth_fill(vals, obj, 1234 if fill == 0 else 1234 ^ 0x5A5A, fill, rule if gaps else 0, gaps)
        pods = ctx.series(vals, po, int(pod_lens.max()), gaps)
        objects = ctx.series(vals, obj, int(np.diff(obj_np).max()), gaps)
        os_ = {key: torch.empty(G, dtype=dt, device=dev) for key, dt in
               (("min", torch.float64), ("max", torch.float64), ("sum", torch.float64), ("count", torch.int64),
                ("flags", torch.int32))}

        def leg_stats():
            ctx.segmented_stats(objects, os_["min"], os_["max"], os_["sum"], os_["count"], os_["flags"])

        def outs():  # one set serves every leg: the legs run one after the other on one stream
            o = {key: torch.empty(n_slots, dtype=torch.int32 if key == "active" else torch.float64, device=dev)
                 for key in STATS}
            o["count"] = torch.empty(G, dtype=torch.int64, device=dev)
            o["flags"] = torch.empty(G, dtype=torch.int32, device=dev)
            return o

        a, b = outs(), outs()

        def launch(o, want=STATS):
            ctx.pods_overlay(pods, groups, G, END, oo, *(o[key] if key in want else None for key in STATS),
                             o["count"], o["flags"])

        leg_stats()
        # the checks, on the buffers that are timed
        for o in (a, b):
            for t in o.values():
                t.fill_(-7)
        launch(a)
        launch(b)
        torch.cuda.synchronize()
        assert same(a["count"], os_["count"]) and same(a["flags"], os_["flags"]), "count / flags differ from k_stats"
        assert all(same(a[key], b[key]) for key in STATS) and same(a["count"], b["count"]), "two launches differ"
        assert not bool((a["flags"] & _native.KRR_FLAG_CAPACITY).any().item())
        legs, written = {"k_stats": leg_stats}, {"k_stats": 0}
        for vn, want in VARIANTS.items():
            for t in b.values():
                t.fill_(-7)
            launch(b, want=want)
            torch.cuda.synchronize()
            assert all(same(a[key], b[key]) for key in want), f"{vn} launch differs"
            assert all(bool((b[key] == -7).all().item()) for key in STATS if key not in want), "a NULL output was written"
            assert same(a["count"], b["count"]) and same(a["flags"], b["flags"])
            legs[f"k_overlay_{vn}"] = lambda want=want: launch(a, want=want)
            written[f"k_overlay_{vn}"] = sum(BYTES[key] for key in want) * n_slots
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        meds = {key: [] for key in legs}
        for _ in range(args.reps):
            ev = {key: [] for key in legs}
            for _ in range(args.iters):
                for key, f in legs.items():  # alternating legs
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    ev[key].append((e0, e1))
            torch.cuda.synchronize()
            for key in legs:
                meds[key].append(float(np.median([x.elapsed_time(y) for x, y in ev[key]])))
        med = {key: float(np.median(v)) for key, v in meds.items()}
        row = {"objects": G, "pods": n * k, "values": N, "object_slots": n_slots, "gapped": bool(gaps),
               "present_samples": int(os_["count"].sum().item()),
               "count_and_flags_equal_k_stats": True, "two_launches_equal_bits": True,
               "partial_launches_equal_the_full_one": True,
               "median_ms": {key: [round(x, 4) for x in v] for key, v in meds.items()},
               "median_of_medians_ms": {key: round(v, 4) for key, v in med.items()},
               "min_max_ms": {key: [round(min(v), 4), round(max(v), 4)] for key, v in meds.items()},
               "effective_GBps": {key: round((8 * N + written[key]) / med[key] / 1e6, 1) for key in legs},
               "over_k_stats": {key: round(med[key] / med["k_stats"], 4) for key in legs if key != "k_stats"},
               "byte_floor": {key: round((8 * N + written[key]) / (8 * N), 4) for key in legs if key != "k_stats"}}
        doc["shapes"][name] = row
        print(name, json.dumps({key: row[key] for key in ("object_slots", "median_of_medians_ms", "min_max_ms",
                                                          "effective_GBps", "over_k_stats", "byte_floor")}), flush=True)
        del vals, pods, objects, os_, legs, a, b
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

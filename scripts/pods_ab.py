"""Same-process A/B of the flat fused launch and cpu_aggregation = "pods_max" on the same buffers.

    python scripts/pods_ab.py [--out profiles/pods_max] [--shapes NAME ...] [--iters 10] [--reps 3]
                              [--scale 1.0]

Legs, per shape (synthetic fleets from krr_synth_fill, seeded; LINEAR p99):
  (flat) krr_simple_run_records: one CPU segment per container
  (pods) krr_simple_run_pods: one CPU segment per pod, then the fold (krr_group_max)
  (fold) krr_group_max alone, over the pod results of leg (pods)
Both streaming legs read the same bytes; the pod leg plans its launch by the pod length instead
of the container length (krr_select_plan for both is recorded), launches the fold after it, and
synchronises the stream once before its launch (the pod_groups check), which the HIP-event
interval of that leg includes.  Before timing, the pod leg's memory half must equal the flat
leg's bit for bit, and on the one-pod shape every output and record must.  Each leg is warmed
up, then timed with HIP events `--iters` times per repetition, the legs alternating; the whole
comparison runs `--reps` times and the spread of the per-repetition medians is reported with
them.  There is no threshold: the ratio is reported, with whether it leaves the legs' spread.
"""
import argparse
import json
import os
import sys
from decimal import Decimal

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import SLOTS_7D, lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)

# name: (length rule, containers, gapped, pod_len: 0 = one pod per container)
SHAPES = {
    "config2_5pods_gapped": ("config2", 10_000, True, SLOTS_7D),
    "config3_1pod_compact": ("config3", 100_000, False, 0),
}
OUT_KEYS = (("cpu_value", "float64"), ("cpu_count", "int64"), ("cpu_flags", "int32"),
            ("mem_value", "float64"), ("mem_count", "int64"), ("mem_flags", "int32"))


def plan_row(_native, L, prm):
    p = _native.select_plan(int(L), prm)
    return {"max_segment_len": int(L), "fused_hselect": int(p.fused_hselect), "tkeep": int(p.tkeep),
            "cap_keys": int(p.cap_keys), "lds_bytes": int(p.lds_bytes), "probe": int(p.probe)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pods_max")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="containers x this (rehearsals)")
    ap.add_argument("--name", default="ab")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    prm = percentile_params(Decimal("99"), "linear")
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "mode": "linear",
           "percentile": "99", "shapes": {}}
    for name in args.shapes:
        kind, n, gaps, pod_len = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        if pod_len:  # every container is whole pods of pod_len slots
            per_object = lens // pod_len
            pod_offs_np = np.arange(int(per_object.sum()) + 1, dtype=np.int64) * pod_len
        else:
            per_object = np.ones(S, dtype=np.int64)
            pod_offs_np = offs_np
        groups_np = np.concatenate([[0], np.cumsum(per_object)]).astype(np.int64)
        assert np.array_equal(pod_offs_np[groups_np], offs_np)
        n_pods, Lpod = pod_offs_np.size - 1, int(np.diff(pod_offs_np).max())
        offs = torch.from_numpy(offs_np).to(dev)
        pod_offs = torch.from_numpy(pod_offs_np).to(dev)
        groups = torch.from_numpy(groups_np).to(dev)
        cpu = torch.empty(N, dtype=torch.float64, device=dev)
        mem = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(cpu, offs, 1234, 0, pod_len, gaps)
        ctx.synth_fill(mem, offs, 1234 ^ 0x5A5A, 1, pod_len, gaps)
        cs = ctx.series(cpu, offs, Lmax, gaps)
        pcs = ctx.series(cpu, pod_offs, Lpod, gaps)
        ms = ctx.series(mem, offs, Lmax, gaps)

        def new_out(extra=False):
            o = {k: torch.empty(S, dtype=getattr(torch, dt), device=dev) for k, dt in OUT_KEYS}
            if extra:
                o.update(pod_value=torch.empty(n_pods, dtype=torch.float64, device=dev),
                         pod_count=torch.empty(n_pods, dtype=torch.int64, device=dev),
                         pod_flags=torch.empty(n_pods, dtype=torch.int32, device=dev),
                         cpu_pod=torch.empty(S, dtype=torch.int64, device=dev))
            return o

        out_f, out_p, out_g = new_out(), new_out(True), new_out(True)
        rec_f = torch.zeros((S, 4), dtype=torch.int64, device=dev)
        rec_p = torch.zeros((S, 4), dtype=torch.int64, device=dev)
        rec_g = torch.zeros((S, 4), dtype=torch.int64, device=dev)

        def leg_flat():
            ctx.simple_run(cs, ms, prm, out_f, records=rec_f)

        def leg_pods():
            ctx.simple_run_pods(pcs, groups, ms, prm, out_p, records=rec_p)

        def leg_fold():
            ctx.group_max(groups, out_p["pod_value"], out_p["pod_count"], out_p["pod_flags"], out_g["cpu_value"],
                          out_g["cpu_count"], out_g["cpu_flags"], out_g["cpu_pod"], records=rec_g)

        legs = {"flat": leg_flat, "pods": leg_pods, "fold": leg_fold}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        row = {"containers": S, "pods": n_pods, "slots": N, "gapped": gaps,
               "plan_flat": plan_row(_native, Lmax, prm), "plan_pods": plan_row(_native, Lpod, prm),
               # both value streams, both offset arrays, the 40-B outputs and the 32-B record per
               # container; the pod leg adds the pod offsets and 20 B of pod outputs written and read
               "bytes": {"flat": 16 * N + 16 * (S + 1) + 72 * S,
                         "pods": 16 * N + 8 * (S + 1) + 8 * (n_pods + 1) + 8 * (S + 1) + 80 * S + 40 * n_pods}}
        for k in ("mem_value", "mem_count", "mem_flags"):
            assert torch.equal(out_f[k].view(torch.int64) if k == "mem_value" else out_f[k],
                               out_p[k].view(torch.int64) if k == "mem_value" else out_p[k]), (name, k)
        assert torch.equal(rec_f[:, 1], rec_p[:, 1]) and torch.equal(rec_f[:, 3], rec_p[:, 3]), name
        row["mem_half_equal"] = True
        if not pod_len:  # one pod per container: the two rules coincide
            assert torch.equal(rec_f, rec_p), name
            row["records_equal"] = True
        else:
            row["containers_where_pods_max_exceeds_flat"] = int((out_p["cpu_value"] > out_f["cpu_value"]).sum().item())
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
        row["median_ms"] = {k: [round(x, 4) for x in v] for k, v in meds.items()}
        row["spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in meds.items()}
        row["GBps"] = {k: round(row["bytes"][k] / (float(np.median(meds[k])) * 1e-3) / 1e9, 1) for k in ("flat", "pods")}
        row["pods_over_flat"] = round(float(np.median(meds["pods"]) / np.median(meds["flat"])), 4)
        gap = abs(float(np.median(meds["pods"]) - np.median(meds["flat"])))
        row["difference_leaves_spread"] = bool(gap > max(row["spread_ms"]["flat"], row["spread_ms"]["pods"]))
        row["wselect_fallbacks_total"] = ctx.wselect_fallbacks()
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in ("median_ms", "spread_ms", "pods_over_flat",
                                                    "difference_leaves_spread", "plan_flat", "plan_pods")}), flush=True)
        del cpu, mem, cs, pcs, ms, out_f, out_p, out_g
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

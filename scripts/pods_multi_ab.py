"""Same-process A/B of simple_limit under cpu_aggregation = "pods_max" on the same buffers.

    python scripts/pods_multi_ab.py [--out profiles/pods_multi] [--shapes NAME ...] [--sets NAME ...]
                                    [--iters 10] [--reps 3] [--scale 1.0]

Legs, per shape and percentile set (synthetic fleets from krr_synth_fill, seeded):
  (a) krr_simple_run_pods_multi: every percentile per pod from one launch, then one fold of P rows
  (b) one krr_simple_run_pods per percentile (what a caller had before the entry point existed)
  (c) krr_simple_run_multi: the flat rule, one CPU segment per container
Legs (a) and (b) plan by the pod length, leg (c) by the container length (krr_multi_plan for both
is recorded): a set may share one pass in (a) and fall back in (c).  Before timing, every row of
(a) must equal leg (b)'s outputs for that percentile bit for bit, and (a)'s memory half leg (c)'s.
Each leg is warmed up, then timed with HIP events `--iters` times per repetition, the legs
alternating; the whole comparison runs `--reps` times and the spread of the per-repetition
medians is reported with them.  (a) and (b) each include their stream synchronisations (the
pod_groups check: one per call, so P in leg (b)).  There is no threshold: the ratios a/b and a/c
are reported, with whether each difference leaves the legs' spread.
"""
import argparse
import json
import os
import sys
from decimal import Decimal

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from multi_pct_ab import lengths  # noqa: E402  (the bench's config-2 / config-3 length rules)
from pods_ab import SHAPES  # noqa: E402

# name: (percentiles, mode)
SETS = {
    "p95_p99_linear": (("95", "99"), "linear"),
    "p90_p99_sorted_lower": (("90", "99"), "sorted_lower"),
    "p66_p96_sorted_lower": (("66", "96"), "sorted_lower"),
}


def plan_row(_native, L, plist):
    p = _native.multi_plan(int(L), plist)
    return {"max_segment_len": int(L), "shared": int(p.shared), "tkeep": int(p.tkeep), "cap_keys": int(p.cap_keys),
            "lds_bytes": int(p.lds_bytes)}


def same(a, b):
    import torch

    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                       b.view(torch.int64) if b.dtype == torch.float64 else b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pods_multi")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--sets", nargs="*", default=list(SETS))
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
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": {}}
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
        doc["shapes"][name] = {"containers": S, "pods": n_pods, "slots": N, "gapped": gaps, "sets": {}}

        def new_out(P, pods):
            o = {}
            for k, dt, rows in (("cpu_value", torch.float64, P), ("cpu_count", torch.int64, 0),
                                ("cpu_flags", torch.int32, P), ("mem_value", torch.float64, 0),
                                ("mem_count", torch.int64, 0), ("mem_flags", torch.int32, 0)):
                o[k] = torch.empty((rows, S) if rows else (S,), dtype=dt, device=dev)
            if pods:
                o["cpu_pod"] = torch.empty((P, S) if P else (S,), dtype=torch.int64, device=dev)
                o["pod_value"] = torch.empty((P, n_pods) if P else (n_pods,), dtype=torch.float64, device=dev)
                o["pod_count"] = torch.empty(n_pods, dtype=torch.int64, device=dev)
                o["pod_flags"] = torch.empty((P, n_pods) if P else (n_pods,), dtype=torch.int32, device=dev)
            return o

        for set_name in args.sets:
            ps, mode = SETS[set_name]
            plist = [percentile_params(Decimal(p), mode) for p in ps]
            P = len(plist)
            out_a, out_c = new_out(P, True), new_out(P, False)
            out_b = [new_out(0, True) for _ in plist]

            def leg_a():
                ctx.simple_run_pods_multi(pcs, groups, ms, plist, out_a)

            def leg_b():
                for prm, o in zip(plist, out_b):
                    ctx.simple_run_pods(pcs, groups, ms, prm, o)

            def leg_c():
                ctx.simple_run_multi(cs, ms, plist, out_c)

            legs = {"a_pods_multi": leg_a, "b_pods_each": leg_b, "c_flat_multi": leg_c}
            for f in legs.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            row = {"percentiles": list(ps), "mode": mode, "plan_pods": plan_row(_native, Lpod, plist),
                   "plan_flat": plan_row(_native, Lmax, plist)}
            for j, o in enumerate(out_b):
                for k in ("cpu_value", "cpu_flags", "cpu_pod", "pod_value", "pod_flags"):
                    assert same(out_a[k][j], o[k]), (name, set_name, j, k)
                for k in ("cpu_count", "pod_count", "mem_value", "mem_count", "mem_flags"):
                    assert same(out_a[k], o[k]), (name, set_name, j, k)
            for k in ("mem_value", "mem_count", "mem_flags"):
                assert same(out_a[k], out_c[k]), (name, set_name, k)
            row["rows_equal_single_launches"] = True
            if not pod_len:  # one pod per container: the two rules coincide
                for k in ("cpu_value", "cpu_count", "cpu_flags"):
                    assert same(out_a[k], out_c[k]), (name, set_name, k)
                row["equals_flat"] = True
            else:
                row["containers_where_pods_max_exceeds_flat"] = [
                    int((out_a["cpu_value"][j] > out_c["cpu_value"][j]).sum().item()) for j in range(P)]
                row["containers_with_different_winners"] = int((out_a["cpu_pod"][0] != out_a["cpu_pod"][-1]).sum().item())
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
            med = {k: float(np.median(v)) for k, v in meds.items()}
            for other, key in (("b_pods_each", "a_over_b"), ("c_flat_multi", "a_over_c")):
                row[key] = round(med["a_pods_multi"] / med[other], 4)
                gap = abs(med["a_pods_multi"] - med[other])
                row[key + "_leaves_spread"] = bool(gap > max(row["spread_ms"]["a_pods_multi"], row["spread_ms"][other]))
            row["wselect_fallbacks_total"] = ctx.wselect_fallbacks()
            doc["shapes"][name]["sets"][set_name] = row
            print(name, set_name, json.dumps({k: row[k] for k in ("median_ms", "spread_ms", "a_over_b", "a_over_c",
                                                                  "plan_pods", "plan_flat")}), flush=True)
            del out_a, out_b, out_c
            torch.cuda.empty_cache()
        del cpu, mem, cs, pcs, ms
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()


if __name__ == "__main__":
    main()

"""Same-process A/B of cpu_aggregation = "pods_max" from raw bodies against the flat path.

    python scripts/pods_bodies_ab.py [--out profiles/pods_bodies] [--objects 2000] [--pods 3] [--runs 7]

The fleet is bench.py's host-path fleet (config-1-shaped objects: ``--pods`` per-pod query_range
bodies of 10,080 samples per object and resource, and the same samples as grouped `sum by (pod)`
bodies over 20 namespaces).  Legs, each the whole ``BatchedRunner.recommend_from_bodies`` /
``recommend_from_grouped`` call (pack -> fused launch -> exact-decimal rounding -> RunResults):
  (a) concat,   parser="device"
  (b) pods_max, parser="device"   (the pod boundaries built on the device, krr_json_pod_bounds)
  (c) pods_max, parser="host"     (the only way before the device packer kept the boundaries)
and (b), (c) again with parser="hybrid" for the record.  Before timing, (b) must equal (c) string
for string.  Every leg is warmed up; then the legs alternate, ``--runs`` times each, host clock
around the call (each call ends with its own synchronisation).  Medians, the sorted runs and the
ratios b/a and b/c are written; there is no threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pods_bodies")
    ap.add_argument("--objects", type=int, default=2000)
    ap.add_argument("--pods", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=48)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--name", default="ab")
    args = ap.parse_args()
    import torch

    from bench import BODY_HEAD, body_fleet  # the bench's generator (importing it runs nothing)
    from krr_amd.core.device_pack import default_threads
    from krr_amd.core.fleet_query import FleetQueryPlan
    from krr_amd.core.runner import BatchedRunner
    from krr_amd.strategies.simple import SimpleStrategy, SimpleStrategySettings

    objects, pods, distinct = args.objects, args.pods, args.distinct
    cpu_vals, mem_vals, cpu_b, mem_b = body_fleet(0, objects, pods, distinct)
    threads = default_threads()
    runners = {agg: BatchedRunner(SimpleStrategy(SimpleStrategySettings(
        cpu_percentile=99, memory_buffer_percentage=5, cpu_aggregation=agg))) for agg in ("concat", "pods_max")}

    class _Obj:
        def __init__(self, o):
            self.namespace, self.container = f"ns{o % 20}", "main"
            self.pods = [f"pod-{o}-{i}" for i in range(pods)]

    plan = FleetQueryPlan.for_settings([_Obj(o) for o in range(objects)], runners["concat"].strategy.settings)

    def grouped(vals, shift):
        out = []
        for gq in plan.groups:
            parts = [f'{{"metric":{{"pod":"{pod}"}},"values":[{vals[(i + shift) % distinct]}]}}'
                     for i, pod in enumerate(reversed(gq.pods))]
            out.append((BODY_HEAD + ",".join(parts) + "]}}").encode())
        return out

    g_cpu, g_mem = grouped(cpu_vals, 0), grouped(mem_vals, 7)

    def per_pod(agg, parser):
        return lambda: runners[agg].recommend_from_bodies(cpu_b, mem_b, threads=threads, parser=parser)

    def by_group(agg, parser):
        return lambda: runners[agg].recommend_from_grouped(plan, g_cpu, g_mem, threads=threads, parser=parser)

    forms = {
        "per_pod": {"a_concat_device": per_pod("concat", "device"), "b_pods_device": per_pod("pods_max", "device"),
                    "c_pods_host": per_pod("pods_max", "host"), "pods_hybrid": per_pod("pods_max", "hybrid"),
                    "concat_hybrid": per_pod("concat", "hybrid")},
        "grouped": {"a_concat_device": by_group("concat", "device"), "b_pods_device": by_group("pods_max", "device"),
                    "c_pods_host": by_group("pods_max", "host"), "pods_hybrid": by_group("pods_max", "hybrid"),
                    "concat_hybrid": by_group("concat", "hybrid")},
    }

    def strings(res):
        return [(str(r[k].request), str(r[k].limit)) for r in res for k in r]

    doc = {"device": torch.cuda.get_device_name(0), "objects": objects, "pods_per_object": pods, "runs": args.runs,
           "threads": threads, "json_bytes_per_pod_form": sum(len(b) for bs in cpu_b + mem_b for b in bs),
           "json_bytes_grouped_form": sum(len(b) for b in g_cpu + g_mem), "forms": {}}
    for form, legs in forms.items():
        first = {}
        for k, f in legs.items():  # warm-up; the hybrid share settles over a few calls
            for _ in range(4 if "hybrid" in k else 1):
                first[k] = strings(f())
        assert first["b_pods_device"] == first["c_pods_host"] == first["pods_hybrid"], form
        assert first["a_concat_device"] == first["concat_hybrid"], form
        differs = sum(a != b for a, b in zip(first["a_concat_device"], first["b_pods_device"]))
        runs = {k: [] for k in legs}
        for _ in range(args.runs):
            for k, f in legs.items():  # alternating legs
                t0 = time.perf_counter()
                f()
                runs[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        row = {"median_ms": {k: round(1e3 * v, 3) for k, v in med.items()},
               "runs_ms": {k: [round(1e3 * x, 3) for x in sorted(v)] for k, v in runs.items()},
               "objects_per_s": {k: round(objects / v, 1) for k, v in med.items()},
               "b_over_a": round(med["b_pods_device"] / med["a_concat_device"], 4),
               "b_over_c": round(med["b_pods_device"] / med["c_pods_host"], 4),
               "hybrid_pods_over_concat": round(med["pods_hybrid"] / med["concat_hybrid"], 4),
               "pods_device_equals_pods_host": True, "results_where_pods_max_differs_from_concat": differs}
        a, b = sorted(runs["a_concat_device"]), sorted(runs["b_pods_device"])
        row["b_median_inside_a_runs"] = bool(a[0] <= med["b_pods_device"] <= a[-1])
        row["a_median_inside_b_runs"] = bool(b[0] <= med["a_concat_device"] <= b[-1])
        doc["forms"][form] = row
        print(form, json.dumps({k: row[k] for k in ("median_ms", "b_over_a", "b_over_c", "hybrid_pods_over_concat",
                                                    "b_median_inside_a_runs")}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()

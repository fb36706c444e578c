"""Generate tests/golden/simple_limit.json BY IMPORTING THE REFERENCE (build container only).

    python tests/golden/make_golden_limit.py

The reference snapshot has no ``simple_limit`` strategy; what it does have is the rule for ONE
CPU percentile (SimpleStrategySettings.calculate_cpu_proposal), the memory proposal and the
rounding (Runner._format_result).  So per case, percentile pair and settings path this records
the reference's CPU proposal at EACH percentile of the pair (unsorted = ref_index, pre-sorted =
sorted_lower; numpy for linear), its memory proposal, and Runner._format_result of the RunResult
holding both CPU values (request, limit) plus the ResourceAllocations strings of that result.
Inputs are cases of simple_strategy.json / simple_strategy_exact.json (make_golden.py), by name.
Nothing from the reference is copied: only input strings and the reference's outputs.
"""
from __future__ import annotations

import json
import math
import os
import sys
from decimal import Decimal

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import dstr, import_reference  # noqa: E402

CASES = {
    "simple_strategy.json": [
        "empty_object", "one_sample", "two_samples", "three_dec_ceil_trap", "below_min_clamp", "ties",
        "zeros_signed", "zeros_signed_2", "inf_cpu", "nan_cpu_index", "nan_mem_raises", "nan_cpu_single",
        "empty_pod_dropped_order", "negative_cpu", "random_0", "random_1", "random_2", "random_3", "random_6",
    ],
    "simple_strategy_exact.json": ["probe_trailing_zeros", "probe_float_collision", "sorted_ties_repr", "zero_forms",
                                   "random_exact_0", "random_exact_3"],
}
PAIRS = [("66", "96"), ("95", "99"), ("50", "100"), ("99", "99"),
         ("33.33333333333333333333333333", "99.99999999999999999999999999")]
PATHS = {"cli": "Config(other_args={'cpu_percentile': p, 'memory_buffer_percentage': '5'}).create_strategy().settings",
         "direct": "SimpleStrategySettings(cpu_percentile=int(p)) (Decimal(p) where p is no integer)"}


def main():
    ResourceType, Config, Runner, SimpleStrategy, SimpleStrategySettings = import_reference()
    from robusta_krr.core.abstract.strategies import ResourceRecommendation
    from robusta_krr.core.models.allocations import ResourceAllocations

    cfg = Config(format="json", strategy="simple", log_to_stderr=True, other_args={})
    runner = Runner.__new__(Runner)
    runner.config = cfg

    def settings(path, p):
        if path == "cli":
            return Config(format="json", strategy="simple", log_to_stderr=True,
                          other_args={"cpu_percentile": p, "memory_buffer_percentage": "5"}).create_strategy().settings
        return SimpleStrategySettings(cpu_percentile=int(p) if p.isdigit() else Decimal(p))

    def attempt(fn):
        try:
            return fn(), None
        except Exception as e:  # noqa: BLE001 - the reference's own exception is the recorded outcome
            return None, type(e).__name__

    def rounded(values, mem):
        """Runner._format_result of {CPU: (request, limit), Memory: mem} + its ResourceAllocations."""
        for v, err in list(values) + [mem]:
            if err:
                return {"error": err}
        raw = {ResourceType.CPU: ResourceRecommendation(request=values[0][0], limit=values[1][0]),
               ResourceType.Memory: ResourceRecommendation(request=mem[0], limit=mem[0])}
        rr, err = attempt(lambda: runner._format_result(raw))
        if err:
            return {"rounded_error": err}
        alloc = ResourceAllocations(requests={rt: rr[rt].request for rt in ResourceType},
                                    limits={rt: rr[rt].limit for rt in ResourceType})
        return {"cpu_request": dstr(rr[ResourceType.CPU].request), "cpu_limit": dstr(rr[ResourceType.CPU].limit),
                "mem_request": dstr(rr[ResourceType.Memory].request), "mem_limit": dstr(rr[ResourceType.Memory].limit),
                "alloc": {"requests": {rt.value: dstr(alloc.requests[rt]) for rt in ResourceType},
                          "limits": {rt.value: dstr(alloc.limits[rt]) for rt in ResourceType}}}

    def rec(pair):
        v, err = pair
        return {"error": err} if err else dstr(v)

    out_cases = []
    for fname, names in CASES.items():
        with open(os.path.join(HERE, fname)) as fh:
            by_name = {c["name"]: c for c in json.load(fh)["cases"]}
        for name in names:
            case = by_name[name]
            cpu = {k: [Decimal(s) for s in v] for k, v in case["cpu"].items() if v}
            mem = {k: [Decimal(s) for s in v] for k, v in case["mem"].items() if v}
            flat = [x for v in cpu.values() for x in v]
            f = np.array([float(x) for x in flat], dtype=np.float64)
            results = {}
            for pr, pl in PAIRS:
                for path in PATHS:
                    sts = [settings(path, p) for p in (pr, pl)]
                    ref = [attempt(lambda st=st: st.calculate_cpu_proposal(cpu)) for st in sts]
                    srt = [attempt(lambda st=st: st.calculate_cpu_proposal({"all": sorted(flat)})) for st in sts]
                    memv = attempt(lambda: sts[0].calculate_memory_proposal(mem))
                    entry = {"ref_index": [rec(x) for x in ref], "sorted": [rec(x) for x in srt], "mem": rec(memv),
                             "rounded": {"ref_index": rounded(ref, memv), "sorted": rounded(srt, memv)}}
                    if f.size:
                        lin = [float(np.percentile(f, float(st.cpu_percentile))) for st in sts]
                        entry["linear_hex"] = ["nan" if math.isnan(x) else x.hex() for x in lin]
                    results[f"{pr}|{pl}|{path}"] = entry
            out_cases.append({"name": name, "from": fname, "cpu": case["cpu"], "mem": case["mem"],
                              "results": results})

    doc = {"generator": "tests/golden/make_golden_limit.py",
           "reference": "yonahd/krr 1.0.0 (imported through make_golden.import_reference, not copied)",
           "pairs": [list(p) for p in PAIRS], "paths": PATHS, "cases": out_cases}
    path = os.path.join(HERE, "simple_limit.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"), sort_keys=True)
    print(f"wrote {path}: {len(out_cases)} cases x {len(PAIRS)} pairs x {len(PATHS)} paths, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

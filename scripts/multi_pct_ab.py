"""Same-process A/B of several CPU percentiles per fused pass (krr_simple_run_multi).

    python scripts/multi_pct_ab.py [--out profiles/multi_pct] [--shapes NAME ...] [--legs abc]
                                   [--iters 10] [--reps 3] [--scale 1.0] [--root TREE]

Legs, per shape (synthetic fleets from krr_synth_fill, seeded):
  (a) P separate krr_simple_run launches, one per percentile   (what a caller paid before)
  (b) one krr_simple_run_multi
  (c) one krr_simple_run at the innermost percentile            (the target: one pass, one answer)
Before timing, (a) and (b) must agree bit for bit on every output.  Each leg is warmed up, then
timed with HIP events `--iters` times per repetition, the legs alternating; the whole comparison
runs `--reps` times and the spread of the per-repetition medians is reported with them.  A
shared shape passes when (b)'s slowest median beats (a)'s fastest by more than the larger spread.

`--legs a --root TREE` runs leg (a) alone against another checkout's package (it uses only
krr_simple_run, which every tree has) and writes output digests: the parent commit's leg (a)
must give the digests this tree's does (`--compare FILE`).
"""
import argparse
import hashlib
import json
import os
import sys
from decimal import Decimal

import numpy as np

SLOTS_7D = 10080


def _splitmix(x):
    z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def lengths(kind, n):
    if kind == "config3":  # 1..14 days @1m per container (bench.py's config 3 rule)
        with np.errstate(over="ignore"):
            h = _splitmix(np.arange(n, dtype=np.uint64) ^ np.uint64(0xC0F1_6303))
        return ((h % np.uint64(14)).astype(np.int64) + 1) * 1440
    if kind == "config2":  # 5 pods x 7d@1m, NaN-gapped
        return np.full(n, 5 * SLOTS_7D, dtype=np.int64)
    return np.full(n, SLOTS_7D, dtype=np.int64)  # config 4


# name: (length rule, containers, gapped, pod_len, percentiles, mode, expected to share)
SHAPES = {
    "config3_95_99_linear": ("config3", 100_000, False, 0, ("95", "99"), "linear", True),
    "config3_95_99_sorted": ("config3", 100_000, False, 0, ("95", "99"), "sorted_lower", True),
    "config4_95_99_linear": ("config4", 100_000, False, 0, ("95", "99"), "linear", True),
    "config2_97_99_linear": ("config2", 20_000, True, SLOTS_7D, ("97", "99"), "linear", True),
    "config2_66_96_refindex": ("config2", 20_000, True, SLOTS_7D, ("66", "96"), "ref_index", True),
    "config4_66_96_sorted_fallback": ("config4", 100_000, False, 0, ("66", "96"), "sorted_lower", False),
}
OUT_KEYS = (("cpu_value", "float64"), ("cpu_count", "int64"), ("cpu_flags", "int32"),
            ("mem_value", "float64"), ("mem_count", "int64"), ("mem_flags", "int32"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/multi_pct")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="containers x this (rehearsals)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--compare", default=None, help="another run's JSON: leg (a)'s digests must match")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from krr_amd import _native
    from krr_amd.core.engine import percentile_params

    multi = "b" in args.legs
    ctx = _native.Context(0)
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "root": os.path.relpath(args.root), "iters": args.iters,
           "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        kind, n, gaps, pod_len, ps, mode, want_shared = SHAPES[name]
        n = max(int(n * args.scale), 8)
        lens = lengths(kind, n)
        offs_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        S, N, Lmax = n, int(offs_np[-1]), int(lens.max())
        offs = torch.from_numpy(offs_np).to(dev)
        cpu = torch.empty(N, dtype=torch.float64, device=dev)
        mem = torch.empty(N, dtype=torch.float64, device=dev)
        ctx.synth_fill(cpu, offs, 1234, 0, pod_len, gaps)
        ctx.synth_fill(mem, offs, 1234 ^ 0x5A5A, 1, pod_len, gaps)
        cs = ctx.series(cpu, offs, Lmax, gaps)
        ms = ctx.series(mem, offs, Lmax, gaps)
        plist = [percentile_params(Decimal(p), mode) for p in ps]
        P = len(plist)

        def new_out(rows=None):
            return {k: torch.empty((rows, S) if rows and k in ("cpu_value", "cpu_flags") else S,
                                   dtype=getattr(torch, dt), device=dev) for k, dt in OUT_KEYS}

        out_a = [new_out() for _ in plist]
        out_c = new_out()
        row = {"containers": S, "slots": N, "max_len": Lmax, "gapped": gaps, "percentiles": list(ps), "mode": mode}
        inner = 0
        if multi:
            out_b = new_out(P)
            plan = _native.multi_plan(Lmax, plist)
            row["shared"] = int(plan.shared)
            row["plan"] = {"tkeep": int(plan.tkeep), "cap_keys": int(plan.cap_keys), "bottom": int(plan.bottom),
                           "lds_bytes": int(plan.lds_bytes)}
            assert bool(plan.shared) == want_shared, (name, plan.shared)
            inner = int(np.argmax([float(p) for p in ps])) if plan.bottom else int(np.argmin([float(p) for p in ps]))
        # algorithmic bytes: the fused launch's (both value streams, both offset arrays, 40 B of
        # outputs per container) plus 20 (P - 1) S bytes of further CPU outputs
        fused = 16 * N + 16 * (S + 1) + 40 * S
        row["bytes"] = {"a": P * fused, "b": fused + 20 * (P - 1) * S, "c": fused}

        def leg_a():
            for prm, o in zip(plist, out_a):
                ctx.simple_run(cs, ms, prm, o)

        def leg_b():
            ctx.simple_run_multi(cs, ms, plist, out_b)

        def leg_c():
            ctx.simple_run(cs, ms, plist[inner], out_c)

        legs = {k: f for k, f in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if k in args.legs}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        if "a" in legs:
            h = hashlib.sha256()
            for o in out_a:
                for k, _ in OUT_KEYS:
                    h.update(o[k].cpu().numpy().tobytes())
            row["digest_a"] = h.hexdigest()
        if multi and "a" in legs:  # (a) and (b): bit-equal, every output
            for j, o in enumerate(out_a):
                for k in ("cpu_value", "cpu_flags"):
                    assert torch.equal(o[k].view(torch.int64) if k == "cpu_value" else o[k],
                                       out_b[k][j].view(torch.int64) if k == "cpu_value" else out_b[k][j]), (name, j, k)
                for k in ("cpu_count", "mem_count", "mem_flags"):
                    assert torch.equal(o[k], out_b[k]), (name, j, k)
                assert torch.equal(o["mem_value"].view(torch.int64), out_b["mem_value"].view(torch.int64)), (name, j)
            row["a_equals_b"] = True
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
        row["GBps"] = {k: round(row["bytes"][k] / (float(np.median(v)) * 1e-3) / 1e9, 1) for k, v in meds.items()}
        if "a" in meds and "b" in meds:
            spread = max(row["spread_ms"]["a"], row["spread_ms"]["b"])
            gain = min(meds["a"]) - max(meds["b"])
            row["b_over_a"] = round(float(np.median(meds["b"]) / np.median(meds["a"])), 4)
            row["b_beats_a_by_more_than_spread"] = bool(gain > spread)
        if "c" in meds and "b" in meds:
            row["b_over_c"] = round(float(np.median(meds["b"]) / np.median(meds["c"])), 4)
        doc["shapes"][name] = row
        print(name, json.dumps({k: row[k] for k in row if k in ("shared", "median_ms", "spread_ms", "b_over_a",
                                                                 "b_over_c", "b_beats_a_by_more_than_spread")}),
              flush=True)
        del cpu, mem, out_a, out_c, cs, ms
        if multi:
            del out_b
        torch.cuda.empty_cache()
    if args.compare:
        other = json.load(open(args.compare))["shapes"]
        doc["leg_a_matches"] = {k: other[k]["digest_a"] == v["digest_a"] for k, v in doc["shapes"].items()
                                if k in other}
        doc["compared_with"] = args.compare
        print("leg (a) digests against", args.compare, doc["leg_a_matches"], flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.name + ".json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", path)
    ctx.close()
    failed = [k for k, v in doc["shapes"].items()
              if v.get("shared") and v.get("b_beats_a_by_more_than_spread") is False]
    if failed or (args.compare and not all(doc["leg_a_matches"].values())):
        print("FAILED:", failed, doc.get("leg_a_matches"))
        sys.exit(1)


if __name__ == "__main__":
    main()

"""Device engine: moves a PackedFleet to HBM, runs the SimpleStrategy kernels
through the C ABI, and returns the raw per-object results.

There is no CPU path: ``SimpleEngine`` raises NativeUnavailable when the HIP
library or a device is missing.  One krr_ctx per (thread, device) keeps the
ABI's "one ctx per thread" rule while the reference's runner calls strategies
from a thread pool (runner.py:104-106).
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import Optional

import numpy as np

from krr_amd import _native
from krr_amd.core.packing import PackedFleet, PackedSeries

MODE_CODES = {"ref_index": _native.KRR_PCT_REF_INDEX, "sorted_lower": _native.KRR_PCT_SORTED_LOWER,
              "linear": _native.KRR_PCT_LINEAR}


def percentile_params(percentile, mode: str) -> _native.KrrPercentileParams:
    """The kernels' percentile parameters for any ``cpu_percentile`` the reference accepts.

    The index rule k(n) (REF_INDEX, SORTED_LOWER) is the reference's int((n-1) * p / 100)
    (simple.py:36) evaluated as it evaluates it (krr_amd.core.index_rule): the kernels'
    128-bit exact floor of p_num / p_den where that provably agrees, else a table of k(n)
    that ``_native`` binds at launch time (``params.rule``, sized by the launch's longest
    segment).  q = float(p) / 100 is numpy's LINEAR rule.
    """
    from krr_amd.core.index_rule import IndexRule

    if mode not in MODE_CODES:
        raise ValueError(f"unknown percentile mode {mode!r}; expected one of {sorted(MODE_CODES)}")
    rule = IndexRule.of(percentile)
    p_num, p_den = rule.approx()
    q = float(percentile) / 100.0
    params = _native.KrrPercentileParams(MODE_CODES[mode], 0, p_num, p_den, q)
    params.rule = rule
    return params


WEIGHT_MAX = 1 << 32  # the largest age weight: a segment's total stays below 2^63
P_DEN_MAX = 10**15    # krr_percentile_params' bound on p_den


def percentile_fraction(percentile) -> tuple:
    """``percentile`` (anything ``Decimal(str(.))`` takes, 0 < p <= 100) as the exact fraction
    (p_num, p_den) in lowest terms that krr_segmented_wquantile compares with.  ValueError
    outside (0, 100] or when the denominator exceeds 10^15."""
    from decimal import Decimal, InvalidOperation
    from fractions import Fraction

    try:
        d = Decimal(str(percentile))
    except InvalidOperation:
        raise ValueError(f"percentile {percentile!r} is not a number") from None
    if not d.is_finite() or not 0 < d <= 100:
        raise ValueError(f"percentile must lie in (0, 100], got {percentile!r}")
    f = Fraction(d)
    if f.denominator > P_DEN_MAX:
        raise ValueError(f"percentile {percentile!r} needs a denominator above 10^15")
    return f.numerator, f.denominator


def weight_table(weights) -> np.ndarray:
    """``weights`` as the contiguous uint64 table krr_segmented_wquantile reads.  ValueError when
    it is not a 1-D array of an unsigned (or non-negative signed) integer dtype, is empty, or
    has an entry above 2^32."""
    w = np.asarray(weights)
    if w.ndim != 1 or w.size == 0:
        raise ValueError(f"weights must be a non-empty 1-D array, got shape {w.shape}")
    if w.dtype == bool or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f"weights must have an integer dtype (uint64), got {w.dtype}")
    if np.issubdtype(w.dtype, np.signedinteger) and (w < 0).any():
        raise ValueError("weights must not be negative")
    if (w > WEIGHT_MAX).any():
        raise ValueError("weights must not exceed 2^32")
    return np.ascontiguousarray(w, dtype=np.uint64)


@dataclass
class RawResults:
    """Per-object raw proposals as the kernels return them (host numpy arrays)."""
    cpu_value: np.ndarray
    cpu_count: np.ndarray
    cpu_flags: np.ndarray
    mem_value: np.ndarray
    mem_count: np.ndarray
    mem_flags: np.ndarray
    # HistoryData segments whose Decimals the float64 values do not reproduce
    # (PackedSeries.exact): krr_locate's answers ({"cpu"|"mem": (lt, eq, pos)}, int64 [S]
    # each, -1 where not located), then krr_amd.core.exact.resolve's object index -> the
    # reference's own sample object (CPU proposal / memory max before the buffer)
    locate: Optional[dict] = None
    cpu_exact: Optional[dict] = None
    mem_exact: Optional[dict] = None
    # cpu_aggregation = "pods_max", on request: each pod segment's own result (pod_value,
    # pod_count, pod_flags [n_pods]), the winning pod's index within its object (cpu_pod [S],
    # -1: none) and, for HistoryData, krr_locate's answers over the pod segments ("locate")
    pods: Optional[dict] = None


def _empty_results() -> RawResults:
    """The results of a fleet without objects."""
    e = np.zeros(0)
    return RawResults(e, e.astype(np.int64), e.astype(np.uint32), e, e.astype(np.int64), e.astype(np.uint32))


class SimpleEngine:
    def __init__(self, device: int = 0):
        self.device = int(device)
        self._tls = threading.local()

    def context(self) -> _native.Context:
        ctx = getattr(self._tls, "ctx", None)
        if ctx is None:
            ctx = _native.Context(self.device)
            self._tls.ctx = ctx
        return ctx

    def _to_device(self, ps: PackedSeries):
        import torch

        dev = torch.device("cuda", self.device)
        if isinstance(ps.values, torch.Tensor) and ps.values.is_cuda:  # already in HBM (device packer)
            if ps.values.device != dev or ps.offsets.device != dev:
                # packed on another GPU: the kernels read only this ctx's HBM
                raise ValueError(f"series packed on {ps.values.device}, engine runs on {dev}: pack on the "
                                 f"engine's device (or copy the fleet there first)")
            return ps.values, ps.offsets
        host = torch.from_numpy(np.ascontiguousarray(ps.values, dtype=np.float64))
        # page-locked values (pinned_alloc) go by DMA without blocking the host; the
        # caller synchronises before the host buffer is released
        vals = host.to(dev, non_blocking=host.is_pinned())
        offs = torch.from_numpy(np.ascontiguousarray(ps.offsets, dtype=np.int64)).to(dev, non_blocking=False)
        return vals, offs

    def run_device(self, cpu_vals, cpu_offs, mem_vals, mem_offs, params: _native.KrrPercentileParams,
                   cpu_max_len: int = 0, mem_max_len: int = 0, gaps_are_nan: bool = False,
                   out: Optional[dict] = None, stream=None) -> dict:
        """All inputs already in HBM (torch tensors).  Returns the device output dict."""
        import torch

        ctx = self.context()
        S = cpu_offs.numel() - 1
        dev = cpu_vals.device
        if out is None:
            out = {
                "cpu_value": torch.empty(S, dtype=torch.float64, device=dev),
                "cpu_count": torch.empty(S, dtype=torch.int64, device=dev),
                "cpu_flags": torch.empty(S, dtype=torch.int32, device=dev),
                "mem_value": torch.empty(S, dtype=torch.float64, device=dev),
                "mem_count": torch.empty(S, dtype=torch.int64, device=dev),
                "mem_flags": torch.empty(S, dtype=torch.int32, device=dev),
            }
        cs = ctx.series(cpu_vals, cpu_offs, cpu_max_len, gaps_are_nan)
        ms = ctx.series(mem_vals, mem_offs, mem_max_len, gaps_are_nan)
        ctx.simple_run(cs, ms, params, out, stream=stream)
        return out

    def run_packed(self, fleet: PackedFleet, params: _native.KrrPercentileParams, aggregation: str = "concat",
                   return_pods: bool = False) -> RawResults:
        """``aggregation``: "concat" (one percentile over an object's concatenated pods) or
        "pods_max" (the max over its pods of each pod's percentile, krr_simple_run_pods; the
        CPU series needs pod boundaries).  ``return_pods`` (pods_max): also the pod-level
        results (RawResults.pods)."""
        import torch

        if fleet.cpu.n_segments != fleet.mem.n_segments:
            raise ValueError("cpu and memory need one segment per object each")
        self.context()  # raises NativeUnavailable without the HIP library or a device
        if fleet.n_objects == 0:
            return _empty_results()
        from krr_amd.core.distributed import unpack_records

        S = fleet.n_objects
        locate = needs_locate(fleet, params)
        with torch.cuda.device(self.device):
            # the launch writes the 32-B records straight into page-locked host memory
            # (krr_simple_run_records with a mapped host buffer): one sync, no D2H copies
            rec = torch.empty((S, 4), dtype=torch.int64, pin_memory=True)
            pods = {} if return_pods and aggregation == "pods_max" else None
            loc = self._run_chunks(fleet, params, rec, locate=locate, aggregation=aggregation, pods=pods)
            torch.cuda.current_stream(self.device).synchronize()
        host = unpack_records(rec.numpy())
        if pods is not None:
            pod_loc = pods.pop("locate", None)
            pods = {k: torch.cat(v).cpu().numpy() for k, v in pods.items()}  # S > 0: at least one chunk
            pods["pod_flags"] = pods["pod_flags"].view(np.uint32)
            pods["locate"] = pod_loc
        return RawResults(host["cpu_value"], host["cpu_count"], host["cpu_flags"], host["mem_value"],
                          host["mem_count"], host["mem_flags"], loc, pods=pods)

    def run_packed_records(self, fleet: PackedFleet, params: _native.KrrPercentileParams,
                           aggregation: str = "concat"):
        """The fused kernel pass over a (shard of a) fleet, returning its 32-B result
        records as an int64 [S, 4] device tensor (krr_simple_run_records, or
        krr_simple_run_pods for ``aggregation`` "pods_max": written by the same launches) on
        the current stream — what a rank sends to rank 0."""
        import torch

        if fleet.cpu.n_segments != fleet.mem.n_segments:
            raise ValueError("cpu and memory need one segment per object each")
        self.context()
        S = fleet.n_objects
        dev = torch.device("cuda", self.device)
        rec = torch.empty((S, 4), dtype=torch.int64, device=dev)
        if S == 0:
            return rec
        with torch.cuda.device(self.device):
            self._run_chunks(fleet, params, rec, aggregation=aggregation)
            # the host buffers may be pinned and released by the caller: finish the copies
            torch.cuda.current_stream(self.device).synchronize()
        return rec

    # a fleet of more than 2 chunks of values runs as chunks of about this many bytes
    # (both resources), each uploaded into buffers of its own and launched on its own:
    # HBM holds one chunk at a time, and big single launches stream slower
    # (profiles/r02/footprint)
    chunk_bytes = 16 << 30

    def _run_chunks(self, fleet: PackedFleet, params: _native.KrrPercentileParams, rec,
                    locate: bool = False, aggregation: str = "concat", pods: Optional[dict] = None) -> Optional[dict]:
        """Upload + fused launch per chunk of objects, records rows into ``rec`` (device or
        page-locked host), all on the current stream: a chunk's device buffers are released
        to the caching allocator after its launch is enqueued, which reuses them in stream
        order for the next chunk.  ``locate``: also krr_locate over each chunk's segments of
        exactness class >= 1 (``_locate_chunk``); returns its answers, else None.
        ``aggregation`` "pods_max": krr_simple_run_pods per chunk over its pod segments;
        ``pods`` (a dict) then collects the chunks' pod-level device tensors and, with
        ``locate``, krr_locate's answers over the pod segments (the CPU side of the exact path
        is resolved per pod, krr_amd.core.exact.resolve_pods)."""
        import torch

        if aggregation not in ("concat", "pods_max"):
            raise ValueError(f"unknown cpu aggregation {aggregation!r}; expected 'concat' or 'pods_max'")
        if aggregation == "pods_max":
            return self._run_chunks_pods(fleet, params, rec, locate, pods)
        S = fleet.n_objects
        ctx = self.context()
        dev = torch.device("cuda", self.device)
        out = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("cpu_value", torch.float64), ("cpu_count", torch.int64), ("cpu_flags", torch.int32),
                ("mem_value", torch.float64), ("mem_count", torch.int64), ("mem_flags", torch.int32))}
        loc = {r: tuple(np.full(S, -1, dtype=np.int64) for _ in range(3)) for r in ("cpu", "mem")} if locate else None
        for lo, hi, part, cs, ms in self._chunks(fleet):
            chunk_out = {k: v[lo:hi] for k, v in out.items()}
            ctx.simple_run(cs, ms, params, chunk_out, records=rec[lo:hi])
            if locate:
                self._locate_chunk(ctx, part, cs, ms, params, chunk_out, loc, lo)
        return loc

    def _run_chunks_pods(self, fleet: PackedFleet, params, rec, locate: bool, pods: Optional[dict]) -> Optional[dict]:
        import torch

        from krr_amd.core.packing import PackedSeries, pod_view

        if fleet.cpu.pod_offsets is None or fleet.cpu.pod_groups is None:
            pod_view(fleet.cpu)  # raises the ValueError that names the packer
        S, n_pods = fleet.n_objects, fleet.cpu.n_pods
        ctx = self.context()
        dev = torch.device("cuda", self.device)
        out = {k: torch.empty(S, dtype=dt, device=dev) for k, dt in
               (("cpu_value", torch.float64), ("cpu_count", torch.int64), ("cpu_flags", torch.int32),
                ("cpu_pod", torch.int64), ("mem_value", torch.float64), ("mem_count", torch.int64),
                ("mem_flags", torch.int32))}
        loc = {r: tuple(np.full(S, -1, dtype=np.int64) for _ in range(3)) for r in ("cpu", "mem")} if locate else None
        pod_loc = None
        if locate and fleet.cpu.exact is not None and params.mode == _native.KRR_PCT_SORTED_LOWER:
            pod_loc = {"cpu": tuple(np.full(n_pods, -1, dtype=np.int64) for _ in range(3))}
        if pods is not None:
            pods.update({"pod_value": [], "pod_count": [], "pod_flags": [], "cpu_pod": [], "locate": pod_loc})
        pod_lo = 0
        for lo, hi, part, cs, ms in self._chunks(fleet):
            view, pg, pcs = self._pod_series(ctx, part, cs)
            n = view.n_segments
            chunk_out = {k: v[lo:hi] for k, v in out.items()}
            chunk_out.update(pod_value=torch.empty(n, dtype=torch.float64, device=dev),
                             pod_count=torch.empty(n, dtype=torch.int64, device=dev),
                             pod_flags=torch.empty(n, dtype=torch.int32, device=dev))
            ctx.simple_run_pods(pcs, pg, ms, params, chunk_out, records=rec[lo:hi])
            if pods is not None:
                for k in ("pod_value", "pod_count", "pod_flags", "cpu_pod"):
                    pods[k].append(chunk_out[k])
            if locate:
                self._locate_chunk(ctx, part, cs, ms, params, chunk_out, loc, lo, names=("mem",))
                if pod_loc is not None and view.exact is not None:
                    pod_out = {"cpu_value": chunk_out["pod_value"], "cpu_count": chunk_out["pod_count"],
                               "cpu_flags": chunk_out["pod_flags"]}
                    self._locate_chunk(ctx, PackedFleet(view, PackedSeries(part.mem.values, part.mem.offsets, 0)),
                                       pcs, ms, params, pod_out, pod_loc, pod_lo, names=("cpu",))
            pod_lo += n
        return loc

    def _pod_series(self, ctx, part: PackedFleet, cs):
        """A chunk's CPU values as one segment per pod: (the pod view, pod_groups in HBM, the
        krr_series over the pod segments).  Host-packed series go through ``pod_view`` and an
        upload of the two arrays; a fleet resident in HBM (device packer: one chunk, canonical)
        hands its pod offsets and groups tensors to the kernels as they are."""
        import torch

        from krr_amd.core.packing import PackedSeries, pod_view

        dev = torch.device("cuda", self.device)
        cpu = part.cpu
        po, pg = cpu.pod_offsets, cpu.pod_groups
        if all(isinstance(t, torch.Tensor) and t.is_cuda for t in (cpu.values, po, pg)):
            if po.device != dev or pg.device != dev:
                raise ValueError(f"pod boundaries on {po.device}, engine runs on {dev}: pack on the engine's device")
            po, pg = po.contiguous(), pg.contiguous()
            longest = cpu.pod_max_len
            if longest is None:  # a resident series put together without it: one synchronising read
                longest = int((po[1:] - po[:-1]).max()) if po.numel() > 1 else 0
            view = PackedSeries(cpu.values, po, int(longest), cpu.gaps_are_nan)
        else:
            view = pod_view(cpu)
            po = torch.from_numpy(np.ascontiguousarray(view.offsets)).to(dev)
            pg = torch.from_numpy(np.ascontiguousarray(cpu.pod_groups, dtype=np.int64)).to(dev)
        return view, pg, ctx.series(cs._keep[0], po, max(view.max_len, 1), view.gaps_are_nan)

    def _chunks(self, fleet: PackedFleet):
        """Per chunk of ``_chunk_bounds``: (lo, hi, the chunk's fleet, its CPU series, its memory
        series), uploaded on the current stream when the generator reaches it."""
        from krr_amd.core.distributed import slice_fleet

        ctx = self.context()
        for lo, hi in self._chunk_bounds(fleet):
            part = fleet if (lo, hi) == (0, fleet.n_objects) else slice_fleet(fleet, lo, hi)
            cv, co = self._to_device(part.cpu)
            mv, mo = self._to_device(part.mem)
            yield (lo, hi, part, ctx.series(cv, co, max(part.cpu.max_len, 1), part.cpu.gaps_are_nan),
                   ctx.series(mv, mo, max(part.mem.max_len, 1), part.mem.gaps_are_nan))

    def _chunk_bounds(self, fleet: PackedFleet) -> list:
        """The object ranges a fleet runs as: whole when it is resident in HBM or within two
        chunks of values, else sample-balanced chunks of about ``chunk_bytes``."""
        import torch

        from krr_amd.core.distributed import fleet_shard_bounds

        S = fleet.n_objects
        nbytes = 8 * (int(fleet.cpu.offsets[-1]) + int(fleet.mem.offsets[-1]))
        resident = isinstance(fleet.cpu.values, torch.Tensor) and fleet.cpu.values.is_cuda
        n = 1 if resident or nbytes <= 2 * self.chunk_bytes else -(-nbytes // self.chunk_bytes)
        return [(0, S)] if n == 1 else [(lo, hi) for lo, hi in fleet_shard_bounds(fleet, n) if hi > lo]

    # --- one series at a time: the statistics behind krr_amd.api.batch.FleetBatch -----------
    def stats_series(self, ps: PackedSeries) -> dict:
        """Count, min, max and sum of every segment of one series (krr_segmented_stats): host
        arrays ``min``, ``max``, ``sum`` (float64), ``count`` (int64) and ``flags`` (uint32),
        [S] each.  A host series is uploaded and run in chunks of whole segments of about
        ``chunk_bytes``; one already in HBM (device packer) runs as it is.  Every launch goes on
        the current stream, with one synchronisation at the end."""
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        parts = [self._stats_part(ctx, part) for part in self._series_parts(ps)]
        return self._host_concat(parts, {"min": np.float64, "max": np.float64, "sum": np.float64,
                                         "count": np.int64, "flags": np.int32})

    def moments_series(self, ps: PackedSeries, trend: bool = True) -> dict:
        """Mean and centred second moments of every segment of one series
        (krr_segmented_moments): host arrays ``mean``, ``m2`` and, with ``trend``, ``tmean``,
        ``t2``, ``cxt`` (float64), ``count`` (int64) and ``flags`` (uint32), [S] each.  Chunks
        and synchronisation as ``stats_series``: segments never span chunks, so the chunks'
        results are concatenated and nothing is merged across them."""
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        parts = [self._moments_part(ctx, part, trend) for part in self._series_parts(ps)]
        dtypes = {k: np.float64 for k in (("mean", "m2", "tmean", "t2", "cxt") if trend else ("mean", "m2"))}
        return self._host_concat(parts, {**dtypes, "count": np.int64, "flags": np.int32})

    def exceed_series(self, ps: PackedSeries, thresholds) -> dict:
        """Per segment and threshold, the samples above it (krr_segmented_exceed): host arrays
        ``above``, ``longest``, ``head``, ``tail``, ``last`` (int64) and ``excess`` (float64),
        [R, S] each, row r for ``thresholds[r]``; ``count`` (int64) and ``flags`` (uint32), [S].
        ``thresholds`` is float64 [R, S] with any R >= 1: rows run in groups of
        KRR_MAX_THRESHOLDS, each group one pass over the series (a host chunk is uploaded once
        and serves all its groups).  Chunks and synchronisation as ``stats_series``; a chunk
        takes the thresholds of its own segment range."""
        import torch

        thr = np.ascontiguousarray(thresholds, dtype=np.float64)
        if thr.ndim != 2 or thr.shape[0] < 1 or thr.shape[1] != ps.n_segments:
            raise ValueError(f"thresholds must be float64 [R, {ps.n_segments}] with R >= 1, got shape {thr.shape}")
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        R, G = thr.shape[0], _native.KRR_MAX_THRESHOLDS
        ints = ("above", "longest", "head", "tail", "last")
        parts, lo = [], 0
        for part in self._series_parts(ps):
            hi = lo + part.n_segments
            if R > G:
                part = self._resident(part)
            groups = [self._exceed_part(ctx, part, thr[a:a + G, lo:hi]) for a in range(0, R, G)]
            out = groups[0]
            if len(groups) > 1:  # rows of the groups one under the other; count and flags are the same in each
                out = {**out, **{k: torch.cat([g[k] for g in groups], dim=0) for k in ints + ("excess",)}}
            parts.append(out)
            lo = hi
        return self._host_concat(parts, {**{k: np.int64 for k in ints}, "excess": np.float64,
                                         "count": np.int64, "flags": np.int32},
                                 rows={**{k: R for k in ints}, "excess": R})

    def wquantile_series(self, ps: PackedSeries, weights, percentile) -> dict:
        """Per segment the exact weighted percentile under age-indexed integer weights
        (krr_segmented_wquantile): host arrays ``value`` (float64), ``wsum`` (uint64: the total
        weight of the present samples), ``passes`` (int32: times the segment was streamed),
        ``count`` (int64) and ``flags`` (uint32), [S] each.  ``weights`` is a 1-D unsigned
        integer table with entries within 0..2^32 (``weight_table`` says what else is refused),
        ``percentile`` anything ``percentile_fraction`` takes.  The table is uploaded once per
        call and serves every chunk; chunks and synchronisation as ``stats_series``."""
        tab = weight_table(weights)
        p_num, p_den = percentile_fraction(percentile)
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        parts, d_tab = [], None
        for part in self._series_parts(ps):
            if d_tab is None:
                d_tab = self._upload_table(tab)
            parts.append(self._wquantile_part(ctx, part, d_tab, p_num, p_den))
        host = self._host_concat(parts, {"value": np.float64, "wsum": np.int64, "passes": np.int32,
                                         "count": np.int64, "flags": np.int32})
        host["wsum"] = host["wsum"].view(np.uint64)
        return host

    def whist_series(self, ps: PackedSeries, weights, bins: _native.KrrSketchParams, age_base=None) -> dict:
        """Per segment a histogram of age-indexed integer weights over the log-linear bins
        ``bins``, from one pass (krr_segmented_whist): ``hist``, an int64 tensor [S, width] LEFT
        IN HBM (uint64 words below 2^63: rows add exactly with a tensor add), and the host arrays
        ``wsum`` (uint64), ``wmin`` / ``wmax`` (float64: the least and greatest sample of
        positive weight, NaN without one), ``count`` (int64) and ``flags`` (uint32), [S] each.
        ``weights`` as ``wquantile_series`` takes it; ``age_base`` None or int64 [S], not
        negative: the slots that FOLLOW each segment in the series it is a slice of.  The table
        is uploaded once; chunks and synchronisation as ``stats_series``, a chunk taking the
        ``age_base`` of its own segment range."""
        import torch

        tab = weight_table(weights)
        base = None
        if age_base is not None:
            base = np.ascontiguousarray(age_base, dtype=np.int64)
            if base.shape != (ps.n_segments,) or (base < 0).any():
                raise ValueError(f"age_base must be int64 [{ps.n_segments}] and not negative")
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        width = ctx.sketch_width(bins)
        parts, d_tab, lo = [], None, 0
        for part in self._series_parts(ps):
            if d_tab is None:
                d_tab = self._upload_table(tab)
            hi = lo + part.n_segments
            parts.append(self._whist_part(ctx, part, d_tab, bins, width, None if base is None else base[lo:hi]))
            lo = hi
        host = self._host_concat([{k: v for k, v in p.items() if k != "hist"} for p in parts],
                                 {"wsum": np.int64, "wmin": np.float64, "wmax": np.float64, "count": np.int64,
                                  "flags": np.int32})
        host["wsum"] = host["wsum"].view(np.uint64)
        if len(parts) == 1:
            host["hist"] = parts[0]["hist"]
        elif parts:
            host["hist"] = torch.cat([p["hist"] for p in parts], dim=0)
        else:
            host["hist"] = torch.empty((0, width), dtype=torch.int64, device=torch.device("cuda", self.device))
        return host

    def whist_query(self, rows, wmin, wmax, bins: _native.KrrSketchParams, percentiles) -> dict:
        """Percentiles read from histogram rows (krr_whist_query): host arrays ``bin`` (int32: the
        answer bin, -1 for a row without weight), ``lower`` / ``upper`` (float64: the bin's range
        clamped to [wmin, wmax]) and ``flags`` (uint32), [P, R] each, row j for
        ``percentiles[j]`` (anything ``percentile_fraction`` takes).  ``rows`` is an int64 tensor
        [R, width] in HBM, ``wmin`` / ``wmax`` float64 [R], host arrays or tensors.  Lists longer
        than KRR_MAX_PERCENTILES run in groups; one synchronisation at the end."""
        import torch

        fracs = [percentile_fraction(p) for p in percentiles]
        if not fracs:
            raise ValueError("at least one percentile")
        ctx = self.context()
        dev = torch.device("cuda", self.device)
        R, P, G = int(rows.shape[0]), len(fracs), _native.KRR_MAX_PERCENTILES
        with torch.cuda.device(self.device):
            mn, mx = (t.to(dev) if isinstance(t, torch.Tensor)
                      else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev) for t in (wmin, wmax))
            out = self._outputs((("bin", torch.int32, P), ("lower", torch.float64, P), ("upper", torch.float64, P),
                                 ("flags", torch.int32, P)), R)
            for a in range(0, P, G):
                ctx.whist_query(rows, mn, mx, bins, fracs[a:a + G], out["bin"][a:a + G], out["lower"][a:a + G],
                                out["upper"][a:a + G], out["flags"][a:a + G])
        return self._host_concat([out], {"bin": np.int32, "lower": np.float64, "upper": np.float64,
                                         "flags": np.int32})

    def rollup_series(self, ps: PackedSeries, window: int, align: int) -> dict:
        """Every segment of one series cut into windows of ``window`` slots
        (krr_segmented_rollup; ``align`` KRR_ROLLUP_START or KRR_ROLLUP_END): ``wcount`` (int32),
        ``min``, ``max``, ``sum`` (float64) as flat DEVICE tensors with one entry per window — at
        a small window they are a large part of the series, so they stay in HBM — ``offsets``
        (host int64 [S + 1]: segment s owns windows offsets[s] .. offsets[s+1]), ``count`` (int64)
        and ``flags`` (uint32) as host arrays [S].  Chunks as ``stats_series``: the chunks'
        windows are concatenated on the device and their offsets rebased.  The window offsets of
        a host series come from its host offsets; for a series resident in HBM they are computed
        there and read back, the one synchronisation before the outputs are sized."""
        import torch

        window = int(window)
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        dev = torch.device("cuda", self.device)
        parts, woffs, base = [], [np.zeros(1, dtype=np.int64)], 0
        for part in self._series_parts(ps):
            out, wo = self._rollup_part(ctx, part, window, align)
            parts.append(out)
            woffs.append(wo[1:] + base)
            base += int(wo[-1])
        names = (("wcount", torch.int32), ("min", torch.float64), ("max", torch.float64), ("sum", torch.float64))
        if not parts:
            res = {k: torch.empty(0, dtype=dt, device=dev) for k, dt in names}
        elif len(parts) == 1:
            res = {k: parts[0][k] for k, _ in names}
        else:
            res = {k: torch.cat([p[k] for p in parts]) for k, _ in names}
        host = self._host_concat([{k: p[k] for k in ("count", "flags")} for p in parts],
                                 {"count": np.int64, "flags": np.int32})
        res.update(offsets=np.concatenate(woffs), count=host["count"], flags=host["flags"])
        return res

    def _rollup_part(self, ctx, part: PackedSeries, window: int, align: int) -> tuple:
        """Upload (host series) and one krr_segmented_rollup launch on the current stream: the
        chunk's device tensors and its window offsets as a host array."""
        import torch

        dev = torch.device("cuda", self.device)
        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            n = part.n_segments
            if isinstance(part.offsets, np.ndarray):
                wo = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(-(-np.diff(part.offsets.astype(np.int64, copy=False)) // window), out=wo[1:])
                d_wo = torch.from_numpy(wo).to(dev)
            else:
                offs = series._keep[1]
                d_wo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum(torch.div(offs[1:] - offs[:-1] + (window - 1), window, rounding_mode="floor"), 0,
                             out=d_wo[1:])
                wo = d_wo.cpu().numpy()
            nwin = int(wo[-1])
            out = {**self._outputs((("wcount", torch.int32, 0), ("min", torch.float64, 0), ("max", torch.float64, 0),
                                     ("sum", torch.float64, 0)), nwin),
                   **self._outputs((("count", torch.int64, 0), ("flags", torch.int32, 0)), n)}
            ctx.segmented_rollup(series, window, align, d_wo, out["min"], out["max"], out["sum"], out["wcount"],
                                 out["count"], out["flags"])
        return out, wo

    SLIDE_STATS = ("mean", "sum", "max", "min", "wcount")

    def sliding_series(self, ps: PackedSeries, window: int, min_count: int, want=("mean",)) -> dict:
        """The window of ``window`` slots that ends at every slot of every segment of one series
        (krr_segmented_slide): for each name in ``want`` (a subset of ``SLIDE_STATS``) a flat
        DEVICE tensor with one entry per slot, laid out by the series' own offsets — ``mean``,
        ``sum``, ``max``, ``min`` (float64; NaN where fewer than ``min_count`` slots of the
        window are present) and ``wcount`` (int32) — each as large as the series, so they stay
        in HBM and only the ones asked for are allocated and written; ``peak`` (float64: the
        largest emitted mean), ``peak_slot`` (int64: its first slot, -1 without one), ``count``
        (int64) and ``flags`` (uint32) as host arrays [S], and ``offsets`` (host int64 [S + 1]).
        With ``want`` empty the launch reads the series and writes [S] results only.  Chunks as
        ``stats_series``: whole segments, the chunks' slots concatenated on the device."""
        import torch

        window, min_count = int(window), int(min_count)
        want = tuple(k for k in self.SLIDE_STATS if k in set(want))
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        dev = torch.device("cuda", self.device)
        parts = [self._slide_part(ctx, part, window, min_count, want) for part in self._series_parts(ps)]
        if not parts:
            res = {k: torch.empty(0, dtype=torch.int32 if k == "wcount" else torch.float64, device=dev) for k in want}
        elif len(parts) == 1:
            res = {k: parts[0][k] for k in want}
        else:
            res = {k: torch.cat([p[k] for p in parts]) for k in want}
        seg = {"peak": np.float64, "peak_slot": np.int64, "count": np.int64, "flags": np.int32}
        res.update(self._host_concat([{k: p[k] for k in seg} for p in parts], seg))
        offs = ps.offsets if isinstance(ps.offsets, np.ndarray) else ps.offsets.cpu().numpy()
        res["offsets"] = np.asarray(offs, dtype=np.int64)
        return res

    def _slide_part(self, ctx, part: PackedSeries, window: int, min_count: int, want: tuple) -> dict:
        """Upload (host series) and one krr_segmented_slide launch on the current stream: the
        chunk's device tensors, per-slot ones for the names in ``want`` only."""
        import torch

        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            out = {**self._outputs([(k, torch.int32 if k == "wcount" else torch.float64, 0) for k in want],
                                   int(series.n_values)),
                   **self._outputs((("peak", torch.float64, 0), ("peak_slot", torch.int64, 0),
                                    ("count", torch.int64, 0), ("flags", torch.int32, 0)), part.n_segments)}
            ctx.segmented_slide(series, window, min_count, out.get("mean"), out.get("sum"), out.get("max"),
                                out.get("min"), out.get("wcount"), out["peak"], out["peak_slot"], out["count"],
                                out["flags"])
        return out

    def overlay_series(self, ps: PackedSeries, align: int) -> dict:
        """Every object's pods folded slot by slot (krr_pods_overlay; ``align`` KRR_OVERLAY_START
        or KRR_OVERLAY_END): ``active`` (int32), ``sum``, ``max``, ``min`` (float64) as flat
        DEVICE tensors with one entry per object slot — together as large as the series, so they
        stay in HBM — ``offsets`` (host int64 [S + 1]: object s owns slots offsets[s] ..
        offsets[s+1]), ``slots`` (its longest pod) and ``pods`` (int64 [S]), ``count`` (int64)
        and ``flags`` (uint32) as host arrays [S].  The series needs its pod boundaries
        (``pod_view``'s ValueError names the packers), which are validated on the host: pod_groups
        spans the pod segments and does not decrease.  Chunks as ``stats_series``: whole objects,
        the chunks' slots concatenated on the device and their offsets rebased.  The slot offsets
        of a host series come from its host pod offsets; for a series resident in HBM they are
        computed there and read back, the one synchronisation before the outputs are sized."""
        import torch

        from krr_amd.core.packing import pod_view

        if ps.pod_offsets is None or ps.pod_groups is None:
            pod_view(ps)  # raises the ValueError that names the packers
        if isinstance(ps.pod_groups, np.ndarray):
            groups = np.asarray(ps.pod_groups, dtype=np.int64)
            if groups.size != ps.n_segments + 1 or groups[0] != 0 or groups[-1] != ps.n_pods or (np.diff(groups) < 0).any():
                raise ValueError(f"pod_groups must run from 0 to the {ps.n_pods} pod segments in {ps.n_segments} + 1 "
                                 f"non-decreasing entries")
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        dev = torch.device("cuda", self.device)
        parts, offs, pods, base = [], [np.zeros(1, dtype=np.int64)], [], 0
        for part in self._series_parts(ps):
            out, oo, npods = self._overlay_part(ctx, part, align)
            parts.append(out)
            offs.append(oo[1:] + base)
            pods.append(npods)
            base += int(oo[-1])
        names = (("active", torch.int32), ("sum", torch.float64), ("max", torch.float64), ("min", torch.float64))
        if not parts:
            res = {k: torch.empty(0, dtype=dt, device=dev) for k, dt in names}
        elif len(parts) == 1:
            res = {k: parts[0][k] for k, _ in names}
        else:
            res = {k: torch.cat([p[k] for p in parts]) for k, _ in names}
        host = self._host_concat([{k: p[k] for k in ("count", "flags")} for p in parts],
                                 {"count": np.int64, "flags": np.int32})
        offsets = np.concatenate(offs)
        res.update(offsets=offsets, slots=np.diff(offsets),
                   pods=np.concatenate(pods) if pods else np.zeros(0, dtype=np.int64),
                   count=host["count"], flags=host["flags"])
        return res

    def _overlay_part(self, ctx, part: PackedSeries, align: int) -> tuple:
        """Upload (host series) and one krr_pods_overlay launch on the current stream: the chunk's
        device tensors, its slot offsets and its pods per object as host arrays."""
        import torch

        dev = torch.device("cuda", self.device)
        n = part.n_segments
        with torch.cuda.device(self.device):
            if isinstance(part.pod_groups, np.ndarray):
                po = np.ascontiguousarray(part.pod_offsets, dtype=np.int64)
                groups = np.ascontiguousarray(part.pod_groups, dtype=np.int64)
                npods = np.diff(groups)
                lg = np.zeros(n, dtype=np.int64)
                np.maximum.at(lg, np.repeat(np.arange(n, dtype=np.int64), npods), np.diff(po))
                oo = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lg, out=oo[1:])
                vals, _ = self._to_device(part)
                d_po, d_groups, d_oo = (torch.from_numpy(a).to(dev) for a in (po, groups, oo))
                longest = int(lg.max(initial=0))
            else:
                vals, _ = self._to_device(part)
                d_po, d_groups = part.pod_offsets.contiguous(), part.pod_groups.contiguous()
                if d_po.device != dev or d_groups.device != dev:
                    raise ValueError(f"pod boundaries on {d_po.device}, engine runs on {dev}: pack on the engine's device")
                n_pods = d_po.numel() - 1
                if d_groups.numel() != n + 1:
                    raise ValueError(f"pod_groups holds {d_groups.numel()} entries for {n} objects")
                per = d_groups[1:] - d_groups[:-1]
                ok = (d_groups[0] == 0) & (d_groups[-1] == n_pods) & (per >= 0).all()
                owner = torch.searchsorted(d_groups[1:].contiguous(), torch.arange(n_pods, device=dev), right=True)
                lg = torch.zeros(n, dtype=torch.int64, device=dev)
                if n_pods > 0:
                    lg.scatter_reduce_(0, owner.clamp_(0, max(n - 1, 0)), d_po[1:] - d_po[:-1], "amax")
                d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum(lg, 0, out=d_oo[1:])
                back = torch.cat([d_oo, per, ok.to(torch.int64).reshape(1)]).cpu().numpy()  # the one synchronisation
                if not back[-1]:
                    raise ValueError(f"pod_groups must run from 0 to the {n_pods} pod segments in {n} + 1 "
                                     f"non-decreasing entries")
                oo, npods = back[:n + 1], back[n + 1:2 * n + 1]
                longest = int(np.diff(oo).max(initial=0))
            series = ctx.series(vals, d_po, max(longest, 1), part.gaps_are_nan)
            out = {**self._outputs((("active", torch.int32, 0), ("sum", torch.float64, 0), ("max", torch.float64, 0),
                                     ("min", torch.float64, 0)), int(oo[-1])),
                   **self._outputs((("count", torch.int64, 0), ("flags", torch.int32, 0)), n)}
            ctx.pods_overlay(series, d_groups, n, align, d_oo, out["sum"], out["max"], out["min"], out["active"],
                             out["count"], out["flags"])
        return out, oo, npods

    def percentiles_series(self, ps: PackedSeries, params_list) -> tuple:
        """Several percentiles of every segment of one series — CPU or memory — through
        krr_segmented_percentiles: (value float64 [P, S], count int64 [S], flags uint32 [P, S]),
        host arrays, row j for ``params_list[j]`` (entries of one mode).  Lists longer than
        KRR_MAX_PERCENTILES run in groups; index tables are bound per launch from the chunk's
        longest segment, as ``run_packed_multi`` binds them.  Chunks and synchronisation as
        ``stats_series``."""
        params_list = list(params_list)
        if not params_list:
            raise ValueError("at least one percentile")
        ctx = self.context()
        parts = [self._percentiles_part(ctx, part, params_list) for part in self._series_parts(ps)]
        host = self._host_concat(parts, {"value": np.float64, "count": np.int64, "flags": np.int32},
                                 rows={"value": len(params_list), "flags": len(params_list)})
        return host["value"], host["count"], host["flags"]

    def _series_parts(self, ps: PackedSeries):
        """The whole-segment ranges one series runs as — ``_chunk_bounds``' rule for a single
        resource: whole when resident in HBM or within two chunks of values, else
        sample-balanced chunks of about ``chunk_bytes``."""
        import torch

        from krr_amd.core.distributed import shard_bounds, slice_series

        S = ps.n_segments
        if S == 0:
            return
        resident = isinstance(ps.values, torch.Tensor) and ps.values.is_cuda
        nbytes = 0 if resident else 8 * int(ps.offsets[-1])
        n = 1 if resident or nbytes <= 2 * self.chunk_bytes else -(-nbytes // self.chunk_bytes)
        if n == 1:
            yield ps
            return
        for lo, hi in shard_bounds(np.diff(ps.offsets), n):
            if hi > lo:
                yield slice_series(ps, lo, hi)

    def _part_series(self, ctx, part: PackedSeries):
        vals, offs = self._to_device(part)
        return ctx.series(vals, offs, max(int(part.max_len), 1), part.gaps_are_nan)

    def _stats_part(self, ctx, part: PackedSeries) -> dict:
        """Upload (host series) and one krr_segmented_stats launch on the current stream: the
        chunk's device tensors."""
        import torch

        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            out = self._outputs((("min", torch.float64, 0), ("max", torch.float64, 0), ("sum", torch.float64, 0),
                                 ("count", torch.int64, 0), ("flags", torch.int32, 0)), part.n_segments)
            ctx.segmented_stats(series, out["min"], out["max"], out["sum"], out["count"], out["flags"])
        return out

    def _moments_part(self, ctx, part: PackedSeries, trend: bool) -> dict:
        """Upload (host series) and one krr_segmented_moments launch on the current stream: the
        chunk's device tensors (without ``trend``: no tmean / t2 / cxt)."""
        import torch

        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            names = ("mean", "m2", "tmean", "t2", "cxt") if trend else ("mean", "m2")
            out = self._outputs([*((k, torch.float64, 0) for k in names), ("count", torch.int64, 0),
                                 ("flags", torch.int32, 0)], part.n_segments)
            ctx.segmented_moments(series, out["mean"], out["m2"], out.get("tmean"), out.get("t2"), out.get("cxt"),
                                  out["count"], out["flags"])
        return out

    def _exceed_part(self, ctx, part: PackedSeries, thresholds: np.ndarray) -> dict:
        """Upload (host series, and the chunk's thresholds [R, n], R <= KRR_MAX_THRESHOLDS) and
        one krr_segmented_exceed launch on the current stream: the six outputs [R, n] and the
        count / flags [n] as device tensors."""
        import torch

        dev = torch.device("cuda", self.device)
        R, n = thresholds.shape
        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            thr = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float64)).to(dev)
            out = self._outputs((*((k, torch.int64, R) for k in ("above", "longest", "head", "tail", "last")),
                                 ("excess", torch.float64, R), ("count", torch.int64, 0), ("flags", torch.int32, 0)), n)
            ctx.segmented_exceed(series, thr, R, out["above"], out["excess"], out["longest"], out["head"],
                                 out["tail"], out["last"], out["count"], out["flags"])
        return out

    def _upload_table(self, tab: np.ndarray):
        """A uint64 weight table in HBM, as the int64 storage the binding takes."""
        import torch

        return torch.from_numpy(tab.view(np.int64)).to(torch.device("cuda", self.device))

    def _wquantile_part(self, ctx, part: PackedSeries, table, p_num: int, p_den: int) -> dict:
        """Upload (host series) and one krr_segmented_wquantile launch on the current stream with
        the weight table ``table`` (int64 storage, already on the device): the chunk's device
        tensors."""
        import torch

        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            out = self._outputs((("value", torch.float64, 0), ("wsum", torch.int64, 0), ("passes", torch.int32, 0),
                                 ("count", torch.int64, 0), ("flags", torch.int32, 0)), part.n_segments)
            ctx.segmented_wquantile(series, table, p_num, p_den, out["value"], out["wsum"], out["passes"],
                                    out["count"], out["flags"])
        return out

    def _whist_part(self, ctx, part: PackedSeries, table, bins, width: int, age_base) -> dict:
        """Upload (host series, and the chunk's ``age_base`` when there is one) and one
        krr_segmented_whist launch on the current stream with the weight table ``table`` (int64
        storage, already on the device): the chunk's device tensors, ``hist`` [n, width]."""
        import torch

        dev = torch.device("cuda", self.device)
        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            base = None if age_base is None else torch.from_numpy(np.array(age_base, dtype=np.int64)).to(dev)
            out = self._outputs((("wsum", torch.int64, 0), ("wmin", torch.float64, 0), ("wmax", torch.float64, 0),
                                 ("count", torch.int64, 0), ("flags", torch.int32, 0)), part.n_segments)
            out["hist"] = torch.empty((part.n_segments, width), dtype=torch.int64, device=dev)
            ctx.segmented_whist(series, bins, table, base, out["hist"], out["wsum"], out["wmin"], out["wmax"],
                                out["count"], out["flags"])
        return out

    def _resident(self, part: PackedSeries) -> PackedSeries:
        """The chunk with its values and offsets in HBM (as it is when it is there already), for
        several launches over one upload."""
        vals, offs = self._to_device(part)
        return PackedSeries(vals, offs, int(part.max_len), part.gaps_are_nan)

    def _percentiles_part(self, ctx, part: PackedSeries, params_list: list) -> dict:
        """Upload (host series) and krr_segmented_percentiles per group of KRR_MAX_PERCENTILES
        entries on the current stream: value / flags [P, n] and the shared count [n]."""
        import torch

        dev = torch.device("cuda", self.device)
        P, n, G = len(params_list), part.n_segments, _native.KRR_MAX_PERCENTILES
        with torch.cuda.device(self.device):
            series = self._part_series(ctx, part)
            value = torch.empty((P, n), dtype=torch.float64, device=dev)
            flags = torch.empty((P, n), dtype=torch.int32, device=dev)
            count = torch.empty(n, dtype=torch.int64, device=dev)
            for a in range(0, P, G):
                ctx.segmented_percentiles(series, params_list[a:a + G], value[a:a + G], count, flags[a:a + G])
        return {"value": value, "count": count, "flags": flags}

    def _host_concat(self, parts: list, dtypes: dict, rows: Optional[dict] = None) -> dict:
        """The chunks' tensors as host arrays, concatenated in segment order (the last axis), the
        int32 ``flags`` the kernels wrote viewed as the uint32 they are; synchronises the current
        stream once, before the first copy."""
        import torch

        rows = rows or {}
        if not parts:  # a series without segments launches nothing
            host = {k: np.zeros((rows[k], 0) if k in rows else 0, dtype=dt) for k, dt in dtypes.items()}
        else:
            if any(t.is_cuda for p in parts for t in p.values()):
                torch.cuda.current_stream(self.device).synchronize()
            host = {k: np.concatenate([p[k].cpu().numpy() for p in parts], axis=-1) for k in dtypes}
        if "flags" in host:
            host["flags"] = host["flags"].view(np.uint32)
        return host

    def _outputs(self, spec, n: int) -> dict:
        """Uninitialised device tensors for one launch: per ``(name, dtype, rows)`` of ``spec`` a
        [rows, n] tensor, [n] where rows is 0."""
        import torch

        dev = torch.device("cuda", self.device)
        return {k: torch.empty((rows, n) if rows else (n,), dtype=dt, device=dev) for k, dt, rows in spec}

    def run_packed_multi(self, fleet: PackedFleet, params_list, aggregation: str = "concat",
                         return_pods: bool = False) -> list:
        """Several CPU percentiles of a fleet (host- or device-packed) from one fused pass per
        chunk (krr_simple_run_multi): one RawResults per entry of ``params_list``, sharing the
        memory arrays and the CPU counts, so ``krr_amd.core.exact.resolve`` and
        ``cpu_from_raw`` work per percentile unchanged.  HistoryData segments of exactness
        class >= 1 are located per percentile (``_locate_chunk``).  ``aggregation`` "pods_max":
        every percentile per pod and its max over the object's pods (krr_simple_run_pods_multi;
        the CPU series needs pod boundaries); ``return_pods`` then adds each percentile's
        pod-level results (RawResults.pods, as run_packed's)."""
        import torch

        params_list = list(params_list)
        if aggregation not in ("concat", "pods_max"):
            raise ValueError(f"unknown cpu aggregation {aggregation!r}; expected 'concat' or 'pods_max'")
        if fleet.cpu.n_segments != fleet.mem.n_segments:
            raise ValueError("cpu and memory need one segment per object each")
        ctx = self.context()  # raises NativeUnavailable without the HIP library or a device
        if aggregation == "pods_max":
            return self._run_packed_multi_pods(fleet, params_list, return_pods)
        S, P = fleet.n_objects, len(params_list)
        if S == 0:
            return [_empty_results() for _ in range(P)]
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(self.device):
            out = {k: torch.empty(shape, dtype=dt, device=dev) for k, dt, shape in
                   (("cpu_value", torch.float64, (P, S)), ("cpu_count", torch.int64, (S,)),
                    ("cpu_flags", torch.int32, (P, S)), ("mem_value", torch.float64, (S,)),
                    ("mem_count", torch.int64, (S,)), ("mem_flags", torch.int32, (S,)))}
            locs = [None] * P
            for j, params in enumerate(params_list):
                if needs_locate(fleet, params):
                    locs[j] = {r: tuple(np.full(S, -1, dtype=np.int64) for _ in range(3)) for r in ("cpu", "mem")}
            for lo, hi, part, cs, ms in self._chunks(fleet):
                n = hi - lo
                whole = n == S
                # a chunk's rows are not contiguous in the [P, S] outputs: its own [P, n] block
                chunk = out if whole else {k: torch.empty((P, n) if v.dim() == 2 else (n,), dtype=v.dtype, device=dev)
                                           for k, v in out.items()}
                ctx.simple_run_multi(cs, ms, params_list, chunk)
                if not whole:
                    for k, v in out.items():
                        v[..., lo:hi] = chunk[k]
                for j, params in enumerate(params_list):
                    if locs[j] is not None:
                        one = dict(chunk, cpu_value=chunk["cpu_value"][j], cpu_flags=chunk["cpu_flags"][j])
                        self._locate_chunk(ctx, part, cs, ms, params, one, locs[j], lo)
            torch.cuda.current_stream(self.device).synchronize()
        host = {k: v.cpu().numpy() for k, v in out.items()}
        return [RawResults(host["cpu_value"][j], host["cpu_count"], host["cpu_flags"][j].view(np.uint32),
                           host["mem_value"], host["mem_count"], host["mem_flags"].view(np.uint32), locs[j])
                for j in range(P)]

    def _run_packed_multi_pods(self, fleet: PackedFleet, params_list: list, return_pods: bool) -> list:
        """run_packed_multi under "pods_max": krr_simple_run_pods_multi per chunk over its pod
        segments (``_run_chunks_pods`` for a set of percentiles), each chunk into [P, n] blocks
        of its own.  The memory side is located once (every RawResults shares the answers); the
        CPU side per percentile over the pod segments, under ``_run_chunks_pods``' condition."""
        import torch

        from krr_amd.core.packing import PackedSeries, pod_view

        if fleet.cpu.pod_offsets is None or fleet.cpu.pod_groups is None:
            pod_view(fleet.cpu)  # raises the ValueError that names the packer
        S, P, n_pods = fleet.n_objects, len(params_list), fleet.cpu.n_pods
        if S == 0:
            return [_empty_results() for _ in range(P)]
        ctx = self.context()
        dev = torch.device("cuda", self.device)
        obj_keys = (("cpu_value", torch.float64, P), ("cpu_count", torch.int64, 0), ("cpu_flags", torch.int32, P),
                    ("cpu_pod", torch.int64, P), ("mem_value", torch.float64, 0), ("mem_count", torch.int64, 0),
                    ("mem_flags", torch.int32, 0))
        pod_keys = (("pod_value", torch.float64, P), ("pod_count", torch.int64, 0), ("pod_flags", torch.int32, P))


        locate = any(needs_locate(fleet, params) for params in params_list)
        loc = {r: tuple(np.full(S, -1, dtype=np.int64) for _ in range(3)) for r in ("cpu", "mem")} if locate else None
        pod_locs = [None] * P
        if fleet.cpu.exact is not None:
            for j, params in enumerate(params_list):
                if params.mode == _native.KRR_PCT_SORTED_LOWER:
                    pod_locs[j] = {"cpu": tuple(np.full(n_pods, -1, dtype=np.int64) for _ in range(3))}
        with torch.cuda.device(self.device):
            out = self._outputs(obj_keys, S)
            pod_chunks = {k: [] for k, _, _ in pod_keys}
            pod_lo = 0
            for lo, hi, part, cs, ms in self._chunks(fleet):
                view, pg, pcs = self._pod_series(ctx, part, cs)
                n = view.n_segments
                whole = hi - lo == S
                # a chunk's rows are not contiguous in the [P, S] outputs: its own [P, n] block
                chunk = dict(out if whole else self._outputs(obj_keys, hi - lo), **self._outputs(pod_keys, n))
                ctx.simple_run_pods_multi(pcs, pg, ms, params_list, chunk)
                if not whole:
                    for k, v in out.items():
                        v[..., lo:hi] = chunk[k]
                for k in pod_chunks:
                    pod_chunks[k].append(chunk[k])
                if locate:
                    self._locate_chunk(ctx, part, cs, ms, params_list[0], chunk, loc, lo, names=("mem",))
                for j, params in enumerate(params_list):
                    if pod_locs[j] is not None and view.exact is not None:
                        pod_out = {"cpu_value": chunk["pod_value"][j], "cpu_count": chunk["pod_count"],
                                   "cpu_flags": chunk["pod_flags"][j]}
                        self._locate_chunk(ctx, PackedFleet(view, PackedSeries(part.mem.values, part.mem.offsets, 0)),
                                           pcs, ms, params, pod_out, pod_locs[j], pod_lo, names=("cpu",))
                pod_lo += n
            torch.cuda.current_stream(self.device).synchronize()
        host = {k: v.cpu().numpy() for k, v in out.items()}
        raws = [RawResults(host["cpu_value"][j], host["cpu_count"], host["cpu_flags"][j].view(np.uint32),
                           host["mem_value"], host["mem_count"], host["mem_flags"].view(np.uint32), loc)
                for j in range(P)]
        if return_pods:
            pod = {k: torch.cat(v, dim=-1).cpu().numpy() for k, v in pod_chunks.items()}  # S > 0: >= 1 chunk
            for j, raw in enumerate(raws):
                raw.pods = {"pod_value": pod["pod_value"][j], "pod_count": pod["pod_count"],
                            "pod_flags": pod["pod_flags"][j].view(np.uint32), "cpu_pod": host["cpu_pod"][j],
                            "locate": pod_locs[j]}
        return raws

    def _locate_chunk(self, ctx, part: PackedFleet, cs, ms, params, out: dict, loc: dict, lo: int,
                      names=("cpu", "mem")) -> None:
        """krr_locate for the chunk's class >= 1 segments that select one sample: memory
        (rank -1: the first maximal element, simple.py:29) and SORTED_LOWER CPU (rank k of
        the stable sort).  REF_INDEX needs no search (its position IS k) and LINEAR is defined
        on the float64 values.  Synchronises the stream (the ranks come from the counts)."""
        import torch

        torch.cuda.current_stream(self.device).synchronize()
        dev = torch.device("cuda", self.device)
        for name, ps, series in (("cpu", part.cpu, cs), ("mem", part.mem, ms)):
            if ps.exact is None or name not in names:
                continue
            rank = locate_ranks(name, ps.exact, out[f"{name}_count"].cpu().numpy(),
                                out[f"{name}_flags"].cpu().numpy(), params)
            if rank is None:
                continue
            rank_d = torch.from_numpy(rank).to(dev)
            lt, eq, pos = (torch.full_like(rank_d, -1) for _ in range(3))
            ctx.locate(series, out[f"{name}_value"], rank_d, lt, eq, pos)
            for dst, src in zip(loc[name], (lt, eq, pos)):
                dst[lo:lo + src.numel()] = src.cpu().numpy()


def locate_ranks(name: str, exact: np.ndarray, count: np.ndarray, flags: np.ndarray, params) -> Optional[np.ndarray]:
    """krr_locate's rank per segment ("cpu" | "mem"): -1 (the first maximal sample) for memory,
    k = floor((n-1)·p/100) for SORTED_LOWER CPU, on class >= 1 segments holding >= 2 samples and
    no NaN (those answer by the NaN rules); -2 (skip) elsewhere.  None: nothing to locate."""
    if name == "cpu" and params.mode != _native.KRR_PCT_SORTED_LOWER:
        return None
    flags = np.asarray(flags).astype(np.uint32)
    ok = (np.asarray(exact) > 0) & (flags & (_native.KRR_FLAG_EMPTY | _native.KRR_FLAG_NAN) == 0) & (count >= 2)
    if not ok.any():
        return None
    rank = np.full(count.size, -2, dtype=np.int64)
    if name == "mem":
        rank[ok] = -1
    else:
        rank[ok] = index_rule_of(params).ks(np.asarray(count)[ok])
    return rank


def index_rule_of(params):
    """The IndexRule a params struct carries (percentile_params), or the exact p_num / p_den one."""
    rule = getattr(params, "rule", None)
    if rule is None:
        from fractions import Fraction

        from krr_amd.core.index_rule import IndexRule

        rule = IndexRule.of(Fraction(int(params.p_num), int(params.p_den)))
    return rule


def needs_locate(fleet: PackedFleet, params) -> bool:
    """Does a fleet hold HistoryData segments whose answer must be located (krr_locate)?"""
    return fleet.cpu.exact is not None and params.mode == _native.KRR_PCT_SORTED_LOWER or fleet.mem.exact is not None


def pinned_alloc(n: int) -> np.ndarray:
    """float64[n] in page-locked host memory (a numpy view that keeps its torch
    tensor alive): pass as ``alloc`` to the packers so the H2D copy runs by DMA."""
    import torch

    return torch.empty(max(int(n), 1), dtype=torch.float64, pin_memory=True).numpy()[: int(n)]


_default_engines: dict[int, SimpleEngine] = {}
_engines_lock = threading.Lock()


def default_engine(device: int = 0) -> SimpleEngine:
    with _engines_lock:
        eng = _default_engines.get(device)
        if eng is None:
            eng = _default_engines[device] = SimpleEngine(device)
        return eng

"""Fleet statistics for custom strategies: what a plugin's ``run_batch`` calls.

``BatchedRunner.raw_results`` hands a strategy that implements ``run_batch(histories, objects)``
the whole fleet at once.  ``FleetBatch`` turns that fleet into per-object float64 arrays computed
on the device, one launch per statistic instead of a Python loop per object:

    batch = FleetBatch(histories, device=0)        # packs each resource on first use, once
    batch = FleetBatch.from_fleet(packed_fleet)    # a PackedFleet (e.g. BatchedRunner.pack_from_bodies)
    st = batch.stats(ResourceType.Memory)          # FleetStats: count, min, max, sum, flags (+ .mean)
    mo = batch.moments(ResourceType.Memory)        # FleetMoments: mean, m2, trend (+ .std(), .slope, ...)
    ex = batch.exceedance(ResourceType.CPU, allocation_thresholds(objects, ResourceType.CPU))
                                                   # FleetExceedance: above, excess, longest run, ... per threshold
    v = batch.percentile(ResourceType.Memory, "95", mode="sorted_lower")         # float64 [S]
    vs = batch.percentiles(ResourceType.CPU, ["50", "95", "99"], mode="linear")  # float64 [P, S]
    pods = batch.per_pod(ResourceType.CPU)         # a FleetBatch over one segment per pod + .pod_groups
    ov = batch.overlay(ResourceType.CPU)           # FleetOverlay: an object's pods folded slot by slot
    w = batch.weighted_percentile(ResourceType.CPU, "95", decay_weights(1440, 10080))  # recency-weighted, exact
    h = batch.histogram(ResourceType.CPU, decay_weights(1440, 10080))  # FleetHistogram: mergeable, many percentiles
    batch.to_decimal(values, flags)                # list[Decimal]

``stats`` is one krr_segmented_stats pass (min and max are the first minimal / maximal sample's own
bits, Python ``min()`` / ``max()``; the sum is a plain float64 sum, include/krr_amd.h);
``percentiles`` is krr_segmented_percentiles over ANY series, memory included, with the three
rules of ``SimpleStrategySettings.percentile_mode``.  There is no CPU path: without the HIP
library or a device every computing call raises ``NativeUnavailable``.

Values are float64.  ``to_decimal`` gives each float's shortest string as a Decimal
(``prom_decimal``: the Decimal the reference's loader parses from Prometheus).  For HistoryData
whose Decimals are NOT Prometheus' strings ('0.10', 25-digit values: ``PackedSeries.exact``) that
is an equal-valued or nearest Decimal, not the caller's own object; ``exact_mask`` names those
objects so a strategy can send them through its per-object ``run()`` instead.
"""
from __future__ import annotations

import decimal
from dataclasses import dataclass
from decimal import Decimal
from typing import Mapping, Optional, Sequence

import numpy as np

from krr_amd import _native
from krr_amd.core.engine import (MODE_CODES, WEIGHT_MAX, SimpleEngine, default_engine, percentile_fraction,
                                 percentile_params, weight_table)
from krr_amd.core.models.allocations import ResourceType
from krr_amd.core.packing import PackedFleet, PackedSeries, pack_resource, pod_view
from krr_amd.utils.prom_decimal import prom_decimal

__all__ = ["FleetBatch", "FleetExceedance", "FleetHistogram", "FleetMoments", "FleetOverlay", "FleetProfile",
           "FleetRollup", "FleetStats", "HistogramBins", "allocation_thresholds", "decay_weights", "default_bins",
           "window_weights"]


@dataclass
class FleetStats:
    """Per-object statistics of one resource (host arrays, [S] each).  ``count`` is the present
    samples; ``flags`` the kernels' KRR_FLAG_* (EMPTY: no sample, min = max = NaN and sum = 0;
    NAN: a NaN sample, min = max = sum = NaN)."""
    count: np.ndarray  # int64
    min: np.ndarray    # float64
    max: np.ndarray    # float64
    sum: np.ndarray    # float64
    flags: np.ndarray  # uint32

    @property
    def mean(self) -> np.ndarray:
        """sum / count in float64; NaN where count == 0."""
        out = np.full(self.count.shape, np.nan, dtype=np.float64)
        np.divide(self.sum, self.count, out=out, where=self.count > 0)
        return out


@dataclass
class FleetMoments:
    """Per-object moments of one resource (host arrays, [S] each): what variance and a linear
    trend need, and mergeable (``concat``).  With P the present slots of an object's series, slot
    i = 0 .. slots-1 counted from the series' start (the time grid of the gapped layout, the
    sample index of the compact one) and n = ``count``:

        mean = sum_P x / n        m2 = sum_P (x - mean)^2
        tmean = sum_P i / n       t2 = sum_P (i - tmean)^2       cxt = sum_P (i - tmean)(x - mean)

    ``tmean``, ``t2`` and ``cxt`` are None on a result asked for without the trend; the trend
    accessors then raise ValueError.  ``flags`` are the kernels' KRR_FLAG_* (EMPTY: no sample;
    NAN: a NaN sample): all moments of a flagged object are NaN."""
    count: np.ndarray            # int64
    mean: np.ndarray             # float64
    m2: np.ndarray               # float64
    tmean: Optional[np.ndarray]  # float64
    t2: Optional[np.ndarray]     # float64
    cxt: Optional[np.ndarray]    # float64
    flags: np.ndarray            # uint32
    slots: np.ndarray            # int64: each series' length in slots

    @property
    def has_trend(self) -> bool:
        return self.tmean is not None and self.t2 is not None and self.cxt is not None

    def _need_trend(self, what: str) -> None:
        if not self.has_trend:
            raise ValueError(f"{what} needs the trend moments: ask for moments(resource, trend=True)")

    def variance(self, ddof: int = 0) -> np.ndarray:
        """m2 / (count - ddof); NaN where count - ddof <= 0."""
        d = self.count - ddof
        out = np.full(self.count.shape, np.nan, dtype=np.float64)
        np.divide(self.m2, d, out=out, where=d > 0)
        return out

    def std(self, ddof: int = 0) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.variance(ddof))

    @property
    def slope(self) -> np.ndarray:
        """Least-squares slope per slot, cxt / t2; NaN where t2 is not > 0 (fewer than two
        distinct slots)."""
        self._need_trend("slope")
        out = np.full(self.count.shape, np.nan, dtype=np.float64)
        np.divide(self.cxt, self.t2, out=out, where=self.t2 > 0)
        return out

    @property
    def intercept(self) -> np.ndarray:
        """The fitted value at slot 0: mean - slope * tmean."""
        return self.mean - self.slope * self.tmean

    @property
    def r2(self) -> np.ndarray:
        """The fit's coefficient of determination, min(1, cxt^2 / (t2 m2)); NaN where t2 or m2
        is not > 0."""
        self._need_trend("r2")
        ok = (self.t2 > 0) & (self.m2 > 0)
        out = np.full(self.count.shape, np.nan, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            np.divide(self.cxt * self.cxt, self.t2 * self.m2, out=out, where=ok)
        return np.where(ok, np.minimum(out, 1.0), np.nan)

    def value_at(self, slot) -> np.ndarray:
        """The fitted line at ``slot`` (a scalar or an array [S]): mean + slope * (slot - tmean)."""
        return self.mean + self.slope * (np.asarray(slot, dtype=np.float64) - self.tmean)

    def forecast(self, ahead) -> np.ndarray:
        """The fitted line ``ahead`` slots after each series' last slot."""
        return self.value_at(self.slots - 1 + np.asarray(ahead, dtype=np.float64))

    def concat(self, other: "FleetMoments") -> "FleetMoments":
        """The moments of each series followed by ``other``'s (``other``'s slot i becomes slot
        ``self.slots + i``), from the two results alone: Chan, Golub and LeVeque's update in
        float64.  An empty side is the identity.  Flags are OR-ed, except EMPTY, which survives
        only where both sides are empty.  Without the trend on either side the result has none."""
        if self.count.shape != other.count.shape:
            raise ValueError("concat needs the same objects on both sides")
        na, nb = self.count.astype(np.float64), other.count.astype(np.float64)
        ea, eb = self.count == 0, other.count == 0
        n = na + nb
        w = nb / np.where(n > 0, n, 1.0)
        q = na * w

        def pick(a, b, merged):
            return np.where(ea, b, np.where(eb, a, merged))

        with np.errstate(invalid="ignore", over="ignore"):
            dx = other.mean - self.mean
            mean = pick(self.mean, other.mean, self.mean + dx * w)
            m2 = pick(self.m2, other.m2, (self.m2 + other.m2) + (dx * dx) * q)
            tmean = t2 = cxt = None
            if self.has_trend and other.has_trend:
                tb = other.tmean + self.slots
                dt = tb - self.tmean
                tmean = pick(self.tmean, tb, self.tmean + dt * w)
                t2 = pick(self.t2, other.t2, (self.t2 + other.t2) + (dt * dt) * q)
                cxt = pick(self.cxt, other.cxt, (self.cxt + other.cxt) + (dx * dt) * q)
        empty = np.uint32(_native.KRR_FLAG_EMPTY)
        fa, fb = self.flags.astype(np.uint32), other.flags.astype(np.uint32)
        flags = ((fa | fb) & ~empty) | (fa & fb & empty)
        return FleetMoments(self.count + other.count, mean, m2, tmean, t2, cxt, flags, self.slots + other.slots)


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@dataclass
class FleetExceedance:
    """Per object and threshold, how the samples lie above the threshold (host arrays): what
    "how often, and for how long at a stretch, was usage above this number?" needs, and mergeable
    (``concat``).  A sample is above when ``x > threshold`` (strict); a threshold of NaN or +Inf
    has nothing above it ("no request set").  Absent slots of the gapped layout are transparent:
    they neither count nor end a run, so a run is a sequence of consecutive PRESENT samples that
    are all above.

    [R, S], row r for ``thresholds[r]``: ``above`` (samples above), ``excess`` (sum of x -
    threshold over them, float64: "core-slots over the request"), ``longest`` (longest run),
    ``head`` / ``tail`` (the runs at the series' first / last present sample; ``tail`` is
    "currently over for this many samples"), ``last`` (slot of the last sample above, -1 if none).
    [S]: ``count`` (present samples), ``flags`` (the kernels' KRR_FLAG_*: EMPTY: no sample; NAN: a
    NaN sample, then ``excess`` is NaN and the integers are 0), ``slots`` (each series' length)."""
    above: np.ndarray       # int64 [R, S]
    excess: np.ndarray      # float64 [R, S]
    longest: np.ndarray     # int64 [R, S]
    head: np.ndarray        # int64 [R, S]
    tail: np.ndarray        # int64 [R, S]
    last: np.ndarray        # int64 [R, S]
    thresholds: np.ndarray  # float64 [R, S]
    count: np.ndarray       # int64 [S]
    flags: np.ndarray       # uint32 [S]
    slots: np.ndarray       # int64 [S]

    @property
    def share(self) -> np.ndarray:
        """above / count: the part of the samples above the threshold; NaN where count == 0."""
        out = np.full(self.above.shape, np.nan, dtype=np.float64)
        np.divide(self.above, self.count, out=out, where=np.broadcast_to(self.count > 0, self.above.shape))
        return out

    @property
    def mean_excess(self) -> np.ndarray:
        """excess / above: how far above the threshold a breaching sample lies on average; NaN
        where nothing is above."""
        out = np.full(self.above.shape, np.nan, dtype=np.float64)
        np.divide(self.excess, self.above, out=out, where=self.above > 0)
        return out

    @property
    def since_last(self) -> np.ndarray:
        """slots - 1 - last: the slots since the last sample above; -1 where there is none."""
        return np.where(self.last >= 0, self.slots - 1 - self.last, -1)

    def concat(self, other: "FleetExceedance") -> "FleetExceedance":
        """The result of each series followed by ``other``'s (``other``'s slot i becomes slot
        ``self.slots + i``), from the two results alone: counts and excess add, and the runs
        merge as run statistics do,

            head = self.head == self.count ? self.count + other.head : self.head
            tail = other.tail == other.count ? other.count + self.tail : other.tail
            longest = max(self.longest, other.longest, self.tail + other.head)

        with an empty side the identity.  ``last`` is ``self.slots + other.last`` where ``other``
        has a sample above, else ``self.last``.  Flags are OR-ed, except EMPTY, which survives
        only where both sides are empty.  Raises ValueError unless both sides hold the same
        objects and bitwise the same thresholds (NaN equals NaN)."""
        if self.count.shape != other.count.shape or self.above.shape != other.above.shape:
            raise ValueError("concat needs the same objects and thresholds on both sides")
        if not _same_bits(self.thresholds, other.thresholds):
            raise ValueError("concat needs bitwise the same thresholds on both sides")
        na, nb = self.count, other.count
        head = np.where(self.head == na, na + other.head, self.head)
        tail = np.where(other.tail == nb, nb + self.tail, other.tail)
        longest = np.maximum(np.maximum(self.longest, other.longest), self.tail + other.head)
        last = np.where(other.last >= 0, self.slots + other.last, self.last)
        empty = np.uint32(_native.KRR_FLAG_EMPTY)
        fa, fb = self.flags.astype(np.uint32), other.flags.astype(np.uint32)
        flags = ((fa | fb) & ~empty) | (fa & fb & empty)
        return FleetExceedance(self.above + other.above, self.excess + other.excess, longest, head, tail, last,
                               self.thresholds, na + nb, flags, self.slots + other.slots)


_ROLLUP_ALIGN = {"start": _native.KRR_ROLLUP_START, "end": _native.KRR_ROLLUP_END}
_ROLLUP_SERIES_STATS = ("min", "max", "sum", "mean")
_ROLLUP_STATS = ("wcount",) + _ROLLUP_SERIES_STATS


@dataclass
class FleetProfile:
    """``FleetRollup.fold(period)``: per object and position mod ``period`` the windows combined
    (host arrays [S, period]).  ``count`` is the present samples, ``min`` / ``max`` NaN and ``sum``
    0 where ``count`` is 0; a column that took a NaN window (a NaN sample in the compact layout)
    is NaN in ``min``, ``max`` and ``sum``."""
    count: np.ndarray  # int64 [S, period]
    min: np.ndarray    # float64
    max: np.ndarray    # float64
    sum: np.ndarray    # float64

    @property
    def mean(self) -> np.ndarray:
        """sum / count in float64; NaN where count == 0."""
        out = np.full(self.count.shape, np.nan, dtype=np.float64)
        np.divide(self.sum, self.count, out=out, where=self.count > 0)
        return out


class _FlatPerObject:
    """What FleetRollup and FleetOverlay share: flat per-entry tensors where the kernel left them,
    object s owning entries ``offsets[s] .. offsets[s+1]``; a host copy per stat on first use;
    ``of`` and ``dense``.  A subclass sets ``offsets``, ``align`` and ``_t`` (the kernel's tensors
    by stat), names its stats in ``_STATS`` and its per-entry count in ``_COUNT``."""
    _STATS: tuple = ()
    _COUNT: str = ""

    @property
    def n_objects(self) -> int:
        return self.offsets.size - 1

    @classmethod
    def _stat(cls, stat: str, allowed=None) -> str:
        allowed = cls._STATS if allowed is None else allowed
        if stat not in allowed:
            raise ValueError(f"unknown stat {stat!r}; expected one of {list(allowed)}")
        return stat

    def tensor(self, stat: str):
        """The flat tensor of ``stat`` where the kernel left it (HBM): the count int32, the others
        float64; ``mean`` is sum / count computed there, NaN where the count is 0."""
        import torch

        stat = self._stat(stat)
        t = self._t.get(stat)
        if t is None:  # mean
            n = self._t[self._COUNT]
            t = self._t["mean"] = torch.where(n > 0, self._t["sum"] / n.to(torch.float64),
                                              torch.full_like(self._t["sum"], float("nan")))
        return t

    def _flat(self, stat: str) -> np.ndarray:
        a = self._host.get(stat)
        if a is None:
            a = self._host[stat] = self.tensor(stat).cpu().numpy()
        return a

    def of(self, s: int, stat: str = "mean") -> np.ndarray:
        """The entries of object ``s``, oldest first."""
        s = int(s)
        if not 0 <= s < self.n_objects:
            raise IndexError(f"object {s} of {self.n_objects}")
        return self._flat(stat)[self.offsets[s]:self.offsets[s + 1]]

    def _dense_index(self, width: int):
        """(rows, columns) of every entry in a [S, width] layout: right-justified for
        ``align="end"`` (the last column is every object's last entry), else left-justified."""
        nw = np.diff(self.offsets)
        rows = np.repeat(np.arange(self.n_objects, dtype=np.int64), nw)
        cols = np.arange(int(self.offsets[-1]), dtype=np.int64) - np.repeat(self.offsets[:-1], nw)
        if self.align == "end":
            cols += np.repeat(width - nw, nw)
        return rows, cols

    def dense(self, stat: str = "mean") -> np.ndarray:
        """float64 [S, longest object], NaN where an object has no entry: right-justified for
        ``align="end"``, left-justified for ``"start"``."""
        flat = self._flat(stat)
        width = int(np.diff(self.offsets).max()) if self.n_objects else 0
        out = np.full((self.n_objects, width), np.nan, dtype=np.float64)
        rows, cols = self._dense_index(width)
        out[rows, cols] = flat
        return out


class FleetRollup(_FlatPerObject):
    """One resource of a fleet with the time axis coarsened: every object's series cut into
    windows of ``window`` slots, and per window the count, min, max and sum of its present samples
    (one krr_segmented_rollup pass; include/krr_amd.h has the rules).  ``align="end"``: the windows
    end at each series' last slot and the FIRST may be partial — fleets end "now", so windows of
    series of different length line up in wall-clock time; ``"start"``: they start at slot 0 and
    the LAST may be partial.

    Object s owns windows ``offsets[s] .. offsets[s+1]`` of the flat per-window arrays (``offsets``
    int64 [S + 1], ``n_windows`` [S], ``slots`` [S] the series' lengths, all host).  The per-window
    arrays live in HBM; ``wcount``, ``min``, ``max``, ``sum`` and ``mean`` (sum / wcount computed
    there, NaN where wcount == 0) copy them to the host on first use.  A window without a present
    sample has wcount 0, min = max = NaN, sum 0.  ``count`` and ``flags`` ([S], host) are
    ``FleetBatch.stats``' for the whole series.

    Two rollups of adjacent time slices cannot be merged: a window that straddles the cut would
    need both sides' partial windows, which the window grid of either side does not keep.  There
    is no ``concat``; roll up the joined series instead."""
    _STATS = _ROLLUP_STATS
    _COUNT = "wcount"

    def __init__(self, resource, window: int, align: str, offsets, slots, count, flags, wcount, wmin, wmax, wsum,
                 device: int = 0, engine: Optional[SimpleEngine] = None):
        import torch

        self.resource = ResourceType(resource)
        self.window = int(window)
        self.align = str(align)
        if self.align not in _ROLLUP_ALIGN:
            raise ValueError(f"unknown align {align!r}; expected 'start' or 'end'")
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.slots = np.asarray(slots, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int64)
        self.flags = np.asarray(flags).astype(np.uint32)
        self.device = int(device)
        self._engine = engine
        self._t = {"wcount": torch.as_tensor(wcount), "min": torch.as_tensor(wmin), "max": torch.as_tensor(wmax),
                   "sum": torch.as_tensor(wsum)}
        n = int(self.offsets[-1]) if self.offsets.size else 0
        if self.offsets.size != self.slots.size + 1 or any(t.numel() != n for t in self._t.values()):
            raise ValueError("offsets, slots and the per-window arrays do not describe the same windows")
        self._host: dict = {}
        self._batches: dict = {}

    @property
    def n_windows(self) -> np.ndarray:
        return np.diff(self.offsets)

    wcount = property(lambda self: self._flat("wcount"), doc="present samples per window (int32, flat, host)")
    min = property(lambda self: self._flat("min"), doc="float64, flat, host")
    max = property(lambda self: self._flat("max"), doc="float64, flat, host")
    sum = property(lambda self: self._flat("sum"), doc="float64, flat, host")
    mean = property(lambda self: self._flat("mean"), doc="sum / wcount, NaN where wcount == 0 (float64, flat, host)")

    def as_batch(self, stat: str = "mean") -> "FleetBatch":
        """A FleetBatch whose series of this resource is the per-window ``stat`` (``min``, ``max``,
        ``sum`` or ``mean``), in HBM as it is: a gapped series over the window offsets, a window
        without a present sample being an absent slot.  ``stats``, ``moments``, ``exceedance``,
        ``percentiles`` and a further ``rollup`` apply to it.  Raises ValueError if an object is
        flagged KRR_FLAG_NAN: its NaN windows would read as absent and the NaN be dropped."""
        import torch

        stat = self._stat(stat, _ROLLUP_SERIES_STATS)
        if (self.flags & _native.KRR_FLAG_NAN).any():
            s = int(np.flatnonzero(self.flags & _native.KRR_FLAG_NAN)[0])
            raise ValueError(f"object {s} holds a NaN sample (KRR_FLAG_NAN): as a gapped series its NaN windows "
                             f"would be dropped silently")
        batch = self._batches.get(stat)
        if batch is None:
            vals = self.tensor(stat)
            if stat == "sum":
                vals = torch.where(self._t["wcount"] > 0, vals, torch.full_like(vals, float("nan")))
            longest = int(self.n_windows.max()) if self.n_objects else 0
            if vals.is_cuda:
                ps = PackedSeries(vals.contiguous(), torch.from_numpy(self.offsets).to(vals.device), longest, True)
            else:
                ps = PackedSeries(vals.numpy(), self.offsets, longest, True)
            batch = self._batches[stat] = FleetBatch._of({self.resource: ps}, self.n_objects, self.device,
                                                         self._engine)
        return batch

    def peak(self, stat: str = "mean") -> np.ndarray:
        """float64 [S]: the largest window value of every object — with ``mean`` the highest
        ``window``-slot average on this window grid (a burst that straddles a grid boundary is
        split over two windows: ``FleetBatch.sustained_peak`` looks at every alignment); NaN
        without a present sample."""
        return self.as_batch(stat).stats(self.resource).max

    def fold(self, period: int) -> FleetProfile:
        """The windows whose position is congruent mod ``period`` combined, per object: column
        ``period - 1`` holds each series' last window for ``align="end"``, column 0 its first for
        ``"start"``.  With ``window=60`` on a 1-minute step and ``period=24`` this is the
        hour-of-day profile.  Computed where the per-window tensors live; sums add in one fixed
        order (oldest window first)."""
        import torch

        if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or period < 1:
            raise ValueError(f"period must be an int >= 1, got {period!r}")
        period, S = int(period), self.n_objects
        nwmax = int(self.n_windows.max()) if S else 0
        reps = max(-(-nwmax // period), 1)
        width = reps * period
        rows, cols = self._dense_index(width)
        wc = self._t["wcount"]
        idx = torch.from_numpy(rows * width + cols).to(wc.device)
        inf = float("inf")

        def grid(src, fill):
            g = torch.full((S * width,), fill, dtype=src.dtype, device=wc.device)
            g[idx] = src
            return g.view(S, reps, period)

        absent = wc <= 0
        bad = grid((~absent & torch.isnan(self._t["sum"])).to(torch.int32), 0).sum(dim=1) > 0
        count = grid(wc.to(torch.int64), 0).sum(dim=1)
        nan = torch.full((S, period), float("nan"), dtype=torch.float64, device=wc.device)
        mn = grid(torch.where(absent, torch.full_like(self._t["min"], inf), self._t["min"]), inf).amin(dim=1)
        mx = grid(torch.where(absent, torch.full_like(self._t["max"], -inf), self._t["max"]), -inf).amax(dim=1)
        sm = grid(self._t["sum"], 0.0)
        total = sm[:, 0, :].clone()
        for r in range(1, reps):
            total += sm[:, r, :]
        none = count == 0
        mn = torch.where(none | bad, nan, mn)
        mx = torch.where(none | bad, nan, mx)
        total = torch.where(bad, nan, total)
        return FleetProfile(count.cpu().numpy(), mn.cpu().numpy(), mx.cpu().numpy(), total.cpu().numpy())


_SLIDE_SERIES_STATS = ("mean", "sum", "max", "min")
_SLIDE_STATS = _SLIDE_SERIES_STATS + ("wcount",)


class FleetSliding(_FlatPerObject):
    """One resource of a fleet under a moving window: for every slot of every object's series the
    ``window`` slots that END there, with the mean, sum, max and min of their present samples and
    their count (one krr_segmented_slide pass; include/krr_amd.h has the rules).  A window with
    fewer than ``min_count`` present slots is NaN in the four float stats: as a value of a gapped
    series that is an absent slot, so every one of them is a series again.

    The per-slot arrays are laid out by the series' own ``offsets`` (int64 [S + 1]; ``slots`` [S]
    the series' lengths, both host) and live in HBM; only the ones named in ``FleetBatch.sliding``'s
    ``stats=`` exist, and asking for another raises ValueError.  ``peak`` (float64 [S]) is every
    object's largest window mean — the sustained peak, the highest load held for ``window``
    consecutive slots wherever they lie, where a rollup's grid splits a burst that straddles one of
    its boundaries — and ``peak_slot`` (int64 [S]) the first slot it ends at, -1 without a window;
    both are always present.  An object with a NaN sample (KRR_FLAG_NAN) has a NaN peak, with the
    first slot whose window holds the NaN.  ``count`` and ``flags`` ([S], host) are
    ``FleetBatch.stats``' for the whole series.  ``dense`` is right-justified: fleets end "now".

    Two slides of adjacent time slices cannot be merged: a window across the cut needs the older
    slice's last ``window - 1`` samples, which neither result keeps.  There is no ``concat``; slide
    the joined series instead."""
    _STATS = _SLIDE_STATS
    _COUNT = "wcount"
    align = "end"

    def __init__(self, resource, window: int, min_count: int, offsets, count, flags, peak, peak_slot, tensors,
                 device: int = 0, engine: Optional[SimpleEngine] = None):
        import torch

        self.resource = ResourceType(resource)
        self.window = int(window)
        self.min_count = int(min_count)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.slots = np.diff(self.offsets)
        self.count = np.asarray(count, dtype=np.int64)
        self.flags = np.asarray(flags).astype(np.uint32)
        self.peak = np.asarray(peak, dtype=np.float64)
        self.peak_slot = np.asarray(peak_slot, dtype=np.int64)
        self.device = int(device)
        self._engine = engine
        self._t = {self._stat(k): torch.as_tensor(t) for k, t in dict(tensors).items()}
        n = int(self.offsets[-1]) if self.offsets.size else 0
        if self.peak.size != self.slots.size or any(t.numel() != n for t in self._t.values()):
            raise ValueError("offsets, peak and the per-slot arrays do not describe the same slots")
        self._host: dict = {}
        self._batches: dict = {}

    @property
    def stats(self) -> tuple:
        """The per-slot stats this result holds."""
        return tuple(k for k in _SLIDE_STATS if k in self._t)

    def tensor(self, stat: str):
        """The flat per-slot tensor of ``stat`` where the kernel left it (HBM): ``wcount`` int32,
        the others float64.  ValueError if the stat was not asked for in ``stats=``."""
        stat = self._stat(stat)
        t = self._t.get(stat)
        if t is None:
            raise ValueError(f"stat {stat!r} was not computed: name it in sliding(..., stats=...) "
                             f"(this result holds {list(self.stats)})")
        return t

    def as_batch(self, stat: str = "mean") -> "FleetBatch":
        """A FleetBatch whose series of this resource is the per-slot ``stat`` (``mean``, ``sum``,
        ``max`` or ``min``), in HBM as it is: a gapped series over the same offsets, a window with
        fewer than ``min_count`` present slots being an absent slot.  ``percentile``, ``stats``,
        ``exceedance`` and ``rollup`` apply to it.  Raises ValueError if an object is flagged
        KRR_FLAG_NAN: its NaN windows would read as absent and the NaN be dropped."""
        import torch

        stat = self._stat(stat, _SLIDE_SERIES_STATS)
        vals = self.tensor(stat)
        if (self.flags & _native.KRR_FLAG_NAN).any():
            s = int(np.flatnonzero(self.flags & _native.KRR_FLAG_NAN)[0])
            raise ValueError(f"object {s} holds a NaN sample (KRR_FLAG_NAN): as a gapped series its NaN windows "
                             f"would be dropped silently")
        batch = self._batches.get(stat)
        if batch is None:
            longest = int(self.slots.max()) if self.n_objects else 0
            if vals.is_cuda:
                ps = PackedSeries(vals.contiguous(), torch.from_numpy(self.offsets).to(vals.device), longest, True)
            else:
                ps = PackedSeries(vals.numpy(), self.offsets, longest, True)
            batch = self._batches[stat] = FleetBatch._of({self.resource: ps}, self.n_objects, self.device,
                                                         self._engine)
        return batch


_OVERLAY_ALIGN = {"start": _native.KRR_OVERLAY_START, "end": _native.KRR_OVERLAY_END}
_OVERLAY_SERIES_STATS = ("sum", "max", "min", "mean")
_OVERLAY_STATS = ("active",) + _OVERLAY_SERIES_STATS


class FleetOverlay(_FlatPerObject):
    """One resource of a fleet with every object's pods folded slot by slot into ONE series (one
    krr_pods_overlay pass; include/krr_amd.h has the rules): per slot ``active`` (the pods with a
    sample there: the replica count), ``sum`` (the workload's total, ``sum by (workload)``),
    ``max`` / ``min`` (the busiest- / idlest-pod envelope) and ``mean`` (sum / active: the
    per-replica load if the work were spread evenly).  The sum adds the pods in pod order,
    ((0 + x1) + x2) + ..., one fixed order with the same bits on every run.

    The slot axis is the pods' own.  On the dense grid (``pack_dense_grid``, the gapped layouts)
    every pod has the same slots and a slot is a point in wall-clock time.  In the compact layouts
    a slot is a SAMPLE INDEX: ``align="end"`` lines the pods up at their last sample (pods end
    "now"), ``"start"`` at their first, and an object has as many slots as its longest pod — the
    convention ``FleetMoments`` uses for its slot index.

    Object s owns slots ``offsets[s] .. offsets[s+1]`` of the flat per-slot arrays (``offsets``
    int64 [S + 1], ``slots`` [S] the longest pod, ``pods`` [S] the pods per object, all host).  The
    per-slot arrays live in HBM; ``active``, ``sum``, ``max``, ``min`` and ``mean`` copy them to
    the host on first use.  A slot no pod has a sample at has active 0, sum 0 and max = min = mean =
    NaN.  ``count`` ([S]: the samples folded, the sum of active) and ``flags`` ([S]) are
    ``FleetBatch.stats``' for the object's whole series."""
    _STATS = _OVERLAY_STATS
    _COUNT = "active"

    def __init__(self, resource, align: str, offsets, slots, pods, count, flags, active, osum, omax, omin,
                 device: int = 0, engine: Optional[SimpleEngine] = None):
        import torch

        self.resource = ResourceType(resource)
        self.align = str(align)
        if self.align not in _OVERLAY_ALIGN:
            raise ValueError(f"unknown align {align!r}; expected 'start' or 'end'")
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.slots = np.asarray(slots, dtype=np.int64)
        self.pods = np.asarray(pods, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int64)
        self.flags = np.asarray(flags).astype(np.uint32)
        self.device = int(device)
        self._engine = engine
        self._t = {"active": torch.as_tensor(active), "sum": torch.as_tensor(osum), "max": torch.as_tensor(omax),
                   "min": torch.as_tensor(omin)}
        n = int(self.offsets[-1]) if self.offsets.size else 0
        if (self.offsets.size != self.slots.size + 1 or self.pods.size != self.slots.size
                or any(t.numel() != n for t in self._t.values())):
            raise ValueError("offsets, slots, pods and the per-slot arrays do not describe the same slots")
        self._host: dict = {}
        self._batches: dict = {}

    active = property(lambda self: self._flat("active"), doc="pods with a sample per slot (int32, flat, host)")
    sum = property(lambda self: self._flat("sum"), doc="float64, flat, host")
    max = property(lambda self: self._flat("max"), doc="float64, flat, host")
    min = property(lambda self: self._flat("min"), doc="float64, flat, host")
    mean = property(lambda self: self._flat("mean"), doc="sum / active, NaN where active == 0 (float64, flat, host)")

    def as_batch(self, stat: str = "sum") -> "FleetBatch":
        """A FleetBatch whose series of this resource is the per-slot ``stat``, in HBM as it is, one
        segment per object over ``offsets``.  ``sum``, ``max``, ``min`` and ``mean`` give a gapped
        series in which a slot with ``active == 0`` is absent; ``active`` gives a compact float64
        series in which 0 is a value ("no pod up").  ``stats``, ``moments``, ``exceedance``,
        ``percentiles`` and ``rollup`` apply to it.  Raises ValueError if an object is flagged
        KRR_FLAG_NAN: its NaN slots would read as absent and the NaN be dropped."""
        import torch

        stat = self._stat(stat)
        if (self.flags & _native.KRR_FLAG_NAN).any():
            s = int(np.flatnonzero(self.flags & _native.KRR_FLAG_NAN)[0])
            raise ValueError(f"object {s} holds a NaN sample (KRR_FLAG_NAN): as a gapped series its NaN slots "
                             f"would be dropped silently")
        batch = self._batches.get(stat)
        if batch is None:
            vals = self.tensor(stat)
            gapped = stat != "active"
            if stat == "active":
                vals = vals.to(torch.float64)
            elif stat == "sum":
                vals = torch.where(self._t["active"] > 0, vals, torch.full_like(vals, float("nan")))
            longest = int(self.slots.max()) if self.n_objects else 0
            if vals.is_cuda:
                ps = PackedSeries(vals.contiguous(), torch.from_numpy(self.offsets).to(vals.device), longest, gapped)
            else:
                ps = PackedSeries(vals.numpy(), self.offsets, longest, gapped)
            batch = self._batches[stat] = FleetBatch._of({self.resource: ps}, self.n_objects, self.device,
                                                         self._engine)
        return batch

    def peak(self, stat: str = "sum") -> np.ndarray:
        """float64 [S]: the largest slot value of every object — with ``sum`` the workload's peak
        total, with ``active`` the most replicas at once; NaN without a sample."""
        return self.as_batch(stat).stats(self.resource).max


def allocation_thresholds(objects: Sequence, resource: ResourceType, which: str = "requests") -> np.ndarray:
    """float64 [S]: each object's current request (or, ``which="limits"``, limit) of ``resource``
    from ``K8sObjectData.allocations``, as a threshold row for ``FleetBatch.exceedance``.  An
    allocation that is not set (None) or not known ("?") becomes NaN: nothing is above it."""
    if which not in ("requests", "limits"):
        raise ValueError(f"which must be 'requests' or 'limits', got {which!r}")
    resource = ResourceType(resource)
    out = np.full(len(objects), np.nan, dtype=np.float64)
    for i, obj in enumerate(objects):
        v = getattr(obj.allocations, which).get(resource)
        if v is not None and v != "?":
            out[i] = float(v)
    return out


def _check_table_args(length, **others) -> int:
    for name, v in {"length": length, **others}.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int (slots), got {v!r}")
    if length < 1:
        raise ValueError(f"length must be at least 1, got {length!r}")
    return int(length)


def decay_weights(half_life: int, length: int) -> np.ndarray:
    """uint64 [length]: the weight table of an exponential decay with ``half_life`` slots, for
    ``FleetBatch.weighted_percentile``.  Entry a (the age: a slots before a series' last one) is
    floor(2^32 * 2^(-a / half_life)), exactly: entry 0 is 2^32, entry k * half_life is 2^(32 - k),
    the table never increases and is 0 from age 32 * half_life + 1 on.  ``length`` is normally the
    longest series: an older slot takes the table's LAST entry.  With one sample a minute,
    ``decay_weights(1440, 10080)`` is VPA's one-day half-life over a week."""
    length = _check_table_args(length, half_life=half_life)
    h = int(half_life)
    if h < 1:
        raise ValueError(f"half_life must be at least 1 slot, got {half_life!r}")
    # floor(2^(e / h)) with e = 32 h - a = q h + r is floor(G[r] / 2^(32 - q)), G[r] = floor(2^32 * 2^(r / h)).
    # 2^(r / h) is irrational for 0 < r < h, so a float64 estimate (within 2^-18 of 2^32 * 2^(r/h)) gives the
    # floor except next to an integer, where the integers decide: g^h <= 2^(32 h + r) < (g + 1)^h.
    est = np.ldexp(np.exp2(np.arange(h, dtype=np.float64) / h), 32)
    g = np.floor(est).astype(np.uint64)
    for r in np.flatnonzero(np.abs(est - np.rint(est)) < 1e-3)[1:]:  # r = 0 is 2^32 exactly
        c = int(np.rint(est[r]))
        g[r] = c if c**h <= 1 << (32 * h + int(r)) else c - 1
    e = 32 * h - np.arange(length, dtype=np.int64)
    live = e >= 0
    q, r = np.divmod(np.where(live, e, 0), h)
    return np.where(live, g[r] >> (32 - q).astype(np.uint64), np.uint64(0)).astype(np.uint64)


def window_weights(last: int, length: int) -> np.ndarray:
    """uint64 [length]: weight 1 for the newest ``last`` slots (ages 0 .. last - 1) and 0 before
    them: "the percentile of the last day" without re-packing.  An older slot takes the table's
    LAST entry, so ``length`` must exceed ``last`` for it to be 0."""
    length = _check_table_args(length, last=last)
    if not 0 <= last < length:
        raise ValueError(f"last must lie in 0 .. length - 1 = {length - 1}, got {last!r}")
    w = np.zeros(length, dtype=np.uint64)
    w[:int(last)] = 1
    return w


_QNAN_BITS = np.uint64(0x7FF8000000000000)


def _okeys(values: np.ndarray) -> np.ndarray:
    """uint64: the kernels' order-preserving key of every float64's bits (-0.0 below +0.0)."""
    u = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


@dataclass(frozen=True)
class HistogramBins:
    """The data-independent log-linear bins of ``FleetBatch.histogram`` (krr_sketch_params):
    every octave [2^E, 2^(E+1)) from E = ``min_exponent`` up, ``octaves`` of them, is cut into
    2^``mantissa_bits`` equal bins, so a bin's relative width is at most 2^-mantissa_bits.  A row
    has ``width`` = nbins + 4 words: [0] negative, [1] +-0, [2] (0, 2^min_exponent),
    [3 .. 3 + nbins) the log-linear bins, [3 + nbins] everything from 2^(min_exponent + octaves)
    up, +Inf included.  A sample's bin comes from its bits alone, so two histograms with equal
    bins add word for word.  ValueError outside 0 <= mantissa_bits <= 10, octaves >= 1,
    min_exponent >= -1022, min_exponent + octaves <= 1024 and width <= 4096."""
    mantissa_bits: int
    min_exponent: int
    octaves: int

    def __post_init__(self):
        for name in ("mantissa_bits", "min_exponent", "octaves"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an int, got {v!r}")
            object.__setattr__(self, name, int(v))
        m, e, o = self.mantissa_bits, self.min_exponent, self.octaves
        if not 0 <= m <= 10 or o < 1 or e < -1022 or e + o > 1024:
            raise ValueError(f"bins outside 0 <= mantissa_bits <= 10, octaves >= 1, min_exponent >= -1022, "
                             f"min_exponent + octaves <= 1024: {self!r}")
        if self.width > 4096:
            raise ValueError(f"a histogram row holds at most 4096 words, these bins need {self.width}")

    @property
    def nbins(self) -> int:
        return self.octaves << self.mantissa_bits

    @property
    def width(self) -> int:
        return self.nbins + 4

    def params(self) -> _native.KrrSketchParams:
        return _native.KrrSketchParams(self.mantissa_bits, self.min_exponent, self.octaves, 0)

    def edges(self) -> np.ndarray:
        """float64 [nbins + 1], exact: entry i is the lower edge of row word 3 + i,
        2^E (1 + j 2^-m) with E = min_exponent + (i >> m) and j = i & (2^m - 1); the last entry
        is 2^(min_exponent + octaves), where the top word starts (+Inf when that is 2^1024)."""
        base = (self.min_exponent + 1023) << self.mantissa_bits
        u = (np.arange(self.nbins + 1, dtype=np.uint64) + np.uint64(base)) << np.uint64(52 - self.mantissa_bits)
        return u.view(np.float64)

    def bin_of(self, values) -> np.ndarray:
        """int64, the shape of ``values``: the row word every float64 falls into, by the kernels'
        rule on its bits; -1 for a NaN."""
        x = np.asarray(values, dtype=np.float64)
        u = np.ascontiguousarray(x).view(np.uint64).reshape(x.shape)
        mag = u & np.uint64((1 << 63) - 1)
        i = (mag >> np.uint64(52 - self.mantissa_bits)).astype(np.int64) - ((self.min_exponent + 1023)
                                                                              << self.mantissa_bits)
        b = np.where((i >= 0) & (i < self.nbins), 3 + i, np.where(i < 0, 2, 3 + self.nbins))
        b = np.where(u >> np.uint64(63) != 0, 0, b)
        b = np.where(mag == 0, 1, b)
        return np.where(np.isnan(x), -1, b).astype(np.int64)


def default_bins(resource: ResourceType) -> HistogramBins:
    """The bins ``FleetBatch.histogram`` takes when none are given: 16 per octave (a relative bin
    width of at most 6.25%) over 2^-10 .. 2^10 cores for CPU and 2^20 .. 2^40 bytes for memory,
    324 words a row either way.  (Kubernetes VPA's buckets grow by 5% over 0.01 .. 1000 cores and
    10 MB .. 1 TB.)"""
    return HistogramBins(4, -10, 20) if ResourceType(resource) == ResourceType.CPU else HistogramBins(4, 20, 20)


class FleetHistogram:
    """Every object's histogram of weights (``FleetBatch.histogram``): the rows stay in HBM, and
    any number of percentiles is read from them without touching the samples again.

    ``count`` (int64) and ``flags`` (uint32) are krr_segmented_stats'; ``wsum`` (uint64) is a
    row's total weight W and ``total`` = W / 2^32 the effective sample count under
    ``decay_weights``; ``wmin`` / ``wmax`` (float64) are the least and greatest sample of positive
    weight, NaN where W == 0.  All [S], host arrays.

    A percentile's answer is a BIN: the one that holds ``FleetBatch.weighted_percentile``'s exact
    answer for the same table (the rule is the same and a sample's bin never decreases with its
    value).  ``bracket(p)`` is that bin's range clamped to [wmin, wmax], and ``percentile(p)`` its
    upper end, VPA's "end of the bucket": never below the exact weighted percentile and, inside
    the log-linear bins, at most (1 + 2^-mantissa_bits) times it.  Below 2^min_exponent and from
    2^(min_exponent + octaves) up the bracket is as wide as the data (KRR_FLAG_SKETCH_RANGE).

    Rows are integers, so ``merge`` is exact in any order: time slices of the same objects (the
    older one built with ``age_base`` = the slots that follow it) and the shards of other ranks
    add up to the histogram of the whole.  A decayed histogram cannot be AGED after the fact:
    integer weights do not rescale exactly, so a later "now" needs a rebuild or ``age_base``."""

    def __init__(self, resource, bins: HistogramBins, hist, count, flags, wsum, wmin, wmax, device: int, engine):
        self.resource, self.bins = resource, bins
        self._hist = hist
        self.count, self.flags = count, flags
        self.wsum, self.wmin, self.wmax = wsum, wmin, wmax
        self.device, self._engine = device, engine
        self._answers: dict = {}

    @property
    def n_objects(self) -> int:
        return int(self.count.size)

    @property
    def total(self) -> np.ndarray:
        return self.wsum.astype(np.float64) / float(WEIGHT_MAX)

    def tensor(self):
        """The rows in HBM: an int64 tensor [S, bins.width] of uint64 words below 2^63."""
        return self._hist

    def of(self, s: int) -> np.ndarray:
        """uint64 [bins.width]: object s's row on the host."""
        return self._hist[int(s)].cpu().numpy().view(np.uint64)

    def _query(self, percentiles) -> dict:
        fracs = tuple(percentile_fraction(p) for p in percentiles)
        missing = {f: p for f, p in zip(fracs, percentiles) if f not in self._answers}  # asked once each
        if missing:
            r = self._engine.whist_query(self._hist, self.wmin, self.wmax, self.bins.params(), list(missing.values()))
            for j, f in enumerate(missing):
                self._answers[f] = {k: v[j] for k, v in r.items()}
        return {k: np.stack([self._answers[f][k] for f in fracs]) for k in ("bin", "lower", "upper", "flags")}

    def percentiles(self, percentiles: Sequence, return_flags: bool = False):
        """float64 [P, S]: row j is the upper end of the bracket of ``percentiles[j]`` (anything
        ``weighted_percentile`` takes), all read from the rows in one launch per
        KRR_MAX_PERCENTILES of them; NaN where an object has no weight.  ``return_flags``: also
        uint32 [P, S], the object's KRR_FLAG_NAN / KRR_FLAG_EMPTY joined with the answer's
        KRR_FLAG_EMPTY (no weight) and KRR_FLAG_SKETCH_RANGE (a lumped bin)."""
        percentiles = list(percentiles)
        if not percentiles:
            raise ValueError("at least one percentile")
        r = self._query(percentiles)
        return (r["upper"], r["flags"] | self.flags[None, :]) if return_flags else r["upper"]

    def percentile(self, percentile, return_flags: bool = False):
        """float64 [S]: ``percentiles([percentile])[0]``."""
        r = self.percentiles([percentile], return_flags)
        return (r[0][0], r[1][0]) if return_flags else r[0]

    def bracket(self, percentile) -> tuple:
        """(lower, upper), float64 [S] each: the range of the bin that holds the exact weighted
        percentile, clamped to [wmin, wmax]; NaN where an object has no weight."""
        r = self._query([percentile])
        return r["lower"][0], r["upper"][0]

    def answer_bins(self, percentile) -> np.ndarray:
        """int32 [S]: the row word that answers ``percentile``, -1 where an object has no weight."""
        return self._query([percentile])["bin"][0]

    def merge(self, other: "FleetHistogram") -> "FleetHistogram":
        """The histogram of both sets of samples, object by object: the rows and the total
        weights add (exact, any order), the counts add, wmin / wmax are the least / greatest of
        the two in sample order (NaN ignored), KRR_FLAG_EMPTY stays only where both were empty
        and KRR_FLAG_NAN where either had it.  ValueError unless both have the same bins and
        number of objects.  For two time slices of the same objects, build the OLDER one with
        ``age_base`` = the newer one's slots."""
        if not isinstance(other, FleetHistogram) or other.bins != self.bins or other.n_objects != self.n_objects:
            raise ValueError("merge needs a FleetHistogram of the same bins and number of objects")

        def pick(a, b, greatest):
            ka, kb = _okeys(a), _okeys(b)
            take_b = np.isnan(a) | (~np.isnan(b) & ((kb > ka) if greatest else (kb < ka)))
            return np.where(take_b, b, a)

        empty = np.uint32(_native.KRR_FLAG_EMPTY)
        flags = ((self.flags | other.flags) & ~empty) | (self.flags & other.flags & empty)
        return FleetHistogram(self.resource, self.bins, self._hist + other._hist.to(self._hist.device),
                              self.count + other.count, flags.astype(np.uint32), self.wsum + other.wsum,
                              pick(self.wmin, other.wmin, False), pick(self.wmax, other.wmax, True), self.device,
                              self._engine)


def _slots(ps: PackedSeries) -> np.ndarray:
    """int64 [S]: each series' length in slots, from the offsets wherever they live."""
    offs = ps.offsets
    if not isinstance(offs, np.ndarray) and hasattr(offs, "is_cuda"):
        offs = offs.cpu().numpy()
    return np.diff(np.asarray(offs, dtype=np.int64))


class FleetBatch:
    """A fleet's histories as device-side series, with cached per-object statistics.

    Results are cached per (resource, call): asking twice launches once.  Not thread-safe (one
    batch per ``run_batch`` call)."""

    def __init__(self, histories: Optional[Sequence[Mapping]] = None, device: int = 0,
                 engine: Optional[SimpleEngine] = None):
        self._histories = histories if histories is not None else []
        self._series: dict[ResourceType, PackedSeries] = {}
        self._n = len(self._histories)
        self.device = int(device)
        self._engine = engine
        self._cache: dict = {}
        self.pod_groups: Optional[np.ndarray] = None  # per_pod() views: the pods of each object

    @classmethod
    def from_fleet(cls, fleet: PackedFleet, device: int = 0, engine: Optional[SimpleEngine] = None) -> "FleetBatch":
        """Over a PackedFleet from any packer (host arrays, or tensors in HBM from the device
        packer, which then run as they are): no Decimal lists at all."""
        if fleet.cpu.n_segments != fleet.mem.n_segments:
            raise ValueError("cpu and memory need one segment per object each")
        return cls._of({ResourceType.CPU: fleet.cpu, ResourceType.Memory: fleet.mem}, fleet.n_objects, device, engine)

    @classmethod
    def _of(cls, series: dict, n: int, device: int, engine: Optional[SimpleEngine]) -> "FleetBatch":
        batch = cls(None, device, engine)
        batch._histories = None
        batch._series = dict(series)
        batch._n = int(n)
        return batch

    @property
    def n_objects(self) -> int:
        return self._n

    @property
    def engine(self) -> SimpleEngine:
        if self._engine is None:
            self._engine = default_engine(self.device)
        return self._engine

    def series(self, resource: ResourceType) -> PackedSeries:
        """The resource's PackedSeries, packed on first use (pack_resource) and kept."""
        resource = ResourceType(resource)
        ps = self._series.get(resource)
        if ps is None:
            if self._histories is None:
                raise KeyError(f"this batch holds no {resource.value} series")
            ps = self._series[resource] = pack_resource(self._histories, resource)
        return ps

    # --- statistics --------------------------------------------------------------------
    def stats(self, resource: ResourceType) -> FleetStats:
        key = (ResourceType(resource), "stats")
        st = self._cache.get(key)
        if st is None:
            r = self.engine.stats_series(self.series(resource))
            st = self._cache[key] = FleetStats(r["count"], r["min"], r["max"], r["sum"], r["flags"])
        return st

    def moments(self, resource: ResourceType, trend: bool = True) -> FleetMoments:
        """Mean, variance and (with ``trend``) the least-squares line over the slot index of
        every object's series: one krr_segmented_moments pass, cached per resource.  A cached
        result with the trend also serves ``trend=False``; the launch without it skips the
        trend's arithmetic and gives the same mean and m2."""
        resource = ResourceType(resource)
        mo = self._cache.get((resource, "moments", True))
        if mo is None and not trend:
            mo = self._cache.get((resource, "moments", False))
        if mo is None:
            ps = self.series(resource)
            r = self.engine.moments_series(ps, trend=bool(trend))
            mo = self._cache[(resource, "moments", bool(trend))] = FleetMoments(
                r["count"], r["mean"], r["m2"], r.get("tmean"), r.get("t2"), r.get("cxt"), r["flags"], _slots(ps))
        return mo

    def _threshold_rows(self, thresholds, S: int) -> np.ndarray:
        """``exceedance``'s thresholds as contiguous float64 [R, S]."""
        if isinstance(thresholds, np.ndarray) and thresholds.dtype != object:
            thr = thresholds.astype(np.float64, copy=False)
        else:
            seq = list(thresholds)
            if any(isinstance(t, (list, tuple, np.ndarray)) for t in seq):
                raise ValueError("thresholds given as a sequence hold one scalar per object (Decimal, float or None); "
                                 "several thresholds per object go in a float64 array [R, S]")
            thr = np.array([np.nan if t is None else float(t) for t in seq], dtype=np.float64)
        if thr.ndim == 1:
            thr = thr[None, :]
        if thr.ndim != 2 or thr.shape[0] < 1 or thr.shape[1] != S:
            raise ValueError(f"thresholds must have shape [{S}] or [R, {S}] with R >= 1 (one column per object), "
                             f"got {thr.shape}")
        return np.ascontiguousarray(thr)

    def exceedance(self, resource: ResourceType, thresholds) -> FleetExceedance:
        """How every object's series lies above its thresholds: samples above, their summed
        excess, the longest run and the runs at both ends (FleetExceedance), from one
        krr_segmented_exceed pass per four thresholds.  ``thresholds`` is float64 [S] (one per
        object), float64 [R, S] (R per object; the result's rows), or a sequence with one
        ``Decimal | float | None`` per object, where None and Decimal('NaN') become NaN: "no
        request set", nothing is above it.  ``allocation_thresholds(objects, resource)`` builds
        the row of current requests or limits.  Cached per (resource, threshold bytes).

        On a ``per_pod()`` view the objects are pods; per-object thresholds go to the pods with

            pods = batch.per_pod(ResourceType.CPU)
            ex = pods.exceedance(ResourceType.CPU, np.repeat(thr, np.diff(pods.pod_groups)))
        """
        resource = ResourceType(resource)
        ps = self.series(resource)
        thr = self._threshold_rows(thresholds, ps.n_segments)
        key = (resource, "exceedance", thr.shape[0], thr.tobytes())
        ex = self._cache.get(key)
        if ex is None:
            r = self.engine.exceed_series(ps, thr)
            ex = self._cache[key] = FleetExceedance(r["above"], r["excess"], r["longest"], r["head"], r["tail"],
                                                    r["last"], thr, r["count"], r["flags"], _slots(ps))
        return ex

    def rollup(self, resource: ResourceType, window: int, align: str = "end") -> FleetRollup:
        """Every object's series cut into windows of ``window`` slots, with count, min, max and sum
        per window (FleetRollup): one krr_segmented_rollup pass, cached per (resource, window,
        align).  ``align="end"`` (the default) ends the windows at each series' last slot;
        ``"start"`` starts them at its first.  The result's ``as_batch(stat)`` is a FleetBatch
        again, so a percentile of smoothed usage is

            batch.rollup(ResourceType.CPU, 5).as_batch("mean").percentile(ResourceType.CPU, "95", mode="linear")

        and ``peak()`` the highest window mean.  Works on a ``per_pod()`` view unchanged (windows
        per pod)."""
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= 2**31 - 1:
            raise ValueError(f"window must be an int in 1 .. 2^31-1 (slots), got {window!r}")
        if align not in _ROLLUP_ALIGN:
            raise ValueError(f"unknown align {align!r}; expected 'start' or 'end'")
        resource = ResourceType(resource)
        key = (resource, "rollup", int(window), align)
        ru = self._cache.get(key)
        if ru is None:
            ps = self.series(resource)
            r = self.engine.rollup_series(ps, int(window), _ROLLUP_ALIGN[align])
            if (r["flags"] & _native.KRR_FLAG_CAPACITY).any():
                s = int(np.flatnonzero(r["flags"] & _native.KRR_FLAG_CAPACITY)[0])
                raise RuntimeError(f"object {s}: window offsets too small for its windows (KRR_FLAG_CAPACITY)")
            ru = self._cache[key] = FleetRollup(resource, int(window), align, r["offsets"], _slots(ps), r["count"],
                                                r["flags"], r["wcount"], r["min"], r["max"], r["sum"],
                                                self.device, self.engine)
        return ru

    @staticmethod
    def _slide_args(window, min_count) -> tuple:
        cap = _native.KRR_SLIDE_MAX_WINDOW
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
            raise ValueError(f"window must be an int in 1 .. {cap} (slots), got {window!r}")
        if window > cap:
            raise ValueError(f"window {window} is above the sliding cap of {cap} slots (KRR_SLIDE_MAX_WINDOW: the "
                             f"kernel keeps a window in LDS); for coarse windows cut the series with rollup() first "
                             f"and slide over rollup(...).as_batch('mean')")
        if min_count is None:
            min_count = window
        if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or not 1 <= min_count <= window:
            raise ValueError(f"min_count must be an int in 1 .. window ({window}) or None, got {min_count!r}")
        return int(window), int(min_count)

    def sliding(self, resource: ResourceType, window: int, min_count: Optional[int] = None,
                stats: Sequence[str] = ("mean",)) -> FleetSliding:
        """The moving window over every object's series (FleetSliding): for every slot the
        ``window`` slots that end there, one krr_segmented_slide pass, cached per (resource,
        window, min_count, stats).  ``stats`` is a subset of ``mean``, ``sum``, ``max``, ``min``,
        ``wcount``: each is an array as large as the series, and only those named are allocated
        and written.  A window is emitted when at least ``min_count`` of its slots are present
        and is NaN (an absent slot) otherwise; ``min_count=None`` means ``window``: full windows
        only, as pandas' ``rolling`` does.  A gapped series (scrape failures, pods that came
        late) usually wants less, or most of its windows are absent: ``min_count=window // 2 + 1``
        asks for a majority.  The result's ``as_batch(stat)`` is a FleetBatch again:

            batch.sliding(ResourceType.CPU, 5).as_batch("mean").percentile(ResourceType.CPU, "95", mode="linear")

        ``window`` is at most ``KRR_SLIDE_MAX_WINDOW`` slots (a day at 1 minute fits); for coarser
        windows use ``rollup`` first.  Cost: the window lives in LDS, so long windows run few waves
        per CU — measured against ``stats`` on the same series, the mean costs 3-4.5x at 5 and 60
        slots but about 10x at 1,440, and all five stats 6-11x and about 31x (k_slide);
        for a day-long window ``rollup(resource, 60)`` first and a 24-slot slide over the hourly
        means reads a sixtieth.  Works on a ``per_pod()`` view unchanged (windows per pod).
        Slides of adjacent time slices cannot be merged (FleetSliding says why)."""
        window, min_count = self._slide_args(window, min_count)
        if isinstance(stats, str):
            stats = (stats,)
        want = tuple(k for k in _SLIDE_STATS if k in set(stats))
        if len(want) != len(set(stats)):
            raise ValueError(f"unknown stat in stats={list(stats)!r}; expected a subset of {list(_SLIDE_STATS)}")
        resource = ResourceType(resource)
        key = (resource, "sliding", window, min_count, want)
        sl = self._cache.get(key)
        if sl is None:
            r = self.engine.sliding_series(self.series(resource), window, min_count, want)
            sl = self._cache[key] = FleetSliding(resource, window, min_count, r["offsets"], r["count"], r["flags"],
                                                 r["peak"], r["peak_slot"], {k: r[k] for k in want}, self.device,
                                                 self.engine)
        return sl

    def sustained_peak(self, resource: ResourceType, window: int, min_count: Optional[int] = None,
                       return_slot: bool = False):
        """float64 [S]: the highest mean every object held over ANY ``window`` consecutive slots
        (NaN without an emitted window, or with a NaN sample) — the launch of ``sliding`` with no
        per-slot output, so it costs one read of the series.  ``return_slot``: also int64 [S],
        the first slot such a window ends at (-1 without one).  ``min_count`` as ``sliding``."""
        sl = self.sliding(resource, window, min_count, stats=())
        return (sl.peak, sl.peak_slot) if return_slot else sl.peak

    def overlay(self, resource: ResourceType, align: str = "end") -> FleetOverlay:
        """Every object's pods folded slot by slot into one series (FleetOverlay): per slot the
        pods with a sample (``active``), their ``sum``, ``max`` and ``min``; one krr_pods_overlay
        pass, cached per (resource, align).  ``align="end"`` (the default) lines an object's pods
        up at their last slot, ``"start"`` at their first; on the dense grid, where every pod has
        the same slots, both are wall-clock time.  The result's ``as_batch(stat)`` is a FleetBatch
        again, so the p95 of a workload's total over hourly means is

            ov = batch.overlay(ResourceType.CPU)
            ov.as_batch("sum").rollup(ResourceType.CPU, 60).as_batch("mean").percentile(ResourceType.CPU, "95")

        Needs the series' pod boundaries (``per_pod`` says which series carry them): on a
        ``per_pod()`` view, whose series has none, it raises the same ValueError."""
        if align not in _OVERLAY_ALIGN:
            raise ValueError(f"unknown align {align!r}; expected 'start' or 'end'")
        resource = ResourceType(resource)
        key = (resource, "overlay", align)
        ov = self._cache.get(key)
        if ov is None:
            r = self.engine.overlay_series(self.series(resource), _OVERLAY_ALIGN[align])
            if (r["flags"] & _native.KRR_FLAG_CAPACITY).any():
                s = int(np.flatnonzero(r["flags"] & _native.KRR_FLAG_CAPACITY)[0])
                raise RuntimeError(f"object {s}: slot offsets too small for its slots (KRR_FLAG_CAPACITY)")
            ov = self._cache[key] = FleetOverlay(resource, align, r["offsets"], r["slots"], r["pods"], r["count"],
                                                 r["flags"], r["active"], r["sum"], r["max"], r["min"],
                                                 self.device, self.engine)
        return ov

    def _wquantile(self, resource: ResourceType, percentile, weights) -> dict:
        """``SimpleEngine.wquantile_series`` of the resource, cached per (resource, percentile as
        a fraction, weight bytes)."""
        resource = ResourceType(resource)
        tab = weight_table(weights)
        frac = percentile_fraction(percentile)
        key = (resource, "wquantile", frac, tab.tobytes())
        r = self._cache.get(key)
        if r is None:
            r = self._cache[key] = self.engine.wquantile_series(self.series(resource), tab, percentile)
        return r

    def weighted_percentile(self, resource: ResourceType, percentile, weights, return_flags: bool = False):
        """float64 [S]: the exact WEIGHTED percentile of every object's series, a sample's weight
        given by its age (krr_segmented_wquantile).  ``weights`` is a uint64 table indexed by age:
        entry 0 weighs a series' last slot ("now"), entry a the slot a places before it, and the
        table's last entry everything older (``decay_weights``, ``window_weights``, or any
        integers within 0 .. 2^32).  With W the summed weight of an object's present samples and
        C(v) that of its samples <= v, the answer is the smallest sample v with C(v) >= W * p / 100,
        compared exactly: the weighted "inverted CDF" quantile, with unit weights
        sorted(x)[ceil(n p / 100) - 1] — NOT the index rule of ``percentile(mode="sorted_lower")``.
        ``percentile`` is anything ``Decimal(str(.))`` takes in (0, 100]; it becomes an exact
        fraction, whose denominator may not exceed 10^15.  ValueError for a table that is empty,
        not 1-D, of a float dtype, negative or above 2^32.  NaN where an object has no weight at
        all (no sample, or only zero-weight ones) and where a flag says so (KRR_FLAG_EMPTY,
        KRR_FLAG_NAN); ``return_flags``: also the uint32 [S] flags, for ``to_decimal``.  Cached
        per (resource, percentile, weight bytes).  Works on a ``per_pod()`` view unchanged
        (weights per pod).  On series packed without gaps (HistoryData lists) age counts SAMPLES,
        not minutes: a series that ended early is not shifted, as for ``overlay(align="end")``."""
        r = self._wquantile(resource, percentile, weights)
        value = np.where((r["wsum"] == 0) | (r["flags"] != 0), np.nan, r["value"])
        return (value, r["flags"]) if return_flags else value

    def weight_sums(self, resource: ResourceType, weights) -> np.ndarray:
        """float64 [S]: every object's total weight / 2^32 under ``weights``: with
        ``decay_weights`` the effective sample count behind ``weighted_percentile``.  Taken from
        a cached ``weighted_percentile`` of the same table when there is one (the total does not
        depend on the percentile), else one launch at p = 100."""
        resource = ResourceType(resource)
        tab = weight_table(weights).tobytes()
        hit = next((v for k, v in self._cache.items()
                    if len(k) == 4 and k[:2] == (resource, "wquantile") and k[3] == tab), None)
        r = hit if hit is not None else self._wquantile(resource, 100, weights)
        return r["wsum"].astype(np.float64) / float(WEIGHT_MAX)

    def histogram(self, resource: ResourceType, weights=None, bins: Optional[HistogramBins] = None,
                  age_base=0) -> FleetHistogram:
        """Every object's histogram of weights over data-independent log-linear bins, from ONE
        pass over the values (krr_segmented_whist): the form of the recency-weighted distribution
        that gives any number of percentiles without another pass and that merges exactly, at the
        price of a value error of one bin.  ``weights`` is an age-indexed table as
        ``weighted_percentile`` takes it (None: the unit table, a plain histogram); ``bins`` a
        ``HistogramBins`` (None: ``default_bins(resource)``); ``age_base`` an int or an int64
        array [S], not negative: the slots that FOLLOW each object's series when this batch holds
        an older slice of it, so that the slice's ``FleetHistogram`` merges with the newer one's
        into the histogram of the whole.  Cached per (resource, bins, weight bytes, age_base
        bytes).  Works on a ``per_pod()`` view unchanged (a row per pod).  On series packed
        without gaps age counts SAMPLES, as for ``weighted_percentile``."""
        resource = ResourceType(resource)
        bins = default_bins(resource) if bins is None else bins
        if not isinstance(bins, HistogramBins):
            raise ValueError(f"bins must be a HistogramBins, got {bins!r}")
        tab = weight_table(np.array([1], dtype=np.uint64) if weights is None else weights)
        ps = self.series(resource)
        if isinstance(age_base, bool) or (np.ndim(age_base) == 0 and not isinstance(age_base, (int, np.integer))):
            raise ValueError(f"age_base must be an int or an int64 array, got {age_base!r}")
        base = np.asarray(age_base)
        if not np.issubdtype(base.dtype, np.integer) or (base < 0).any() or base.shape not in ((), (ps.n_segments,)):
            raise ValueError(f"age_base must be a non-negative int or an int64 array [{ps.n_segments}]")
        base = np.ascontiguousarray(np.broadcast_to(base.astype(np.int64), (ps.n_segments,)))
        key = (resource, "histogram", bins, tab.tobytes(), base.tobytes())
        h = self._cache.get(key)
        if h is None:
            r = self.engine.whist_series(ps, tab, bins.params(), base if base.any() else None)
            h = self._cache[key] = FleetHistogram(resource, bins, r["hist"], r["count"], r["flags"], r["wsum"],
                                                  r["wmin"], r["wmax"], self.device, self.engine)
        return h

    def percentiles(self, resource: ResourceType, percentiles: Sequence, mode: str = "ref_index",
                    return_flags: bool = False):
        """float64 [P, S]: row j is percentile ``percentiles[j]`` (anything ``cpu_percentile``
        accepts: int, str, Decimal; 0 < p <= 100) of every object's series under ``mode``
        ("ref_index": the sample at index int((n-1)·p/100) of the unsorted series; "sorted_lower":
        sorted(x)[that index]; "linear": np.percentile).  No sample: NaN.  A NaN sample
        (KRR_FLAG_NAN): NaN here, and ``to_decimal`` applies the reference's rule.
        KRR_FLAG_CAPACITY raises RuntimeError.  ``return_flags``: also the uint32 [P, S] flags."""
        if mode not in MODE_CODES:
            raise ValueError(f"unknown percentile mode {mode!r}; expected one of {sorted(MODE_CODES)}")
        resource = ResourceType(resource)
        ps = [Decimal(str(p)) for p in percentiles]
        keys = [(resource, "percentile", mode, p) for p in ps]
        todo = [p for p, k in dict(zip(ps, keys)).items() if k not in self._cache]
        if todo:
            value, count, flags = self.engine.percentiles_series(self.series(resource),
                                                                 [percentile_params(p, mode) for p in todo])
            if (flags & _native.KRR_FLAG_CAPACITY).any():
                j, s = np.argwhere(flags & _native.KRR_FLAG_CAPACITY)[0]
                raise RuntimeError(f"object {s}: selection bound violated for percentile {todo[j]} (KRR_FLAG_CAPACITY)")
            value = np.where(flags & _native.KRR_FLAG_NAN, np.nan, value)
            for j, p in enumerate(todo):
                self._cache[(resource, "percentile", mode, p)] = (value[j], flags[j], count)
        rows = [self._cache[k] for k in keys]
        S = self.series(resource).n_segments
        value = np.stack([r[0] for r in rows]) if rows else np.zeros((0, S))
        if return_flags:
            return value, (np.stack([r[1] for r in rows]) if rows else np.zeros((0, S), dtype=np.uint32))
        return value

    def percentile(self, resource: ResourceType, percentile, mode: str = "ref_index", return_flags: bool = False):
        """One percentile: float64 [S] (and, with ``return_flags``, uint32 [S])."""
        out = self.percentiles(resource, [percentile], mode, return_flags)
        return (out[0][0], out[1][0]) if return_flags else out[0]

    def counts(self, resource: ResourceType, percentile, mode: str = "ref_index") -> np.ndarray:
        """The present samples behind a percentile already asked for (int64 [S])."""
        self.percentiles(resource, [percentile], mode)
        return self._cache[(ResourceType(resource), "percentile", mode, Decimal(str(percentile)))][2]

    # --- pods --------------------------------------------------------------------------
    def per_pod(self, resource: ResourceType) -> "FleetBatch":
        """A FleetBatch whose objects are the PODS of this one's, for that resource alone;
        its ``pod_groups`` (int64 [S + 1], host) says which pods object s owns:
        pod_groups[s] .. pod_groups[s + 1].  Raises ValueError for a series without pod
        boundaries: ``FleetBatch(histories)`` (pack_resource) attaches them to the CPU series
        only; the packers of response bodies keep them for every series they pack."""
        resource = ResourceType(resource)
        key = (resource, "per_pod")
        pods = self._cache.get(key)
        if pods is None:
            ps = self.series(resource)
            if ps.pod_offsets is None or ps.pod_groups is None:
                pod_view(ps)  # raises the ValueError that names the packers
            groups = ps.pod_groups
            if isinstance(groups, np.ndarray) or not hasattr(groups, "is_cuda"):
                view = pod_view(ps)
                groups = np.asarray(groups, dtype=np.int64)
            else:  # a series in HBM (device packer): its tensors go to the kernels as they are
                po = ps.pod_offsets.contiguous()
                longest = ps.pod_max_len
                if longest is None:
                    longest = int((po[1:] - po[:-1]).max()) if po.numel() > 1 else 0
                view = PackedSeries(ps.values, po, int(longest), ps.gaps_are_nan)
                groups = groups.cpu().numpy().astype(np.int64)
            pods = self._cache[key] = FleetBatch._of({resource: view}, view.n_segments, self.device, self._engine)
            pods.pod_groups = groups
        return pods

    # --- Decimals ----------------------------------------------------------------------
    def exact_mask(self, resource: ResourceType) -> Optional[np.ndarray]:
        """bool [S]: the objects whose Decimals are not Prometheus' own strings, so that
        ``to_decimal`` cannot give back the caller's sample object; None when there is none
        (always None for fleets packed from response bodies)."""
        exact = self.series(resource).exact
        return None if exact is None else np.asarray(exact) > 0

    @staticmethod
    def to_decimal(values, flags=None, counts=None, mode: Optional[str] = None) -> list:
        """list[Decimal] of a float64 array: ``prom_decimal(float)``, the float's shortest
        string.  With ``flags``, ``SimpleStrategySettings.cpu_from_raw``'s rule: KRR_FLAG_CAPACITY
        raises RuntimeError, KRR_FLAG_EMPTY gives Decimal('NaN'), and KRR_FLAG_NAN gives
        Decimal('NaN') — or, as the reference's sorted() / max() over Decimals would, raises
        decimal.InvalidOperation when ``mode`` is "sorted_lower" and ``counts`` shows two or more
        samples."""
        values = np.asarray(values, dtype=np.float64)
        if flags is None:
            return [prom_decimal(float(v)) for v in values]
        flags = np.asarray(flags).astype(np.uint32)
        out = []
        for i, (v, f) in enumerate(zip(values.tolist(), flags.tolist())):
            if f & _native.KRR_FLAG_CAPACITY:
                raise RuntimeError(f"object {i}: selection bound violated (KRR_FLAG_CAPACITY)")
            if f & _native.KRR_FLAG_EMPTY:
                out.append(Decimal("NaN"))
            elif f & _native.KRR_FLAG_NAN:
                if mode == "sorted_lower" and counts is not None and int(counts[i]) >= 2:
                    raise decimal.InvalidOperation([decimal.InvalidOperation])
                out.append(Decimal("NaN"))
            else:
                out.append(prom_decimal(v))
        return out

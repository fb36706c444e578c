"""A custom strategy on the GPU path: size CPU from the load a pod actually HELD.

    CPU request    = per pod, the 95th percentile (numpy's linear rule) of its 5-slot sliding
                     means; the object gets the max over its pods
    CPU limit      = per pod, the sustained 5-slot peak: the highest mean of ANY 5 consecutive
                     slots; the max over the pods
    memory request = max(samples) x (1 + memory_buffer_percentage / 100), also the limit

On a one-minute scrape step a window of 5 slots is five minutes.  ``smoothed_strategy`` cuts every
series into windows on one fixed grid, which splits a burst that straddles a grid boundary over
two windows and can report a 5-slot burst at 3/5 of its height; here a window ends at EVERY slot
(``FleetBatch.sliding``, one krr_segmented_slide pass), so "the highest 5-minute mean" is that.
The sliding means stay in HBM as a series of their own, whose percentile is the call every
FleetBatch has; the limit comes from the same launch, and costs nothing per slot when asked for
alone (``FleetBatch.sustained_peak``).  The windows are per POD: a window over the object's
concatenated samples would run across the boundary between two pods.  Only full windows count
(``min_count=None``): a pod with fewer samples than the window has none, and an object without a
full window gets NaN (the runner prints "?").  One Decimal multiplication per object stays on the
host.  ``run()`` is the same code over a fleet of one.

    from examples.burst_strategy import BurstStrategy, BurstSettings
    strategy = BurstStrategy(BurstSettings(window_slots=5))
    results = BatchedRunner(strategy).recommend(objects, histories)
"""
from __future__ import annotations

import decimal
from decimal import Decimal
from typing import Optional, Sequence

import numpy as np
import pydantic.v1 as pd

from krr_amd import _native
from krr_amd.api import FleetBatch
from krr_amd.core.abstract.strategies import (
    BaseStrategy,
    HistoryData,
    K8sObjectData,
    ResourceRecommendation,
    ResourceType,
    RunResult,
    StrategySettings,
)
from krr_amd.core.rounding import reference_context


def max_over_pods(per_pod: np.ndarray, pod_groups: np.ndarray) -> np.ndarray:
    """float64 [S]: the largest non-NaN value among each object's pods, NaN without one."""
    out = np.full(pod_groups.size - 1, np.nan)
    for s in range(out.size):
        v = per_pod[pod_groups[s]:pod_groups[s + 1]]
        v = v[~np.isnan(v)]
        if v.size:
            out[s] = v.max()
    return out


class BurstSettings(StrategySettings):
    window_slots: int = pd.Field(5, ge=1, le=_native.KRR_SLIDE_MAX_WINDOW,
                                 description="Slots per sliding window (5 on a 1-minute step: five minutes).")
    cpu_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the sliding means.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory peak (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


class BurstStrategy(BaseStrategy[BurstSettings]):
    __display_name__ = "burst"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        pods = batch.per_pod(ResourceType.CPU)
        sl = pods.sliding(ResourceType.CPU, st.window_slots)  # the mean of every full window, and the peak
        p95 = sl.as_batch("mean").percentile(ResourceType.CPU, st.cpu_percentile, mode="linear")
        req = max_over_pods(p95, pods.pod_groups)
        lim = max_over_pods(sl.peak, pods.pod_groups)
        absent = _native.KRR_FLAG_EMPTY  # no full window in any pod: Decimal('NaN')
        cpu_req = batch.to_decimal(req, np.where(np.isnan(req), absent, 0))
        cpu_lim = batch.to_decimal(lim, np.where(np.isnan(lim), absent, 0))
        ms = batch.stats(ResourceType.Memory)
        mem = batch.to_decimal(ms.max, ms.flags)
        results = []
        with decimal.localcontext(reference_context()):
            buffer = 1 + st.memory_buffer_percentage / 100
            for c, l, m in zip(cpu_req, cpu_lim, mem):
                m = m * buffer  # NaN stays NaN: the runner prints "?"
                results.append({ResourceType.CPU: ResourceRecommendation(request=c, limit=l),
                                ResourceType.Memory: ResourceRecommendation(request=m, limit=m)})
        return results

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        return self.run_batch([history_data], [object_data])[0]

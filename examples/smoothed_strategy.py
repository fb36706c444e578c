"""A fourth custom strategy on the GPU path: size CPU from SMOOTHED usage.

    CPU request    = the 95th percentile (numpy's linear rule) of the object's 5-slot window means
    CPU limit      = the highest 5-slot window mean (the sustained peak)
    memory request = max(samples) x (1 + memory_buffer_percentage / 100), also the limit

CPU is compressible: a one-slot spike is throttled for one slot and should not size a request,
which is why autoscalers size from averages over a few minutes.  On a one-minute scrape step a
window of 5 slots is the 5-minute mean.  ``run_batch`` cuts every series into windows with ONE
``FleetBatch.rollup`` call (a single krr_segmented_rollup pass); the window means stay in HBM as a
series of their own, whose percentile and maximum are the calls every FleetBatch has.  One
Decimal multiplication per object stays on the host.  ``run()`` is the same code over a fleet of
one.

    from examples.smoothed_strategy import SmoothedStrategy, SmoothedSettings
    strategy = SmoothedStrategy(SmoothedSettings(window_slots=5))
    results = BatchedRunner(strategy).recommend(objects, histories)
"""
from __future__ import annotations

import decimal
from decimal import Decimal
from typing import Optional, Sequence

import pydantic.v1 as pd

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


class SmoothedSettings(StrategySettings):
    window_slots: int = pd.Field(5, ge=1, description="Slots per window (5 on a 1-minute step: 5-minute means).")
    cpu_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the window means.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory peak (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


class SmoothedStrategy(BaseStrategy[SmoothedSettings]):
    __display_name__ = "smoothed"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        ru = batch.rollup(ResourceType.CPU, st.window_slots)  # windows end at each series' last sample
        means = ru.as_batch("mean")
        req, req_flags = means.percentile(ResourceType.CPU, st.cpu_percentile, mode="linear", return_flags=True)
        cpu_req = batch.to_decimal(req, req_flags)  # Decimal('NaN') for objects without samples
        cpu_lim = batch.to_decimal(ru.peak("mean"), means.stats(ResourceType.CPU).flags)
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

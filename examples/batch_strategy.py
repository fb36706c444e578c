"""A custom strategy on the GPU path.

    CPU request    = mean(samples) x cpu_headroom
    memory request = percentile(samples, memory_percentile) x (1 + memory_buffer_percentage / 100)

``run_batch`` is the hook ``krr_amd.core.runner.BatchedRunner`` calls once for the whole fleet:
``FleetBatch`` packs the histories and computes every object's mean (one krr_segmented_stats
pass) and memory percentile (krr_segmented_percentiles) on the device; the Decimal arithmetic
left on the host is one multiplication per object.  ``run()`` — what the reference's Runner
calls per object — is the same code over a fleet of one.

    from examples.batch_strategy import MeanHeadroomStrategy, MeanHeadroomSettings
    strategy = MeanHeadroomStrategy(MeanHeadroomSettings(cpu_headroom=Decimal("1.3")))
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


class MeanHeadroomSettings(StrategySettings):
    cpu_headroom: Decimal = pd.Field(Decimal("1.5"), gt=0, description="CPU request = mean usage times this factor.")
    memory_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the memory usage.")
    memory_percentile_mode: str = pd.Field("sorted_lower", description="ref_index, sorted_lower or linear.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory percentile (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


class MeanHeadroomStrategy(BaseStrategy[MeanHeadroomSettings]):
    __display_name__ = "mean_headroom"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        cpu = batch.stats(ResourceType.CPU)
        mean = batch.to_decimal(cpu.mean, cpu.flags)  # Decimal('NaN') for objects without samples
        mem, mem_flags = batch.percentile(ResourceType.Memory, st.memory_percentile, mode=st.memory_percentile_mode,
                                          return_flags=True)
        mem = batch.to_decimal(mem, mem_flags)
        results = []
        with decimal.localcontext(reference_context()):
            buffer = 1 + st.memory_buffer_percentage / 100
            for c, m in zip(mean, mem):
                c, m = c * st.cpu_headroom, m * buffer  # NaN stays NaN: the runner prints "?"
                results.append({ResourceType.CPU: ResourceRecommendation(request=c, limit=None),
                                ResourceType.Memory: ResourceRecommendation(request=m, limit=m)})
        return results

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        return self.run_batch([history_data], [object_data])[0]

"""A fifth custom strategy on the GPU path: size CPU for an EVEN spread over the replicas.

    CPU request    = the 95th percentile (numpy's linear rule) of the object's per-replica load,
                     total / active per slot: what each pod would use if the work were balanced
    CPU limit      = the 99th percentile of the busiest-pod envelope (the max over pods per slot)
    memory request = max(samples) x (1 + memory_buffer_percentage / 100), also the limit

``simple`` concatenates the pods' samples, ``pods_max`` takes the single worst pod; a workload
behind a load balancer sits between the two.  ``run_batch`` folds every object's pods slot by slot
with ONE ``FleetBatch.overlay`` call (a single krr_pods_overlay pass): the workload's total, the
pods up and the busiest pod per slot stay in HBM, and ``as_batch`` hands the balanced share and
the envelope to the percentile calls every FleetBatch has.  The slots are the pods' own: with
compact histories the pods are lined up at their last sample (``align="end"``), on a dense grid
(``pack_dense_grid``) a slot is a point in time.  One Decimal multiplication per object stays on
the host.  ``run()`` is the same code over a fleet of one.

    from examples.balanced_strategy import BalancedStrategy, BalancedSettings
    strategy = BalancedStrategy(BalancedSettings(cpu_percentile=95))
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


class BalancedSettings(StrategySettings):
    cpu_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the per-replica load.")
    cpu_limit_percentile: Decimal = pd.Field(99, gt=0, le=100, description="The percentile of the busiest-pod envelope.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory peak (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


class BalancedStrategy(BaseStrategy[BalancedSettings]):
    __display_name__ = "balanced"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        ov = batch.overlay(ResourceType.CPU)  # the pods end together, at each one's last sample
        req, req_flags = ov.as_batch("mean").percentile(ResourceType.CPU, st.cpu_percentile, mode="linear",
                                                        return_flags=True)
        lim, lim_flags = ov.as_batch("max").percentile(ResourceType.CPU, st.cpu_limit_percentile, mode="linear",
                                                       return_flags=True)
        cpu_req = batch.to_decimal(req, req_flags)  # Decimal('NaN') for objects without samples
        cpu_lim = batch.to_decimal(lim, lim_flags)
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

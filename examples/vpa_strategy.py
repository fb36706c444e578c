"""A custom strategy on the GPU path in the shape of Kubernetes VPA's recommender.

    per pod: the decaying histogram of its CPU usage (a sample's weight halves every
             ``half_life_slots`` slots of age; with one sample a minute 1440 is VPA's one day)
    lower bound = p50, target = p90, upper bound = p95 of that histogram, each the END of the
             bucket that holds the percentile, all three read from ONE histogram
    CPU request    = max over the object's pods of the target x (1 + cpu_margin_percentage / 100)
    CPU limit      = max over the object's pods of the upper bound x the same margin
    memory request = memory limit = max(samples) x (1 + memory_buffer_percentage / 100)

VPA keeps one histogram per container and reads its three estimates from it; here
``FleetBatch.per_pod(...).histogram(...)`` builds every pod's histogram in one launch over the
fleet (krr_segmented_whist: integer weights over data-independent log-linear bins, at most 6.25%
wide by default), and ``FleetHistogram.percentiles`` reads the three percentiles from the rows in
one more, without touching the samples again.  The end of a bucket is never below the exact
weighted percentile (``FleetBatch.weighted_percentile``) and at most one bin width above it.  The
lower bound does not enter the result; ``estimates()`` returns it with the other two.  ``run()`` is
the same code over a fleet of one.
On HistoryData lists age counts a pod's samples from its last one, not wall-clock minutes.

    from examples.vpa_strategy import VpaStrategy, VpaSettings
    strategy = VpaStrategy(VpaSettings(half_life_slots=1440))
    results = BatchedRunner(strategy).recommend(objects, histories)
"""
from __future__ import annotations

import decimal
from decimal import Decimal
from typing import Optional, Sequence

import pydantic.v1 as pd

from examples.recency_strategy import weighted_pods_to_objects
from krr_amd.api import FleetBatch, decay_weights
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


class VpaSettings(StrategySettings):
    lower_percentile: Decimal = pd.Field(50, gt=0, le=100, description="The lower bound's percentile.")
    target_percentile: Decimal = pd.Field(90, gt=0, le=100, description="The target's percentile: the CPU request.")
    upper_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The upper bound's percentile: the CPU limit.")
    half_life_slots: int = pd.Field(1440, ge=1, description="Slots of age after which a sample's weight has halved.")
    cpu_margin_percentage: Decimal = pd.Field(15, ge=0, description="Safety margin added to the CPU estimates (%).")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory peak (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


class VpaStrategy(BaseStrategy[VpaSettings]):
    __display_name__ = "vpa"

    def estimates(self, batch: FleetBatch) -> list:
        """[lower, target, upper]: per object the max over its pods of the three percentiles' bucket
        ends, as list[Decimal] each (Decimal('NaN') for an object without a weighted sample)."""
        st = self.settings
        pods = batch.per_pod(ResourceType.CPU)
        table = decay_weights(st.half_life_slots, max(int(pods.series(ResourceType.CPU).max_len), 1))
        hist = pods.histogram(ResourceType.CPU, table)
        ends, flags = hist.percentiles([st.lower_percentile, st.target_percentile, st.upper_percentile],
                                       return_flags=True)
        out = []
        for row, row_flags in zip(ends, flags):
            value, obj_flags = weighted_pods_to_objects(row, row_flags, pods.pod_groups)
            out.append(batch.to_decimal(value, obj_flags))
        return out

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        _, target, upper = self.estimates(batch)
        ms = batch.stats(ResourceType.Memory)
        mem = batch.to_decimal(ms.max, ms.flags)
        results = []
        with decimal.localcontext(reference_context()):
            margin = 1 + Decimal(st.cpu_margin_percentage) / 100
            buffer = 1 + Decimal(st.memory_buffer_percentage) / 100
            for c, l, m in zip(target, upper, mem):
                m = m * buffer  # NaN stays NaN: the runner prints "?"
                results.append({ResourceType.CPU: ResourceRecommendation(request=c * margin, limit=l * margin),
                                ResourceType.Memory: ResourceRecommendation(request=m, limit=m)})
        return results

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        return self.run_batch([history_data], [object_data])[0]

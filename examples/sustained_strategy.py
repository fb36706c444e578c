"""A third custom strategy on the GPU path: the lowest request that is not breached for long.

    CPU request    = the lowest of the candidate percentiles of the object's samples (default
                     50, 75, 90, 95) above which the object spent at most ``max_share`` of its
                     samples and never more than ``max_sustained_slots`` samples in a row;
                     the highest candidate if none qualifies
    memory request = percentile(samples, memory_percentile) x (1 + memory_buffer_percentage / 100)

A percentile alone says how OFTEN usage was above it, not for how long at a stretch: a pod that
sits above its p90 for an hour on end is throttled for an hour, one that crosses it for a minute
sixty times is not.  ``run_batch`` takes the candidates from ONE ``FleetBatch.percentiles`` call
and looks back at the samples with ONE ``FleetBatch.exceedance`` call of four thresholds per
object (a single krr_segmented_exceed pass); the choice is numpy over [4, S] arrays and one
Decimal multiplication per object stays on the host.  ``run()`` is the same code over a fleet of
one.

    from examples.sustained_strategy import SustainedStrategy, SustainedSettings
    strategy = SustainedStrategy(SustainedSettings(max_share=0.1, max_sustained_slots=5))
    results = BatchedRunner(strategy).recommend(objects, histories)
"""
from __future__ import annotations

import decimal
from decimal import Decimal
from typing import Optional, Sequence

import numpy as np
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


class SustainedSettings(StrategySettings):
    cpu_percentiles: list[Decimal] = pd.Field([Decimal(50), Decimal(75), Decimal(90), Decimal(95)], min_items=1,
                                              description="Candidate CPU percentiles, lowest first.")
    cpu_percentile_mode: str = pd.Field("sorted_lower", description="ref_index, sorted_lower or linear.")
    max_share: float = pd.Field(0.3, ge=0, le=1, description="Largest part of the samples allowed above the request.")
    max_sustained_slots: int = pd.Field(5, ge=0, description="Longest run of samples allowed above the request.")
    memory_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the memory usage.")
    memory_percentile_mode: str = pd.Field("sorted_lower", description="ref_index, sorted_lower or linear.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory percentile (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


def lowest_sustainable(share: np.ndarray, longest: np.ndarray, max_share: float, max_sustained_slots: int) -> np.ndarray:
    """int64 [S]: per object the first row of [R, S] ``share`` / ``longest`` with share <= max_share
    and longest <= max_sustained_slots, R - 1 where no row qualifies (a NaN share never does)."""
    with np.errstate(invalid="ignore"):
        ok = (share <= max_share) & (longest <= max_sustained_slots)
    return np.where(ok.any(axis=0), ok.argmax(axis=0), share.shape[0] - 1).astype(np.int64)


class SustainedStrategy(BaseStrategy[SustainedSettings]):
    __display_name__ = "sustained"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        ps = sorted(st.cpu_percentiles)
        cand, cand_flags = batch.percentiles(ResourceType.CPU, ps, mode=st.cpu_percentile_mode, return_flags=True)
        ex = batch.exceedance(ResourceType.CPU, cand)  # the candidates are the thresholds: [R, S]
        pick = lowest_sustainable(ex.share, ex.longest, st.max_share, st.max_sustained_slots)
        col = np.arange(cand.shape[1])
        cpu = batch.to_decimal(cand[pick, col], cand_flags[pick, col])  # Decimal('NaN') for objects without samples
        mem, mem_flags = batch.percentile(ResourceType.Memory, st.memory_percentile, mode=st.memory_percentile_mode,
                                          return_flags=True)
        mem = batch.to_decimal(mem, mem_flags)
        results = []
        with decimal.localcontext(reference_context()):
            buffer = 1 + st.memory_buffer_percentage / 100
            for c, m in zip(cpu, mem):
                m = m * buffer  # NaN stays NaN: the runner prints "?"
                results.append({ResourceType.CPU: ResourceRecommendation(request=c, limit=None),
                                ResourceType.Memory: ResourceRecommendation(request=m, limit=m)})
        return results

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        return self.run_batch([history_data], [object_data])[0]

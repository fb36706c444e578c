"""A second custom strategy on the GPU path: headroom from variability and direction.

    CPU request    = max over the object's pods of
                     (pod mean + cpu_sigmas x pod sigma + max(pod slope, 0) x horizon_slots)
    memory request = percentile(samples, memory_percentile) x (1 + memory_buffer_percentage / 100)

The pod slope is the least-squares trend of the pod's samples over their slot index (one slot =
one scrape step), so ``horizon_slots`` is how many steps ahead a climbing pod is provisioned for;
a falling or flat pod adds nothing.  ``run_batch`` asks ``FleetBatch`` for the moments of every
POD in one krr_segmented_moments pass (``per_pod(...).moments(...)``), folds them to objects with
``pod_groups`` in numpy, and leaves one Decimal multiplication per object on the host.  ``run()``
is the same code over a fleet of one.

    from examples.trend_strategy import TrendHeadroomStrategy, TrendHeadroomSettings
    strategy = TrendHeadroomStrategy(TrendHeadroomSettings(cpu_sigmas=3, horizon_slots=1440))
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


class TrendHeadroomSettings(StrategySettings):
    cpu_sigmas: float = pd.Field(2.0, ge=0, description="Standard deviations added to a pod's mean CPU usage.")
    horizon_slots: float = pd.Field(0.0, ge=0, description="Scrape steps ahead a climbing pod is provisioned for.")
    memory_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The percentile of the memory usage.")
    memory_percentile_mode: str = pd.Field("sorted_lower", description="ref_index, sorted_lower or linear.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory percentile (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


def pods_to_objects(pod_values: np.ndarray, pod_flags: np.ndarray, pod_groups: np.ndarray):
    """(float64 [S], uint32 [S]): the max of each object's pod values (NaN if any is NaN) and the
    OR of their flags; an object without pods is NaN with KRR_FLAG_EMPTY."""
    S = pod_groups.size - 1
    value = np.full(S, np.nan)
    flags = np.full(S, _native.KRR_FLAG_EMPTY, dtype=np.uint32)
    has = pod_groups[1:] > pod_groups[:-1]
    if has.any():  # reduceat over the non-empty groups' starts: an empty group shares its start with the next
        starts = pod_groups[:-1][has]
        value[has] = np.maximum.reduceat(pod_values, starts)
        flags[has] = np.bitwise_or.reduceat(pod_flags.astype(np.uint32), starts)
    return value, flags


class TrendHeadroomStrategy(BaseStrategy[TrendHeadroomSettings]):
    __display_name__ = "trend_headroom"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        pods = batch.per_pod(ResourceType.CPU)
        mo = pods.moments(ResourceType.CPU, trend=st.horizon_slots > 0)
        per_pod = mo.mean + st.cpu_sigmas * mo.std()
        if st.horizon_slots > 0:
            slope = mo.slope
            per_pod = per_pod + np.where(slope > 0, slope, 0.0) * st.horizon_slots  # one sample: no slope, no term
        cpu, cpu_flags = pods_to_objects(per_pod, mo.flags, pods.pod_groups)
        cpu = batch.to_decimal(cpu, cpu_flags)  # Decimal('NaN') for objects without samples
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

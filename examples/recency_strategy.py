"""A custom strategy on the GPU path that sizes a workload by what it needs NOW.

    CPU request    = max over the object's pods of the pod's WEIGHTED percentile, a sample's weight
                     halving every ``half_life_slots`` slots of age (cpu_percentile, default 95)
    CPU limit      = the flat percentile of all the object's samples (cpu_limit_percentile, default 99),
                     and never below the request
    memory request = memory limit = max(samples) x (1 + memory_buffer_percentage / 100)

A flat percentile gives a sample from a week ago the say of one from the last hour, so a
deployment re-tuned yesterday is sized by the six days before it.  The decaying weight is what
Kubernetes VPA's histogram applies (half-life one day); here the weighted percentile is exact
(krr_segmented_wquantile: integer weights, no histogram buckets in the answer).  With one sample
a minute ``half_life_slots=1440`` is one day.  The limit stays the flat p99: a burst from last
week is still a burst the limit should admit.

``run_batch`` asks ``FleetBatch`` for the weighted percentile of every POD in one launch
(``per_pod(...).weighted_percentile(...)``), folds the pods to objects with ``pod_groups`` in
numpy and leaves one Decimal multiplication per object on the host.  ``run()`` is the same code
over a fleet of one.  On HistoryData lists age counts a pod's samples from its last one, not
wall-clock minutes: a pod that stopped reporting early is weighted as if it ended now.

    from examples.recency_strategy import RecencyStrategy, RecencySettings
    strategy = RecencyStrategy(RecencySettings(half_life_slots=1440))
    results = BatchedRunner(strategy).recommend(objects, histories)
"""
from __future__ import annotations

import decimal
from decimal import Decimal
from typing import Optional, Sequence

import numpy as np
import pydantic.v1 as pd

from krr_amd import _native
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


class RecencySettings(StrategySettings):
    cpu_percentile: Decimal = pd.Field(95, gt=0, le=100, description="The weighted percentile of a pod's CPU usage.")
    half_life_slots: int = pd.Field(1440, ge=1, description="Slots of age after which a sample's weight has halved.")
    cpu_limit_percentile: Decimal = pd.Field(99, gt=0, le=100, description="The flat percentile for the CPU limit.")
    cpu_limit_percentile_mode: str = pd.Field("sorted_lower", description="ref_index, sorted_lower or linear.")
    memory_buffer_percentage: Decimal = pd.Field(5, ge=0, description="Buffer added to the memory peak (%).")
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")


def weighted_pods_to_objects(pod_values: np.ndarray, pod_flags: np.ndarray, pod_groups: np.ndarray):
    """(float64 [S], uint32 [S]): the max of each object's pod values, a pod without weight (NaN:
    no sample, or only samples older than the table reaches) left out; KRR_FLAG_NAN where a pod
    has it, else KRR_FLAG_EMPTY where no pod of the object has a value."""
    S = pod_groups.size - 1
    value = np.full(S, np.nan)
    nan_flag = np.zeros(S, dtype=np.uint32)
    has = pod_groups[1:] > pod_groups[:-1]
    if has.any():  # reduceat over the non-empty groups' starts: an empty group shares its start with the next
        starts = pod_groups[:-1][has]
        value[has] = np.fmax.reduceat(pod_values, starts)
        nan_flag[has] = np.bitwise_or.reduceat(pod_flags.astype(np.uint32) & _native.KRR_FLAG_NAN, starts)
    empty = np.where(np.isnan(value), np.uint32(_native.KRR_FLAG_EMPTY), np.uint32(0))
    return value, np.where(nan_flag != 0, nan_flag, empty).astype(np.uint32)


class RecencyStrategy(BaseStrategy[RecencySettings]):
    __display_name__ = "recency"

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        st = self.settings
        batch = FleetBatch(histories, device=st.device)
        pods = batch.per_pod(ResourceType.CPU)
        table = decay_weights(st.half_life_slots, max(int(pods.series(ResourceType.CPU).max_len), 1))
        per_pod, pod_flags = pods.weighted_percentile(ResourceType.CPU, st.cpu_percentile, table, return_flags=True)
        req, req_flags = weighted_pods_to_objects(per_pod, pod_flags, pods.pod_groups)
        req = batch.to_decimal(req, req_flags)  # Decimal('NaN') for objects without a weighted sample
        lim, lim_flags = batch.percentile(ResourceType.CPU, st.cpu_limit_percentile,
                                          mode=st.cpu_limit_percentile_mode, return_flags=True)
        lim = batch.to_decimal(lim, lim_flags)
        ms = batch.stats(ResourceType.Memory)
        mem = batch.to_decimal(ms.max, ms.flags)
        results = []
        with decimal.localcontext(reference_context()):
            buffer = 1 + st.memory_buffer_percentage / 100
            for c, l, m in zip(req, lim, mem):
                m = m * buffer  # NaN stays NaN: the runner prints "?"
                if not (c.is_nan() or l.is_nan()) and l < c:
                    l = c  # a recent climb past the week's flat percentile: never a limit below the request
                results.append({ResourceType.CPU: ResourceRecommendation(request=c, limit=l),
                                ResourceType.Memory: ResourceRecommendation(request=m, limit=m)})
        return results

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        return self.run_batch([history_data], [object_data])[0]

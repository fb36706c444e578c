"""simple_limit on MI355X — ``simple`` with a CPU limit: the CPU request comes from one
percentile and the CPU limit from a higher one, both from ONE fused kernel pass
(krr_simple_run_multi: the candidate buffer kept for the request's percentile also holds
the limit's).  ``cpu_aggregation`` "pods_max" takes both per pod and the max over the
object's pods (krr_simple_run_pods_multi), as the later upstream strategy does.  Later
upstream KRR ships a strategy of this name; the reference snapshot this package mirrors
(KRR 1.0.0) does not, so the defaults below are this project's.

  CPU    request = value at ``cpu_request``, limit = value at ``cpu_limit``, each by the
         rule ``percentile_mode`` names (krr_amd.strategies.simple)
  Memory = max(samples) * Decimal(1 + b / 100), limit = request            (as ``simple``)
  empty  -> Decimal('NaN') for both CPU values

``percentile_mode`` defaults to "sorted_lower" here: a limit below the request makes no
sense, and only the sorted rules are monotone in the percentile.  Under "ref_index" each
value is the reference's positional pick X[k] of the UNSORTED samples (simple.py:36), so
the limit MAY fall below the request; it is offered for parity with ``simple``'s CPU value
at either percentile, not as a sensible limit.

NaN samples behave per percentile as ``SimpleStrategySettings.cpu_from_raw`` does.  The
32-byte multi-GPU result record holds one CPU value, so the sharded entry points
(``run_fleet_records``, BatchedRunner.recommend_shard and friends) raise
NotImplementedError for this strategy.
"""
from __future__ import annotations

import decimal
import threading
from decimal import Decimal
from typing import Optional, Sequence

import numpy as np
import pydantic.v1 as pd

from krr_amd.core.abstract.strategies import (
    BaseStrategy,
    HistoryData,
    K8sObjectData,
    ResourceRecommendation,
    ResourceType,
    RunResult,
    StrategySettings,
)
from krr_amd.core.engine import RawResults, default_engine, percentile_params
from krr_amd.core.packing import PackedFleet, pack_resource
from krr_amd.core.rounding import format_result, reference_context
from krr_amd.strategies.simple import CpuAggregation, PercentileMode, SimpleStrategySettings

SHARDED_MESSAGE = ("simple_limit has no multi-GPU sharded path: the 32-byte result record holds one CPU value "
                   "(request and limit need two); run it on one GPU")


class SimpleLimitStrategySettings(StrategySettings):
    cpu_request: Decimal = pd.Field(
        66, gt=0, le=100, description="The percentile to use for the CPU request."
    )
    cpu_limit: Decimal = pd.Field(
        96, gt=0, le=100, description="The percentile to use for the CPU limit (at least cpu_request)."
    )
    memory_buffer_percentage: Decimal = pd.Field(
        5, gt=0, description="The percentage of added buffer to the peak memory usage for memory recommendation."
    )
    percentile_mode: PercentileMode = pd.Field(
        PercentileMode.SORTED_LOWER,
        description="CPU percentile rule: sorted_lower (default), linear (numpy), or ref_index (the reference's "
                    "positional pick: the limit may then fall below the request).",
    )
    cpu_aggregation: CpuAggregation = pd.Field(
        CpuAggregation.CONCAT,
        description="CPU over an object's pods: concat (one percentile over the pods' samples concatenated, "
                    "reference KRR 1.0.0) or pods_max (the max over the pods of each pod's percentile).",
    )
    device: int = pd.Field(0, ge=0, description="HIP device that runs the kernels.")

    @pd.root_validator(skip_on_failure=True)
    def _limit_not_below_request(cls, values):
        # defaults are not validated (pydantic v1): compare as Decimals whatever the types
        if Decimal(str(values["cpu_limit"])) < Decimal(str(values["cpu_request"])):
            raise ValueError("cpu_limit must be at least cpu_request")
        return values

    def percentiles(self) -> tuple:
        return (self.cpu_request, self.cpu_limit)

    def params_list(self) -> list:
        mode = PercentileMode(self.percentile_mode).value
        return [percentile_params(p, mode) for p in self.percentiles()]

    def simple_settings(self) -> SimpleStrategySettings:
        """``simple``'s settings with this strategy's mode, buffer and device (field values as
        they are here, unvalidated: an int default stays an int, as in the reference): its
        cpu_from_raw / memory_from_raw turn raw kernel results into Decimals."""
        return SimpleStrategySettings.construct(
            cpu_percentile=self.cpu_request, memory_buffer_percentage=self.memory_buffer_percentage,
            percentile_mode=PercentileMode(self.percentile_mode),
            cpu_aggregation=CpuAggregation(self.cpu_aggregation), device=self.device,
            history_duration=self.history_duration, timeframe_duration=self.timeframe_duration)

    def memory_buffer(self) -> Decimal:
        with decimal.localcontext(reference_context()):
            return Decimal(1 + self.memory_buffer_percentage / 100)

    def run_fleet_multi(self, fleet: PackedFleet, device: Optional[int] = None) -> list:
        """One fused pass -> [RawResults at cpu_request, RawResults at cpu_limit] (they share
        the memory arrays).  ``cpu_aggregation`` "pods_max": request and limit per pod, each the
        max over the object's pods — its own first maximal pod — from one fused launch plus one
        fold (krr_simple_run_pods_multi); the fleet's CPU series must carry pod boundaries (every
        packer attaches them, the device packer included; a series built by hand without them:
        ValueError).  NaN samples among the CPU values stay out of
        contract, as in ``simple``: ``cpu_from_raw`` sees the folded flags and count."""
        params = self.params_list()
        engine = default_engine(self.device if device is None else device)
        exact = fleet.cpu.exact is not None or fleet.mem.exact is not None
        agg = CpuAggregation(self.cpu_aggregation).value
        if agg == CpuAggregation.PODS_MAX.value:
            raws = engine.run_packed_multi(fleet, params, aggregation=agg, return_pods=exact)
            if exact and fleet.n_objects:
                from krr_amd.core.exact import resolve_pods

                for raw, p in zip(raws, params):
                    resolve_pods(fleet, raw, p)
            return raws
        raws = engine.run_packed_multi(fleet, params)
        if exact:
            from krr_amd.core.exact import resolve

            for raw, p in zip(raws, params):
                resolve(fleet, raw, p)
        return raws

    def run_fleet(self, fleet: PackedFleet, device: Optional[int] = None) -> RawResults:
        raise NotImplementedError("simple_limit returns two CPU values per object: use run_fleet_multi")

    def run_fleet_records(self, fleet: PackedFleet, device: Optional[int] = None):
        raise NotImplementedError(SHARDED_MESSAGE)


_COALESCER_LOCK = threading.Lock()


class SimpleLimitStrategy(BaseStrategy[SimpleLimitStrategySettings]):
    __display_name__ = "simple_limit"

    def run(self, history_data: HistoryData, object_data: K8sObjectData) -> RunResult:
        """One object; overlapping calls share a launch (krr_amd.core.coalesce.RunCoalescer).
        Equal to run_batch([history_data])[0]."""
        raws, i = self.coalescer().submit(history_data)
        return self.result_at(raws, i)

    def coalescer(self):
        c = self.__dict__.get("_coalescer")
        if c is None:
            from krr_amd.core.coalesce import RunCoalescer

            with _COALESCER_LOCK:
                c = self.__dict__.get("_coalescer")
                if c is None:
                    c = self.__dict__["_coalescer"] = RunCoalescer(
                        lambda hs: self.settings.run_fleet_multi(self.pack(hs)))
        return c

    def result_at(self, raws: Sequence[RawResults], i: int, buffer: Optional[Decimal] = None,
                  simple: Optional[SimpleStrategySettings] = None) -> RunResult:
        st = simple or self.settings.simple_settings()
        request = st.cpu_from_raw(raws[0], i)
        limit = st.cpu_from_raw(raws[1], i)
        mem = st.memory_from_raw(raws[0], i, buffer)
        return {
            ResourceType.CPU: ResourceRecommendation(request=request, limit=limit),
            ResourceType.Memory: ResourceRecommendation(request=mem, limit=mem),
        }

    def run_batch(self, histories: Sequence[HistoryData],
                  objects: Optional[Sequence[K8sObjectData]] = None) -> list[RunResult]:
        """One fleet-wide kernel pass for every object and both percentiles."""
        return self.results_from_raw(self.settings.run_fleet_multi(self.pack(histories)))

    @staticmethod
    def pack(histories: Sequence[HistoryData]) -> PackedFleet:
        return PackedFleet(pack_resource(histories, ResourceType.CPU), pack_resource(histories, ResourceType.Memory))

    def results_from_raw(self, raws: Sequence[RawResults]) -> list[RunResult]:
        st = self.settings.simple_settings()
        buffer = self.settings.memory_buffer()
        return [self.result_at(raws, i, buffer, st) for i in range(int(np.asarray(raws[0].cpu_value).size))]

    def format_packed(self, fleet: PackedFleet, cpu_min_value: int, memory_min_value: int) -> list[RunResult]:
        """Kernel pass + the reference's rounding (Runner._format_result) for a packed fleet:
        format_result over run_batch's results (the Python restatement: both CPU values)."""
        return [format_result(r, cpu_min_value, memory_min_value)
                for r in self.results_from_raw(self.settings.run_fleet_multi(fleet))]

    def format_raw(self, raw, cpu_min_value: int, memory_min_value: int) -> list[RunResult]:
        raise NotImplementedError(SHARDED_MESSAGE)

    def allocations_from_packed(self, fleet: PackedFleet, cpu_min_value: int, memory_min_value: int, model=None,
                                resource_type=None) -> list:
        """The BatchedRunner's packed hook: one ResourceAllocations per object with both CPU
        values (``model`` / ``resource_type``: the reference's own classes, default this
        package's mirror)."""
        from krr_amd.core.models.allocations import ResourceAllocations

        model = model or ResourceAllocations
        rtypes = list(resource_type or ResourceType)
        out = []
        for r in self.format_packed(fleet, cpu_min_value, memory_min_value):
            by = [r[rt] for rt in ResourceType]
            out.append(model(requests={k: v.request for k, v in zip(rtypes, by)},
                             limits={k: v.limit for k, v in zip(rtypes, by)}))
        return out


__all__ = ["SimpleLimitStrategy", "SimpleLimitStrategySettings"]

"""TEST INFRASTRUCTURE: ``SimpleEngine.run_packed_multi`` stood in for by the CPU oracle.

One ``oracle.percentile`` call per percentile (``_standin.oracle_run_packed``: values, counts,
flags, and krr_locate's answers for HistoryData outside Prometheus' canonical strings), so
the CPU tests of ``simple_limit`` check everything above the kernels without a GPU."""
from __future__ import annotations

from _standin import oracle_run_packed


def oracle_run_packed_multi(self, fleet, params_list):
    return [oracle_run_packed(self, fleet, params) for params in params_list]


def install(monkeypatch):
    from krr_amd.core.engine import SimpleEngine

    monkeypatch.setattr(SimpleEngine, "run_packed_multi", oracle_run_packed_multi)
    monkeypatch.setattr(SimpleEngine, "run_packed", oracle_run_packed)
    monkeypatch.setattr(SimpleEngine, "context", lambda self: None)

"""Public plugin-author surface: ``krr_amd.api.strategies`` / ``krr_amd.api.models`` (the
reference's names) and ``FleetBatch``, the fleet statistics a custom strategy's ``run_batch``
computes on the device (krr_amd.api.batch)."""
from krr_amd.api.batch import (FleetBatch, FleetExceedance, FleetHistogram, FleetMoments, FleetOverlay, FleetProfile,
                               FleetRollup, FleetSliding, FleetStats, HistogramBins, allocation_thresholds,
                               decay_weights,
                               default_bins, window_weights)

__all__ = ["FleetBatch", "FleetExceedance", "FleetHistogram", "FleetMoments", "FleetOverlay", "FleetProfile",
           "FleetRollup", "FleetSliding", "FleetStats", "HistogramBins", "allocation_thresholds", "decay_weights",
           "default_bins", "window_weights"]

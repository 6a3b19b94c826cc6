"""srcdsp_amd -- MI355X (gfx950) implementation of SrcDsp's sample-buffer hot path.

The operators (FilterDnsamplingFir, FilterFir, FilterUpsamplingFir, Mixer,
FixedPatternCorrelator, DemodulatorOqpsk, SymbolMapperSdpsk, SymbolMapperQpsk, FifoWithTimeTrack; the OQPSK Q-rail stagger QStagger; estimateFreq (FreqEstimator); files.read/saveBinarySamples) mirror the reference classes and run in the HIP
kernels of libsrcdsp_hip.so through its C ABI (include/srcdsp_hip.h).
"""
from ._capi import SrcdspError, lib  # noqa: F401
from . import files  # noqa: F401
from .operators import (  # noqa: F401
    DemodulatorOqpsk,
    demod_acquire_batched,
    demod_step_batched,
    estimate_freq,
    FreqEstimator,
    demod_tables,
    FifoWithTimeTrack,
    FilterDnsamplingFir,
    FilterFir,
    FilterUpsamplingFir,
    FixedPatternCorrelator,
    Mixer,
    MixerDecimatorChain,
    corr_all_stats,
    corr_batched_stats,
    corr_step_all_batched,
    corr_step_batched,
    decim_step_batched,
    fill_synthetic,
    mixdecim_batched_stats,
    mixdecim_step_batched,
    UpsamplerMixerChain,
    upmix_stats,
    upmix_step_batched,
    SymbolMapperSdpsk,
    SymbolMapperQpsk,
    mapper_step_batched,
    ModulatorChain,
    modulate_step_batched,
    modulate_stats,
    QStagger,
    stagger_geometry,
    stagger_step_batched,
    OffsetModulatorChain,
    modulate_offset_step,
    modulate_offset_step_batched,
    modulate_offset_stats,
)

__all__ = ["FifoWithTimeTrack", "files", "FilterDnsamplingFir", "FilterFir", "FilterUpsamplingFir", "Mixer", "MixerDecimatorChain",
           "UpsamplerMixerChain", "upmix_step_batched", "upmix_stats",
           "SymbolMapperSdpsk", "SymbolMapperQpsk", "mapper_step_batched", "ModulatorChain", "modulate_step_batched",
           "modulate_stats",
           "QStagger", "stagger_geometry", "stagger_step_batched", "OffsetModulatorChain", "modulate_offset_step",
           "modulate_offset_step_batched", "modulate_offset_stats",
           "FixedPatternCorrelator", "decim_step_batched", "mixdecim_step_batched", "mixdecim_batched_stats",
           "corr_step_batched", "corr_batched_stats", "corr_step_all_batched", "corr_all_stats", "DemodulatorOqpsk", "demod_step_batched", "demod_tables",
           "FreqEstimator", "estimate_freq", "demod_acquire_batched",
           "fill_synthetic", "SrcdspError", "lib"]

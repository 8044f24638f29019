"""openmeters_amd — MI355X-native DSP hot path behind OpenMeters' processor API.

The product is the C-ABI shared library ``openmeters_amd/csrc/libomx_hip.so`` (hand-written HIP
for gfx950, declared in ``include/omx.h``).  This package is only the Python-side mirror of the
reference's processor interface on top of that library (``capi.py``) plus the multi-GPU sharding
helper (``sharding.py``).  There is no CPU fallback: if the HIP library is missing the import of
``api()`` raises, and every entry point returns ``OMX_ERR_NO_DEVICE`` without a gfx950 device.
"""
from __future__ import annotations

import os

from . import capi
from .capi import (  # noqa: F401  (re-exported: the reference's config / snapshot vocabulary)
    AudioBlock, LoudnessConfig, OscilloscopeConfig, SpectrogramConfig, SpectrumConfig, StereometerConfig, WaveformConfig,
    OmxError,
)
from .program_loudness import ProgramLoudnessBank, ProgramLoudnessRecord  # noqa: F401  (include/omx/program_loudness.h)
from .program_loudness import ProgramPeakRecord  # noqa: F401  (include/omx/program_peaks.h)
from .program_loudness import CProgramTimelineRow, CProgramInterval  # noqa: F401  (include/omx/program_timeline.h)
from .program_loudness import CProgramHistogram, ProgramHistogram, histogram_boundaries  # noqa: F401  (include/omx/program_histogram.h)
from .program_loudness import CProgramGroup, GROUP_DTYPE, TO_END  # noqa: F401  (include/omx/program_groups.h)
from .program_loudness import (  # noqa: F401  (include/omx/program_normalize.h)
    APPLY_RECORD_DTYPE, GAIN_RECORD_DTYPE, UNITY_GAIN, CProgramApplyRecord, CProgramGainRecord, CProgramGainRule, GainRule, evaluate_gain)
from .program_loudness import (  # noqa: F401  (include/omx/program_limit.h)
    LIMIT_RECORD_DTYPE, CProgramLimitRecord, CProgramLimitRule, LimitRule, limit_latency)
from .program_loudness import (  # noqa: F401  (include/omx/program_pcm.h)
    DITHER_NONE, DITHER_TPDF, EXPORT_RECORD_DTYPE, PCM_S16, PCM_S24, PCM_S32, CProgramExportRecord, CProgramExportRule, ExportRule,
    dither_value, pcm_format_bytes)
from .program_loudness import (  # noqa: F401  (include/omx/program_resample.h)
    RESAMPLE_INFO_DTYPE, RESAMPLE_RECORD_DTYPE, CProgramResampleInfo, CProgramResampleRecord, CProgramResampleRule, ResampleRule,
    resample_frames, resample_plan, resample_taps)
from .program_loudness import (  # noqa: F401  (include/omx/program_remix.h)
    REMIX_INFO_DTYPE, REMIX_KIND_MONO, REMIX_KIND_STEREO, REMIX_MAX_MATRICES, REMIX_NORMALIZE, REMIX_RECORD_DTYPE, CProgramDownmixRule,
    CProgramRemixInfo, CProgramRemixRecord, DownmixRule, remix_downmix, remix_plan, remix_select)
from .program_loudness import (  # noqa: F401  (include/omx/program_inspect.h)
    INSPECT_ALL_SILENT, INSPECT_ANTIPHASE, INSPECT_CLIPPED, INSPECT_DB_FLOOR, INSPECT_DC, INSPECT_DROPOUT, INSPECT_INFO_DTYPE,
    INSPECT_MAX_PAIRS, INSPECT_NAN, INSPECT_RECORD_DTYPE, INSPECT_SUMMARY_DTYPE, CProgramInspectChannel, CProgramInspectInfo,
    CProgramInspectPair, CProgramInspectRecord, CProgramInspectRule, CProgramInspectSummary, InspectRule, inspect_plan,
    inspect_rule_default, inspect_summarize)
from .program_loudness import (  # noqa: F401  (include/omx/program_edit.h)
    EDIT_CLIP_DTYPE, EDIT_CURVE_EQUAL_POWER, EDIT_CURVE_LINEAR, EDIT_CURVE_POINTS, EDIT_CURVE_RAISED_COSINE, EDIT_INFO_DTYPE, EDIT_MAX_FADE,
    EDIT_MAX_OUTPUTS, EDIT_MAX_POSITION, EDIT_RECORD_DTYPE, CProgramEditClip, CProgramEditInfo, CProgramEditRecord, CProgramTrimRule,
    EditClip, TrimRule, edit_curve, edit_extent, edit_gain, edit_plan, edit_table, edit_trim)
from .program_loudness import (  # noqa: F401  (include/omx/program_peak_timeline.h)
    PART_PEAK_DTYPE, PEAK_ROW_DTYPE, CProgramPartPeak, CProgramPeakRow)
from .program_loudness import (  # noqa: F401  (include/omx/program_filter.h)
    FILTER_BYPASS, FILTER_DC_BLOCK, FILTER_DEEMPHASIS, FILTER_DTYPE, FILTER_HIGH_SHELF, FILTER_HIGHPASS, FILTER_INFO_DTYPE,
    FILTER_LOW_SHELF, FILTER_LOWPASS, FILTER_MAX_FILTERS, FILTER_MAX_SECTIONS, FILTER_NOTCH, FILTER_PEAKING, FILTER_PREEMPHASIS,
    FILTER_RECORD_DTYPE, CProgramFilter, CProgramFilterInfo, CProgramFilterRecord, CProgramFilterSection, CProgramFilterSpec, FilterSpec,
    filter_cascade, filter_check, filter_design, filter_plan, filter_response, filter_table)
from .program_loudness import (  # noqa: F401  (include/omx/program_mix.h)
    MIX_INFO_DTYPE, MIX_MAX_BUSES, MIX_MAX_LAYERS, MIX_MAX_POSITION, MIX_MAX_SENDS, MIX_RECORD_DTYPE, MIX_SEND_DTYPE, CProgramMixInfo,
    CProgramMixRecord, CProgramMixSend, MixSend, mix_extent, mix_null, mix_plan, mix_table)
from .program_loudness import (  # noqa: F401  (include/omx/program_convolve.h)
    CONVOLVE_BANDPASS, CONVOLVE_BANDSTOP, CONVOLVE_BYPASS, CONVOLVE_FLUSHED, CONVOLVE_HIGHPASS, CONVOLVE_IDLE, CONVOLVE_INFO_DTYPE,
    CONVOLVE_LOWPASS, CONVOLVE_MAX_FIRS, CONVOLVE_MAX_TAPS, CONVOLVE_RECORD_DTYPE, CONVOLVE_RUNNING, ConvolveSpec, CProgramConvolveInfo,
    CProgramConvolveRecord, CProgramConvolveSpec, CProgramFir, convolve_check, convolve_design, convolve_frames, convolve_plan,
    convolve_response)
from .program_loudness import (  # noqa: F401  (include/omx/program_dynamics.h)
    DYNAMICS_BYPASS, DYNAMICS_CURVE_POINTS, DYNAMICS_FLUSHED, DYNAMICS_IDLE, DYNAMICS_INFO_DTYPE, DYNAMICS_L_MAX, DYNAMICS_L_MIN,
    DYNAMICS_MAX_ATTACK, DYNAMICS_MAX_CURVES, DYNAMICS_MAX_GAIN, DYNAMICS_MAX_HOLD, DYNAMICS_MAX_POINTS, DYNAMICS_MAX_STEP,
    DYNAMICS_OCTAVE_DB, DYNAMICS_RECORD_DTYPE, DYNAMICS_RUNNING, DYNAMICS_TABLE_ENTRIES, CProgramDynamicsCurve, CProgramDynamicsInfo,
    CProgramDynamicsPoint, CProgramDynamicsRecord, CProgramDynamicsSpec, DynamicsCurve, DynamicsSpec, dynamics_check, dynamics_design,
    dynamics_frames, dynamics_from_points, dynamics_gain_db, dynamics_latency, dynamics_plan, dynamics_tables, dynamics_time)
from .program_loudness import (  # noqa: F401  (include/omx/program_spectrum.h)
    SPECTRUM_BANDLIMITED, SPECTRUM_DB_FLOOR, SPECTRUM_INFO_DTYPE, SPECTRUM_MAX_BANDS, SPECTRUM_MAX_PROBES, SPECTRUM_MAX_TAPS,
    SPECTRUM_RECORD_DTYPE, SPECTRUM_RUN, SPECTRUM_SUMMARY_DTYPE, SPECTRUM_TONE, CProgramSpectrumInfo, CProgramSpectrumMatchSpec,
    CProgramSpectrumQc, CProgramSpectrumRecord, CProgramSpectrumRule, CProgramSpectrumSummary, SpectrumMatchSpec, SpectrumQc, SpectrumRule,
    spectrum_bands, spectrum_density, spectrum_match, spectrum_match_spec_default, spectrum_plan, spectrum_qc_default,
    spectrum_rule_default, spectrum_summarize, spectrum_transforms, spectrum_window)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMX_HIP_LIB") or os.path.join(_HERE, "csrc", "libomx_hip.so")  # OMX_HIP_LIB: A/B builds (tuning)
_API = None


def api() -> capi.Api:
    """The product C-ABI (prefix ``omx_``).  Fails loudly when the HIP extension is not built."""
    global _API
    if _API is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  openmeters_amd has no CPU fallback.")
        # PyTorch wheels bundle their own libamdhip64; a process must not end up with two HIP runtimes (the second one
        # sees no device).  Loading torch first makes libomx_hip.so's NEEDED libamdhip64.so.7 resolve to the copy that is
        # already mapped, whatever order the caller imports things in.  Hosts without torch (the Rust binding) have one
        # runtime anyway.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _API = capi.Api(LIB_PATH, "omx_")
    return _API


def device_available() -> bool:
    import ctypes
    return bool(api().fn("device_available", ctypes.c_int, [])())

"""Programme loudness bank (include/omx/program_loudness.h): gated integrated loudness (BS.1770-4), loudness range
(EBU Tech 3342) and the maxima of momentary loudness, short-term loudness and true peak for S streams on one GPU.
Inputs are device pointers; nothing here touches sample data."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import Api

_u8x8 = C.c_uint8 * 8

_ENERGIES = ("integrated_energy", "relative_threshold_energy", "lra_low_energy", "lra_high_energy", "momentary_energy",
             "short_term_energy", "max_momentary_energy", "max_short_term_energy")
_COUNTS = ("frames", "segments", "gating_blocks", "gating_above_absolute", "gating_above_relative", "short_term_blocks",
           "short_term_above_absolute", "short_term_above_relative")
_LEVELS = ("integrated_lufs", "relative_threshold_lufs", "loudness_range_lu", "momentary_lufs", "short_term_lufs",
           "max_momentary_lufs", "max_short_term_lufs", "max_true_peak_db")


class CProgramLoudnessRecord(C.Structure):
    _fields_ = ([(n, C.c_double) for n in _ENERGIES] + [(n, C.c_uint64) for n in _COUNTS] + [(n, C.c_float) for n in _LEVELS]
                + [("overflow", C.c_uint32), ("_pad", C.c_uint32)])


@dataclass
class ProgramLoudnessRecord:
    """omx_program_loudness_record: dB fields floored at the configured floor, the f64 energies they were made from, counts."""
    integrated_energy: float
    relative_threshold_energy: float
    lra_low_energy: float
    lra_high_energy: float
    momentary_energy: float
    short_term_energy: float
    max_momentary_energy: float
    max_short_term_energy: float
    frames: int
    segments: int
    gating_blocks: int
    gating_above_absolute: int
    gating_above_relative: int
    short_term_blocks: int
    short_term_above_absolute: int
    short_term_above_relative: int
    integrated_lufs: float
    relative_threshold_lufs: float
    loudness_range_lu: float
    momentary_lufs: float
    short_term_lufs: float
    max_momentary_lufs: float
    max_short_term_lufs: float
    max_true_peak_db: float
    overflow: bool

    LEVEL_FIELDS = _LEVELS
    COUNT_FIELDS = _COUNTS
    ENERGY_FIELDS = _ENERGIES


_u64x8, _f32x8 = C.c_uint64 * 8, C.c_float * 8


class CProgramPeakRecord(C.Structure):
    """omx_program_peak_record (include/omx/program_peaks.h)"""
    _fields_ = [("frames", C.c_uint64), ("true_peak_frame", _u64x8), ("sample_peak_frame", _u64x8), ("true_peak", _f32x8),
                ("sample_peak", _f32x8), ("true_peak_db", _f32x8), ("sample_peak_db", _f32x8), ("max_true_peak_db", C.c_float),
                ("max_sample_peak_db", C.c_float), ("max_true_peak_channel", C.c_uint32), ("oversampling", C.c_uint32),
                ("channels", C.c_uint32), ("_pad", C.c_uint32)]


assert C.sizeof(CProgramPeakRecord) == 288


@dataclass
class ProgramPeakRecord:
    """omx_program_peak_record: per channel slot the maximum true peak and sample peak since the last reset (linear f32 and dB) with
    the frame each first occurred at; arrays have 8 entries, slots at or above `channels` hold 0 / the floor."""
    frames: int
    true_peak_frame: np.ndarray      # uint64[8]
    sample_peak_frame: np.ndarray
    true_peak: np.ndarray            # float32[8]
    sample_peak: np.ndarray
    true_peak_db: np.ndarray
    sample_peak_db: np.ndarray
    max_true_peak_db: float
    max_sample_peak_db: float
    max_true_peak_channel: int
    oversampling: int                # 4, 2 or 1; 0 until the stream takes a sample
    channels: int

    def tobytes(self) -> bytes:
        """every field, bit for bit (records compare equal exactly when these do)"""
        return b"".join([np.uint64(self.frames).tobytes(), self.true_peak_frame.tobytes(), self.sample_peak_frame.tobytes(),
                         self.true_peak.tobytes(), self.sample_peak.tobytes(), self.true_peak_db.tobytes(), self.sample_peak_db.tobytes(),
                         np.array([self.max_true_peak_db, self.max_sample_peak_db], np.float32).tobytes(),
                         np.array([self.max_true_peak_channel, self.oversampling, self.channels], np.uint32).tobytes()])


class CProgramTimelineRow(C.Structure):
    """omx_program_timeline_row (include/omx/program_timeline.h)"""
    _fields_ = [("integrated_energy", C.c_double), ("relative_threshold_energy", C.c_double), ("momentary_lufs", C.c_float),
                ("short_term_lufs", C.c_float), ("integrated_lufs", C.c_float), ("gating_above_absolute", C.c_uint32),
                ("gating_above_relative", C.c_uint32), ("valid", C.c_uint32)]


class CProgramInterval(C.Structure):
    """omx_program_interval (include/omx/program_timeline.h)"""
    _fields_ = [("stream", C.c_uint32), ("_pad", C.c_uint32), ("first_segment", C.c_uint64), ("segment_count", C.c_uint64)]


assert C.sizeof(CProgramTimelineRow) == 40 and C.sizeof(CProgramInterval) == 24 and C.sizeof(CProgramLoudnessRecord) == 168

# numpy views of the three structures (same layout: natural alignment, no padding but the named one)
TIMELINE_ROW_DTYPE = np.dtype([("integrated_energy", "<f8"), ("relative_threshold_energy", "<f8"), ("momentary_lufs", "<f4"),
                               ("short_term_lufs", "<f4"), ("integrated_lufs", "<f4"), ("gating_above_absolute", "<u4"),
                               ("gating_above_relative", "<u4"), ("valid", "<u4")])
INTERVAL_DTYPE = np.dtype([("stream", "<u4"), ("_pad", "<u4"), ("first_segment", "<u8"), ("segment_count", "<u8")])
RECORD_DTYPE = np.dtype([(n, "<f8") for n in _ENERGIES] + [(n, "<u8") for n in _COUNTS] + [(n, "<f4") for n in _LEVELS]
                        + [("overflow", "<u4"), ("_pad", "<u4")])
assert TIMELINE_ROW_DTYPE.itemsize == 40 and INTERVAL_DTYPE.itemsize == 24 and RECORD_DTYPE.itemsize == 168


class CProgramGroup(C.Structure):
    """omx_program_group (include/omx/program_groups.h): members[first_member : first_member + member_count]"""
    _fields_ = [("first_member", C.c_uint64), ("member_count", C.c_uint64)]


GROUP_DTYPE = np.dtype([("first_member", "<u8"), ("member_count", "<u8")])
TO_END = 2 ** 64 - 1   # OMX_PROGRAM_TO_END, as a member's segment_count: up to the stream's last stored segment
assert C.sizeof(CProgramGroup) == 16 and GROUP_DTYPE.itemsize == 16


class CProgramGainRule(C.Structure):
    """omx_program_gain_rule (include/omx/program_normalize.h)"""
    _fields_ = [("target_lufs", C.c_float), ("true_peak_ceiling_db", C.c_float), ("min_gain_db", C.c_float), ("max_gain_db", C.c_float),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramGainRecord(C.Structure):
    """omx_program_gain_record (include/omx/program_normalize.h)"""
    _fields_ = [("gain_db", C.c_float), ("gain", C.c_float), ("source_lufs", C.c_float), ("source_peak_db", C.c_float),
                ("predicted_lufs", C.c_float), ("predicted_peak_db", C.c_float), ("limited_by", C.c_uint32), ("peak_known", C.c_uint32)]


class CProgramApplyRecord(C.Structure):
    """omx_program_apply_record (include/omx/program_normalize.h)"""
    _fields_ = [("frames", C.c_uint64), ("samples_over", C.c_uint64), ("gain", C.c_float), ("out_sample_peak", C.c_float),
                ("out_sample_peak_db", C.c_float), ("gain_index", C.c_uint32)]


GAIN_RECORD_DTYPE = np.dtype([("gain_db", "<f4"), ("gain", "<f4"), ("source_lufs", "<f4"), ("source_peak_db", "<f4"),
                              ("predicted_lufs", "<f4"), ("predicted_peak_db", "<f4"), ("limited_by", "<u4"), ("peak_known", "<u4")])
APPLY_RECORD_DTYPE = np.dtype([("frames", "<u8"), ("samples_over", "<u8"), ("gain", "<f4"), ("out_sample_peak", "<f4"),
                               ("out_sample_peak_db", "<f4"), ("gain_index", "<u4")])
assert C.sizeof(CProgramGainRule) == 24 and C.sizeof(CProgramGainRecord) == 32 and C.sizeof(CProgramApplyRecord) == 32
assert GAIN_RECORD_DTYPE.itemsize == 32 and APPLY_RECORD_DTYPE.itemsize == 32
UNITY_GAIN = 2 ** 32 - 1   # OMX_PROGRAM_UNITY_GAIN, as a gain index of apply_gains: factor 1
GAIN_LIMIT_PEAK = 1        # GainRule.flags
GAIN_BY_TARGET, GAIN_BY_PEAK, GAIN_BY_MAX_GAIN, GAIN_BY_MIN_GAIN, GAIN_BY_NO_MEASUREMENT = 0, 1, 2, 3, 4


@dataclass
class GainRule:
    """omx_program_gain_rule: the target, the clamp and, with flags = GAIN_LIMIT_PEAK, the true-peak ceiling"""
    target_lufs: float = -23.0
    true_peak_ceiling_db: float = -1.0
    min_gain_db: float = -60.0
    max_gain_db: float = 60.0
    flags: int = 0

    def to_c(self) -> CProgramGainRule:
        return CProgramGainRule(self.target_lufs, self.true_peak_ceiling_db, self.min_gain_db, self.max_gain_db, self.flags, 0)


def evaluate_gain(api: Api, rule: GainRule, integrated_lufs: float, gating_above_relative: int, max_true_peak_db: float,
                  floor_db: float) -> np.ndarray:
    """The gain record the plan kernels write for these source values (omx_program_gain_evaluate), as a GAIN_RECORD_DTYPE scalar.
    Needs no device."""
    out = np.zeros((1,), GAIN_RECORD_DTYPE)
    c = rule.to_c()
    api.check(api.fn("program_gain_evaluate", C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_float, C.c_float, C.c_void_p])(
        C.byref(c), integrated_lufs, gating_above_relative, max_true_peak_db, floor_db, out.ctypes.data))
    return out[0]


# ---- include/omx/program_peak_timeline.h
_u32x8 = C.c_uint32 * 8


class CProgramPeakRow(C.Structure):
    """omx_program_peak_row (include/omx/program_peak_timeline.h)"""
    _fields_ = [("true_peak", _f32x8), ("sample_peak", _f32x8), ("true_peak_offset", _u32x8), ("sample_peak_offset", _u32x8),
                ("frames", C.c_uint32), ("valid", C.c_uint32)]


class CProgramPartPeak(C.Structure):
    """omx_program_part_peak (include/omx/program_peak_timeline.h)"""
    _fields_ = [("frames", C.c_uint64), ("true_peak_frame", _u64x8), ("sample_peak_frame", _u64x8), ("true_peak_member", _u32x8),
                ("sample_peak_member", _u32x8), ("true_peak", _f32x8), ("sample_peak", _f32x8), ("true_peak_db", _f32x8),
                ("sample_peak_db", _f32x8), ("max_true_peak_db", C.c_float), ("max_sample_peak_db", C.c_float),
                ("max_true_peak_channel", C.c_uint32), ("channels", C.c_uint32)]


PEAK_ROW_DTYPE = np.dtype([("true_peak", "<f4", (8,)), ("sample_peak", "<f4", (8,)), ("true_peak_offset", "<u4", (8,)),
                           ("sample_peak_offset", "<u4", (8,)), ("frames", "<u4"), ("valid", "<u4")])
PART_PEAK_DTYPE = np.dtype([("frames", "<u8"), ("true_peak_frame", "<u8", (8,)), ("sample_peak_frame", "<u8", (8,)),
                            ("true_peak_member", "<u4", (8,)), ("sample_peak_member", "<u4", (8,)), ("true_peak", "<f4", (8,)),
                            ("sample_peak", "<f4", (8,)), ("true_peak_db", "<f4", (8,)), ("sample_peak_db", "<f4", (8,)),
                            ("max_true_peak_db", "<f4"), ("max_sample_peak_db", "<f4"), ("max_true_peak_channel", "<u4"),
                            ("channels", "<u4")])
assert C.sizeof(CProgramPeakRow) == 136 and C.sizeof(CProgramPartPeak) == 344
assert PEAK_ROW_DTYPE.itemsize == 136 and PART_PEAK_DTYPE.itemsize == 344


class CProgramLimitRule(C.Structure):
    """omx_program_limit_rule (include/omx/program_limit.h)"""
    _fields_ = [("ceiling_db", C.c_float), ("attack_frames", C.c_uint32), ("release_hold_frames", C.c_uint32), ("flags", C.c_uint32)]


class CProgramLimitRecord(C.Structure):
    """omx_program_limit_record (include/omx/program_limit.h)"""
    _fields_ = [("frames_in", C.c_uint64), ("frames_out", C.c_uint64), ("frames_written", C.c_uint64), ("frames_limited", C.c_uint64),
                ("samples_over", C.c_uint64), ("gain", C.c_float), ("ceiling", C.c_float), ("min_envelope", C.c_float),
                ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float), ("max_reduction_db", C.c_float),
                ("gain_index", C.c_uint32), ("state", C.c_uint32), ("latency_frames", C.c_uint32), ("_pad", C.c_uint32)]


LIMIT_RECORD_DTYPE = np.dtype([("frames_in", "<u8"), ("frames_out", "<u8"), ("frames_written", "<u8"), ("frames_limited", "<u8"),
                               ("samples_over", "<u8"), ("gain", "<f4"), ("ceiling", "<f4"), ("min_envelope", "<f4"),
                               ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("max_reduction_db", "<f4"),
                               ("gain_index", "<u4"), ("state", "<u4"), ("latency_frames", "<u4"), ("_pad", "<u4")])
assert C.sizeof(CProgramLimitRule) == 16 and C.sizeof(CProgramLimitRecord) == 80 and LIMIT_RECORD_DTYPE.itemsize == 80
LIMIT_IDLE, LIMIT_RUNNING, LIMIT_FLUSHED = 0, 1, 2   # omx_program_limit_record.state


@dataclass
class LimitRule:
    """omx_program_limit_rule: the true-peak ceiling, the attack (look-ahead) and the hold before the release, in frames"""
    ceiling_db: float = -1.0
    attack_frames: int = 64
    release_hold_frames: int = 0
    flags: int = 0

    def to_c(self) -> CProgramLimitRule:
        return CProgramLimitRule(self.ceiling_db, self.attack_frames, self.release_hold_frames, self.flags)


def limit_latency(api: Api, rule: LimitRule) -> int:
    """Frames by which the limiter's output trails its input (omx_program_limit_latency): attack_frames + 23.  Needs no device."""
    out, c = C.c_uint32(), rule.to_c()
    api.check(api.fn("program_limit_latency", C.c_int, [C.c_void_p, C.c_void_p])(C.byref(c), C.byref(out)))
    return int(out.value)


class CProgramExportRule(C.Structure):
    """omx_program_export_rule (include/omx/program_pcm.h)"""
    _fields_ = [("format", C.c_uint32), ("dither", C.c_uint32), ("seed", C.c_uint64), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramExportRecord(C.Structure):
    """omx_program_export_record (include/omx/program_pcm.h)"""
    _fields_ = [("frames_out", C.c_uint64), ("frames_written", C.c_uint64), ("samples_clipped", C.c_uint64), ("samples_nan", C.c_uint64),
                ("out_peak", C.c_uint32), ("out_peak_db", C.c_float), ("format", C.c_uint32), ("dither", C.c_uint32)]


EXPORT_RECORD_DTYPE = np.dtype([("frames_out", "<u8"), ("frames_written", "<u8"), ("samples_clipped", "<u8"), ("samples_nan", "<u8"),
                                ("out_peak", "<u4"), ("out_peak_db", "<f4"), ("format", "<u4"), ("dither", "<u4")])
assert C.sizeof(CProgramExportRule) == 24 and C.sizeof(CProgramExportRecord) == 48 and EXPORT_RECORD_DTYPE.itemsize == 48
PCM_S16, PCM_S24, PCM_S32 = 1, 2, 3     # OMX_PCM_*: 2, 3 (packed) and 4 bytes per sample, little-endian, interleaved
DITHER_NONE, DITHER_TPDF = 0, 1         # OMX_DITHER_*


@dataclass
class ExportRule:
    """omx_program_export_rule: the integer format, the dither and its seed"""
    format: int = PCM_S16
    dither: int = DITHER_TPDF
    seed: int = 0
    flags: int = 0

    def to_c(self) -> CProgramExportRule:
        return CProgramExportRule(self.format, self.dither, self.seed, self.flags, 0)


def pcm_format_bytes(api: Api, format: int) -> int:
    """Bytes per sample of a PCM_* format (omx_pcm_format_bytes).  Needs no device."""
    out = C.c_uint32()
    api.check(api.fn("pcm_format_bytes", C.c_int, [C.c_uint32, C.c_void_p])(format, C.byref(out)))
    return int(out.value)


def dither_value(api: Api, rule: ExportRule, stream: int, frame: int, channel: int) -> float:
    """The dither, in LSB, that the export adds to (stream, absolute frame, channel) under `rule` (omx_program_dither_evaluate): the
    function the kernel runs.  Needs no device."""
    out, c = C.c_double(), rule.to_c()
    api.check(api.fn("program_dither_evaluate", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])(
        C.byref(c), stream, frame, channel, C.byref(out)))
    return float(out.value)


class CProgramResampleRule(C.Structure):
    """omx_program_resample_rule (include/omx/program_resample.h)"""
    _fields_ = [("rate_in", C.c_uint32), ("rate_out", C.c_uint32), ("half_width", C.c_uint32), ("beta", C.c_float), ("cutoff", C.c_float),
                ("flags", C.c_uint32)]


class CProgramResampleInfo(C.Structure):
    """omx_program_resample_info (include/omx/program_resample.h)"""
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("taps", C.c_uint32), ("latency_frames", C.c_uint32), ("table_floats", C.c_uint64),
                ("tile_frames", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramResampleRecord(C.Structure):
    """omx_program_resample_record (include/omx/program_resample.h)"""
    _fields_ = [("frames_in", C.c_uint64), ("frames_out", C.c_uint64), ("frames_written", C.c_uint64), ("samples_over", C.c_uint64),
                ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float), ("state", C.c_uint32), ("L", C.c_uint32),
                ("M", C.c_uint32), ("taps", C.c_uint32), ("latency_frames", C.c_uint32), ("_pad", C.c_uint32)]


RESAMPLE_INFO_DTYPE = np.dtype([("L", "<u4"), ("M", "<u4"), ("taps", "<u4"), ("latency_frames", "<u4"), ("table_floats", "<u8"),
                                ("tile_frames", "<u4"), ("_pad", "<u4")])
RESAMPLE_RECORD_DTYPE = np.dtype([("frames_in", "<u8"), ("frames_out", "<u8"), ("frames_written", "<u8"), ("samples_over", "<u8"),
                                  ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("state", "<u4"), ("L", "<u4"), ("M", "<u4"),
                                  ("taps", "<u4"), ("latency_frames", "<u4"), ("_pad", "<u4")])
assert C.sizeof(CProgramResampleRule) == 24 and C.sizeof(CProgramResampleInfo) == 32 and C.sizeof(CProgramResampleRecord) == 64
assert RESAMPLE_INFO_DTYPE.itemsize == 32 and RESAMPLE_RECORD_DTYPE.itemsize == 64
RESAMPLE_IDLE, RESAMPLE_RUNNING, RESAMPLE_FLUSHED = 0, 1, 2   # omx_program_resample_record.state


@dataclass
class ResampleRule:
    """omx_program_resample_rule: the two rates in whole Hz, the filter's half width in zero crossings, Kaiser beta and the -6 dB
    point as a fraction of the narrower Nyquist; the defaults are the header's"""
    rate_in: int = 44100
    rate_out: int = 48000
    half_width: int = 32
    beta: float = 12.0
    cutoff: float = 0.94
    flags: int = 0

    def to_c(self) -> CProgramResampleRule:
        return CProgramResampleRule(self.rate_in, self.rate_out, self.half_width, self.beta, self.cutoff, self.flags)


def resample_plan(api: Api, rule: ResampleRule) -> np.ndarray:
    """The plan of `rule` (omx_program_resample_plan) as a RESAMPLE_INFO_DTYPE scalar: L, M, taps per phase, the latency H in input
    frames, the table's size in floats and the main kernel's tile in output frames.  Needs no device."""
    out, c = np.zeros((1,), RESAMPLE_INFO_DTYPE), rule.to_c()
    api.check(api.fn("program_resample_plan", C.c_int, [C.c_void_p, C.c_void_p])(C.byref(c), out.ctypes.data))
    return out[0]


def resample_taps(api: Api, rule: ResampleRule) -> np.ndarray:
    """The f32 table [L][taps] the kernel uses under `rule` (omx_program_resample_taps).  Needs no device."""
    info, c = resample_plan(api, rule), rule.to_c()
    out = np.zeros((int(info["L"]), int(info["taps"])), np.float32)
    api.check(api.fn("program_resample_taps", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64])(C.byref(c), out.ctypes.data, out.size))
    return out


def resample_frames(api: Api, rule: ResampleRule, frames_in_before: int, frames_out_before: int, frames: int, flush: bool = False) -> int:
    """Frames a stream emits in a call that brings `frames` frames, after frames_in_before taken and frames_out_before emitted
    (omx_program_resample_frames): what d_out has to hold.  Needs no device."""
    out, c = C.c_uint64(), rule.to_c()
    api.check(api.fn("program_resample_frames", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])(
        C.byref(c), frames_in_before, frames_out_before, frames, 1 if flush else 0, C.byref(out)))
    return int(out.value)


class CProgramRemixInfo(C.Structure):
    """omx_program_remix_info (include/omx/program_remix.h)"""
    _fields_ = [("tile_frames", C.c_uint32), ("channels_in", C.c_uint32), ("channels_out", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramDownmixRule(C.Structure):
    """omx_program_downmix_rule (include/omx/program_remix.h)"""
    _fields_ = [("kind", C.c_uint32), ("center_level", C.c_float), ("surround_level", C.c_float), ("lfe_level", C.c_float),
                ("flags", C.c_uint32)]


class CProgramRemixRecord(C.Structure):
    """omx_program_remix_record (include/omx/program_remix.h)"""
    _fields_ = [("frames", C.c_uint64), ("samples_over", C.c_uint64), ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float),
                ("matrix_index", C.c_uint32), ("terms", C.c_uint32)]


REMIX_INFO_DTYPE = np.dtype([("tile_frames", "<u4"), ("channels_in", "<u4"), ("channels_out", "<u4"), ("_pad", "<u4")])
REMIX_RECORD_DTYPE = np.dtype([("frames", "<u8"), ("samples_over", "<u8"), ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"),
                               ("matrix_index", "<u4"), ("terms", "<u4")])
assert C.sizeof(CProgramRemixInfo) == 16 and C.sizeof(CProgramDownmixRule) == 20 and C.sizeof(CProgramRemixRecord) == 32
assert REMIX_INFO_DTYPE.itemsize == 16 and REMIX_RECORD_DTYPE.itemsize == 32
REMIX_MAX_MATRICES = 65536
REMIX_KIND_STEREO, REMIX_KIND_MONO = 0, 1   # omx_program_downmix_rule.kind
REMIX_NORMALIZE = 1                          # omx_program_downmix_rule.flags


@dataclass
class DownmixRule:
    """omx_program_downmix_rule: the kind of fold-down (REMIX_KIND_STEREO: Lo/Ro, REMIX_KIND_MONO: its mono fold), the levels of the
    centre, the surrounds and the LFE, and REMIX_NORMALIZE or 0; the defaults are the header's"""
    kind: int = REMIX_KIND_STEREO
    center_level: float = 0.70710678
    surround_level: float = 0.70710678
    lfe_level: float = 0.0
    flags: int = 0

    def to_c(self) -> CProgramDownmixRule:
        return CProgramDownmixRule(self.kind, self.center_level, self.surround_level, self.lfe_level, self.flags)


def remix_plan(api: Api, channels_in: int, channels_out: int) -> np.ndarray:
    """The plan of a channel pair (omx_program_remix_plan) as a REMIX_INFO_DTYPE scalar: the main kernel's tile in frames.  Needs no
    device."""
    out = np.zeros((1,), REMIX_INFO_DTYPE)
    api.check(api.fn("program_remix_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p])(channels_in, channels_out, out.ctypes.data))
    return out[0]


def remix_downmix(api: Api, rule: DownmixRule, channels_in: int, positions_in: Sequence[int]):
    """The fold-down of a layout given as positions (omx_program_remix_downmix) -> (matrix f32 [channels_out][channels_in], positions_out
    as a list of 8).  Needs no device."""
    c, pos = rule.to_c(), _u8x8(*(list(positions_in) + [capi.POS_UNKNOWN] * 8)[:8])
    matrix, n_out, pos_out = np.zeros((2 * 8,), np.float32), C.c_uint32(), _u8x8()
    api.check(api.fn("program_remix_downmix", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])(
        C.byref(c), channels_in, pos, matrix.ctypes.data, C.byref(n_out), pos_out))
    return matrix[:n_out.value * channels_in].reshape(n_out.value, channels_in).copy(), list(pos_out)


def remix_select(api: Api, channels_in: int, positions_in: Sequence[int], channels_out: int, positions_out: Sequence[int]):
    """The matrix that gives every output position the first input channel of that position (omx_program_remix_select) ->
    (matrix f32 [channels_out][channels_in], the mask of the outputs without a source).  Needs no device."""
    pos_in = _u8x8(*(list(positions_in) + [capi.POS_UNKNOWN] * 8)[:8])
    pos_out = _u8x8(*(list(positions_out) + [capi.POS_UNKNOWN] * 8)[:8])
    matrix, missing = np.zeros((8 * 8,), np.float32), C.c_uint32()
    api.check(api.fn("program_remix_select", C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])(
        channels_in, pos_in, channels_out, pos_out, matrix.ctypes.data, C.byref(missing)))
    return matrix[:channels_out * channels_in].reshape(channels_out, channels_in).copy(), int(missing.value)


class CProgramInspectRule(C.Structure):
    """omx_program_inspect_rule (include/omx/program_inspect.h)"""
    _fields_ = [("clip_level", C.c_float), ("clip_min_run", C.c_uint32), ("silence_level", C.c_float), ("silence_min_run", C.c_uint32),
                ("dc_limit", C.c_float), ("correlation_min", C.c_float), ("flags", C.c_uint32)]


class CProgramInspectInfo(C.Structure):
    """omx_program_inspect_info (include/omx/program_inspect.h)"""
    _fields_ = [("tile_frames", C.c_uint32), ("channels", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class CProgramInspectChannel(C.Structure):
    """omx_program_inspect_channel (include/omx/program_inspect.h)"""
    _fields_ = [("dc_sum", C.c_int64), ("nan_samples", C.c_uint64), ("clipped_samples", C.c_uint64), ("clip_runs", C.c_uint64),
                ("longest_clip_run", C.c_uint64), ("longest_clip_start", C.c_uint64), ("open_clip_run", C.c_uint64), ("_pad", C.c_uint64)]


class CProgramInspectPair(C.Structure):
    """omx_program_inspect_pair (include/omx/program_inspect.h)"""
    _fields_ = [("sum_ab", C.c_int64), ("sum_aa", C.c_uint64), ("sum_bb", C.c_uint64), ("a", C.c_uint32), ("b", C.c_uint32)]


INSPECT_MAX_PAIRS = 4


class CProgramInspectRecord(C.Structure):
    """omx_program_inspect_record (include/omx/program_inspect.h)"""
    _fields_ = [("frames", C.c_uint64), ("silent_frames", C.c_uint64), ("silent_runs", C.c_uint64), ("longest_silent_run", C.c_uint64),
                ("longest_silent_start", C.c_uint64), ("leading_silence", C.c_uint64), ("trailing_silence", C.c_uint64),
                ("channels", C.c_uint32), ("n_pairs", C.c_uint32), ("channel", CProgramInspectChannel * 8),
                ("pair", CProgramInspectPair * INSPECT_MAX_PAIRS)]


class CProgramInspectSummary(C.Structure):
    """omx_program_inspect_summary (include/omx/program_inspect.h)"""
    _fields_ = [("verdict", C.c_uint32), ("channels", C.c_uint32), ("n_pairs", C.c_uint32), ("_pad", C.c_uint32),
                ("interior_silent_runs", C.c_uint64), ("dc_offset", C.c_float * 8), ("dc_offset_db", C.c_float * 8),
                ("correlation", C.c_float * INSPECT_MAX_PAIRS), ("correlation_valid", C.c_uint32 * INSPECT_MAX_PAIRS)]


INSPECT_INFO_DTYPE = np.dtype([("tile_frames", "<u4"), ("channels", "<u4"), ("_pad", "<u4", (2,))])
INSPECT_CHANNEL_DTYPE = np.dtype([("dc_sum", "<i8"), ("nan_samples", "<u8"), ("clipped_samples", "<u8"), ("clip_runs", "<u8"),
                                  ("longest_clip_run", "<u8"), ("longest_clip_start", "<u8"), ("open_clip_run", "<u8"), ("_pad", "<u8")])
INSPECT_PAIR_DTYPE = np.dtype([("sum_ab", "<i8"), ("sum_aa", "<u8"), ("sum_bb", "<u8"), ("a", "<u4"), ("b", "<u4")])
INSPECT_RECORD_DTYPE = np.dtype([("frames", "<u8"), ("silent_frames", "<u8"), ("silent_runs", "<u8"), ("longest_silent_run", "<u8"),
                                 ("longest_silent_start", "<u8"), ("leading_silence", "<u8"), ("trailing_silence", "<u8"),
                                 ("channels", "<u4"), ("n_pairs", "<u4"), ("channel", INSPECT_CHANNEL_DTYPE, (8,)),
                                 ("pair", INSPECT_PAIR_DTYPE, (INSPECT_MAX_PAIRS,))])
INSPECT_SUMMARY_DTYPE = np.dtype([("verdict", "<u4"), ("channels", "<u4"), ("n_pairs", "<u4"), ("_pad", "<u4"),
                                  ("interior_silent_runs", "<u8"), ("dc_offset", "<f4", (8,)), ("dc_offset_db", "<f4", (8,)),
                                  ("correlation", "<f4", (INSPECT_MAX_PAIRS,)), ("correlation_valid", "<u4", (INSPECT_MAX_PAIRS,))])
assert C.sizeof(CProgramInspectRule) == 28 and C.sizeof(CProgramInspectInfo) == 16 and C.sizeof(CProgramInspectChannel) == 64
assert C.sizeof(CProgramInspectPair) == 32 and C.sizeof(CProgramInspectRecord) == 704 and C.sizeof(CProgramInspectSummary) == 120
assert INSPECT_INFO_DTYPE.itemsize == 16 and INSPECT_RECORD_DTYPE.itemsize == 704 and INSPECT_SUMMARY_DTYPE.itemsize == 120
# omx_program_inspect_summary.verdict
INSPECT_NAN, INSPECT_CLIPPED, INSPECT_DROPOUT, INSPECT_ALL_SILENT, INSPECT_DC, INSPECT_ANTIPHASE = 1, 2, 4, 8, 16, 32
INSPECT_DB_FLOOR = -400.0


@dataclass
class InspectRule:
    """omx_program_inspect_rule: a sample is hot at |x| >= clip_level and clip_min_run hot samples in a row are a clipping run; a frame
    is quiet when every channel has |x| <= silence_level and silence_min_run quiet frames in a row are a silent run; the summary flags
    a DC offset above dc_limit and a pair whose correlation lies below correlation_min.  The defaults are the header's."""
    clip_level: float = 0.99996948
    clip_min_run: int = 3
    silence_level: float = 0.0
    silence_min_run: int = 480
    dc_limit: float = 1e-3
    correlation_min: float = -0.2
    flags: int = 0

    def to_c(self) -> CProgramInspectRule:
        return CProgramInspectRule(self.clip_level, self.clip_min_run, self.silence_level, self.silence_min_run, self.dc_limit,
                                   self.correlation_min, self.flags)


def inspect_rule_default(api: Api) -> InspectRule:
    """The header's defaults as the library fills them (omx_program_inspect_rule_default).  Needs no device."""
    c = CProgramInspectRule()
    api.check(api.fn("program_inspect_rule_default", C.c_int, [C.c_void_p])(C.byref(c)))
    return InspectRule(c.clip_level, c.clip_min_run, c.silence_level, c.silence_min_run, c.dc_limit, c.correlation_min, c.flags)


def inspect_plan(api: Api, channels: int) -> np.ndarray:
    """The plan of a channel count (omx_program_inspect_plan) as an INSPECT_INFO_DTYPE scalar: the main kernel's tile in frames.  Needs
    no device."""
    out = np.zeros((1,), INSPECT_INFO_DTYPE)
    api.check(api.fn("program_inspect_plan", C.c_int, [C.c_uint32, C.c_void_p])(channels, out.ctypes.data))
    return out[0]


def inspect_summarize(api: Api, rule: InspectRule, record: np.ndarray) -> np.ndarray:
    """The figures a person reads from one INSPECT_RECORD_DTYPE record (omx_program_inspect_summarize) as an INSPECT_SUMMARY_DTYPE
    scalar: DC offsets, pair correlations, interior silent runs and the verdict bits (INSPECT_*).  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(record, INSPECT_RECORD_DTYPE).reshape(1))
    out, c = np.zeros((1,), INSPECT_SUMMARY_DTYPE), rule.to_c()
    api.check(api.fn("program_inspect_summarize", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])(C.byref(c), rec.ctypes.data, out.ctypes.data))
    return out[0]


class CProgramEditClip(C.Structure):
    """omx_program_edit_clip (include/omx/program_edit.h)"""
    _fields_ = [("src_stream", C.c_uint32), ("dst_stream", C.c_uint32), ("src_first", C.c_uint64), ("dst_first", C.c_uint64),
                ("frames", C.c_uint64), ("fade_in_frames", C.c_uint32), ("fade_out_frames", C.c_uint32), ("fade_in_curve", C.c_uint8),
                ("fade_out_curve", C.c_uint8), ("flags", C.c_uint16), ("gain", C.c_float)]


class CProgramEditInfo(C.Structure):
    """omx_program_edit_info (include/omx/program_edit.h)"""
    _fields_ = [("tile_frames", C.c_uint32), ("channels", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class CProgramTrimRule(C.Structure):
    """omx_program_trim_rule (include/omx/program_edit.h)"""
    _fields_ = [("keep_head", C.c_uint64), ("keep_tail", C.c_uint64), ("pad_head", C.c_uint64), ("pad_tail", C.c_uint64),
                ("fade_in_frames", C.c_uint32), ("fade_out_frames", C.c_uint32), ("fade_in_curve", C.c_uint8), ("fade_out_curve", C.c_uint8),
                ("flags", C.c_uint16), ("_pad", C.c_uint32)]


class CProgramEditRecord(C.Structure):
    """omx_program_edit_record (include/omx/program_edit.h)"""
    _fields_ = [("out_first", C.c_uint64), ("frames", C.c_uint64), ("silent_frames", C.c_uint64), ("faded_frames", C.c_uint64),
                ("mixed_frames", C.c_uint64), ("samples_over", C.c_uint64), ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float),
                ("clips", C.c_uint32), ("_pad", C.c_uint32)]


EDIT_CLIP_DTYPE = np.dtype([("src_stream", "<u4"), ("dst_stream", "<u4"), ("src_first", "<u8"), ("dst_first", "<u8"), ("frames", "<u8"),
                            ("fade_in_frames", "<u4"), ("fade_out_frames", "<u4"), ("fade_in_curve", "u1"), ("fade_out_curve", "u1"),
                            ("flags", "<u2"), ("gain", "<f4")])
EDIT_INFO_DTYPE = np.dtype([("tile_frames", "<u4"), ("channels", "<u4"), ("_pad", "<u4", (2,))])
EDIT_RECORD_DTYPE = np.dtype([("out_first", "<u8"), ("frames", "<u8"), ("silent_frames", "<u8"), ("faded_frames", "<u8"),
                              ("mixed_frames", "<u8"), ("samples_over", "<u8"), ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"),
                              ("clips", "<u4"), ("_pad", "<u4")])
assert C.sizeof(CProgramEditClip) == 48 and C.sizeof(CProgramEditInfo) == 16 and C.sizeof(CProgramTrimRule) == 48
assert C.sizeof(CProgramEditRecord) == 64
assert EDIT_CLIP_DTYPE.itemsize == 48 and EDIT_INFO_DTYPE.itemsize == 16 and EDIT_RECORD_DTYPE.itemsize == 64
EDIT_CURVE_LINEAR, EDIT_CURVE_EQUAL_POWER, EDIT_CURVE_RAISED_COSINE = 0, 1, 2   # omx_program_edit_clip.fade_*_curve
EDIT_CURVE_POINTS = 4097
EDIT_MAX_FADE = 1 << 24
EDIT_MAX_OUTPUTS = 1 << 24
EDIT_MAX_POSITION = 1 << 40


@dataclass
class EditClip:
    """omx_program_edit_clip: source frames [src_first, src_first + frames) of input stream src_stream land at output frames
    [dst_first, dst_first + frames) of output stream dst_stream, times gain, under a fade-in and a fade-out (EDIT_CURVE_*)"""
    src_stream: int = 0
    dst_stream: int = 0
    src_first: int = 0
    dst_first: int = 0
    frames: int = 0
    fade_in_frames: int = 0
    fade_out_frames: int = 0
    fade_in_curve: int = EDIT_CURVE_LINEAR
    fade_out_curve: int = EDIT_CURVE_LINEAR
    flags: int = 0
    gain: float = 1.0

    def to_row(self) -> tuple:
        return (self.src_stream, self.dst_stream, self.src_first, self.dst_first, self.frames, self.fade_in_frames, self.fade_out_frames,
                self.fade_in_curve, self.fade_out_curve, self.flags, self.gain)


def edit_table(clips) -> np.ndarray:
    """A clip table as a contiguous EDIT_CLIP_DTYPE array, from a sequence of EditClip or from such an array"""
    if isinstance(clips, np.ndarray):
        return np.ascontiguousarray(clips, EDIT_CLIP_DTYPE).reshape(-1)
    return np.array([c.to_row() for c in clips], EDIT_CLIP_DTYPE).reshape(-1)


@dataclass
class TrimRule:
    """omx_program_trim_rule: frames of the found silence to keep in front and behind, frames of exact zero to put in front and
    behind, and the fades of the cut (clamped to the kept length)"""
    keep_head: int = 0
    keep_tail: int = 0
    pad_head: int = 0
    pad_tail: int = 0
    fade_in_frames: int = 0
    fade_out_frames: int = 0
    fade_in_curve: int = EDIT_CURVE_LINEAR
    fade_out_curve: int = EDIT_CURVE_LINEAR
    flags: int = 0

    def to_c(self) -> CProgramTrimRule:
        return CProgramTrimRule(self.keep_head, self.keep_tail, self.pad_head, self.pad_tail, self.fade_in_frames, self.fade_out_frames,
                                self.fade_in_curve, self.fade_out_curve, self.flags, 0)


def edit_plan(api: Api, channels: int) -> np.ndarray:
    """The plan of a channel count (omx_program_edit_plan) as an EDIT_INFO_DTYPE scalar: the main kernel's tile in output frames.
    Needs no device."""
    out = np.zeros((1,), EDIT_INFO_DTYPE)
    api.check(api.fn("program_edit_plan", C.c_int, [C.c_uint32, C.c_void_p])(channels, out.ctypes.data))
    return out[0]


def edit_curve(api: Api, curve: int) -> np.ndarray:
    """The table of a fade curve (omx_program_edit_curve): f32 [4097].  Needs no device."""
    out = np.zeros((EDIT_CURVE_POINTS,), np.float32)
    api.check(api.fn("program_edit_curve", C.c_int, [C.c_uint32, C.c_void_p])(curve, out.ctypes.data))
    return out


def edit_gain(api: Api, curve: int, fade_frames: int, index: int) -> np.float32:
    """The fade factor at `index` of a fade of `fade_frames` frames (omx_program_edit_gain), by the function the kernel runs.  Needs
    no device."""
    out = C.c_float()
    api.check(api.fn("program_edit_gain", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])(curve, fade_frames, index, C.byref(out)))
    return np.float32(out.value)


def edit_extent(api: Api, clips, frames_in: Sequence[int], n_out: int) -> np.ndarray:
    """Validate a clip table against the frames of the input streams (omx_program_edit_extent) -> uint64 [n_out]: one past the last
    covered frame of every output stream.  Needs no device."""
    table = edit_table(clips)
    fr = np.ascontiguousarray(frames_in, np.uint32).reshape(-1)
    out = np.zeros((n_out,), np.uint64)
    api.check(api.fn("program_edit_extent", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])(
        table.ctypes.data if table.size else None, table.size, fr.size, fr.ctypes.data if fr.size else None, n_out,
        out.ctypes.data if n_out else None))
    return out


def edit_trim(api: Api, record: np.ndarray, rule: TrimRule, src_stream: int = 0, dst_stream: int = 0):
    """The clip that cuts a stream where inspect found silence (omx_program_edit_trim), from one INSPECT_RECORD_DTYPE record ->
    (EditClip, the frames of the output: pad_head + the clip + pad_tail).  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(record, INSPECT_RECORD_DTYPE).reshape(1))
    c, clip, total = rule.to_c(), np.zeros((1,), EDIT_CLIP_DTYPE), C.c_uint64()
    api.check(api.fn("program_edit_trim", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])(
        rec.ctypes.data, C.byref(c), src_stream, dst_stream, clip.ctypes.data, C.byref(total)))
    row = clip[0]
    return EditClip(*[int(row[f]) for f in EDIT_CLIP_DTYPE.names[:-1]], float(row["gain"])), int(total.value)


class CProgramMixSend(C.Structure):
    """omx_program_mix_send (include/omx/program_mix.h)"""
    _fields_ = [("src_stream", C.c_uint32), ("dst_bus", C.c_uint32), ("src_first", C.c_uint64), ("dst_first", C.c_uint64),
                ("frames", C.c_uint64), ("gain", C.c_float), ("flags", C.c_uint32)]


class CProgramMixInfo(C.Structure):
    """omx_program_mix_info (include/omx/program_mix.h)"""
    _fields_ = [("tile_frames", C.c_uint32), ("layers_per_batch", C.c_uint32), ("channels", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramMixRecord(C.Structure):
    """omx_program_mix_record (include/omx/program_mix.h)"""
    _fields_ = [("out_first", C.c_uint64), ("frames", C.c_uint64), ("silent_frames", C.c_uint64), ("mixed_frames", C.c_uint64),
                ("samples_over", C.c_uint64), ("samples_nonfinite", C.c_uint64), ("out_sample_peak", C.c_float),
                ("out_sample_peak_db", C.c_float), ("sends", C.c_uint32), ("max_layers", C.c_uint32)]


MIX_SEND_DTYPE = np.dtype([("src_stream", "<u4"), ("dst_bus", "<u4"), ("src_first", "<u8"), ("dst_first", "<u8"), ("frames", "<u8"),
                           ("gain", "<f4"), ("flags", "<u4")])
MIX_INFO_DTYPE = np.dtype([("tile_frames", "<u4"), ("layers_per_batch", "<u4"), ("channels", "<u4"), ("_pad", "<u4")])
MIX_RECORD_DTYPE = np.dtype([("out_first", "<u8"), ("frames", "<u8"), ("silent_frames", "<u8"), ("mixed_frames", "<u8"),
                             ("samples_over", "<u8"), ("samples_nonfinite", "<u8"), ("out_sample_peak", "<f4"),
                             ("out_sample_peak_db", "<f4"), ("sends", "<u4"), ("max_layers", "<u4")])
assert C.sizeof(CProgramMixSend) == 40 and C.sizeof(CProgramMixInfo) == 16 and C.sizeof(CProgramMixRecord) == 64
assert MIX_SEND_DTYPE.itemsize == 40 and MIX_INFO_DTYPE.itemsize == 16 and MIX_RECORD_DTYPE.itemsize == 64
MIX_MAX_LAYERS = 64
MIX_MAX_SENDS = 1 << 20
MIX_MAX_BUSES = 1 << 24
MIX_MAX_POSITION = 1 << 40


@dataclass
class MixSend:
    """omx_program_mix_send: source frames [src_first, src_first + frames) of input stream src_stream land at frames
    [dst_first, dst_first + frames) of bus dst_bus, times gain (negative: inverted polarity)"""
    src_stream: int = 0
    dst_bus: int = 0
    src_first: int = 0
    dst_first: int = 0
    frames: int = 0
    gain: float = 1.0
    flags: int = 0

    def to_row(self) -> tuple:
        return (self.src_stream, self.dst_bus, self.src_first, self.dst_first, self.frames, self.gain, self.flags)


def mix_table(sends) -> np.ndarray:
    """A send table as a contiguous MIX_SEND_DTYPE array, from a sequence of MixSend or from such an array"""
    if isinstance(sends, np.ndarray):
        return np.ascontiguousarray(sends, MIX_SEND_DTYPE).reshape(-1)
    return np.array([s.to_row() for s in sends], MIX_SEND_DTYPE).reshape(-1)


def mix_plan(api: Api, channels: int) -> np.ndarray:
    """The plan of a channel count (omx_program_mix_plan) as a MIX_INFO_DTYPE scalar: the main kernel's tile in bus frames and the
    layers whose loads it keeps in flight together.  Needs no device."""
    out = np.zeros((1,), MIX_INFO_DTYPE)
    api.check(api.fn("program_mix_plan", C.c_int, [C.c_uint32, C.c_void_p])(channels, out.ctypes.data))
    return out[0]


def mix_extent(api: Api, sends, frames_in: Sequence[int], n_out: int) -> np.ndarray:
    """Validate a send table against the frames of the input streams (omx_program_mix_extent) -> uint64 [n_out]: one past the last
    covered frame of every bus.  Needs no device."""
    table = mix_table(sends)
    fr = np.ascontiguousarray(frames_in, np.uint32).reshape(-1)
    out = np.zeros((n_out,), np.uint64)
    api.check(api.fn("program_mix_extent", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])(
        table.ctypes.data if table.size else None, table.size, fr.size, fr.ctypes.data if fr.size else None, n_out,
        out.ctypes.data if n_out else None))
    return out


def mix_null(api: Api, stems: Sequence[int], reference_stream: int, frames: int, bus: int = 0) -> np.ndarray:
    """The table of a null test (omx_program_mix_null) as a MIX_SEND_DTYPE array: every stem at +1, then the reference at -1, over
    frames [0, frames) of `bus`.  Needs no device."""
    st = np.ascontiguousarray(stems, np.uint32).reshape(-1)
    out = np.zeros((st.size + 1,), MIX_SEND_DTYPE)
    api.check(api.fn("program_mix_null", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p])(
        st.ctypes.data if st.size else None, st.size, reference_stream, frames, bus, out.ctypes.data))
    return out


HISTOGRAM_BINS, HISTOGRAM_TAIL = 1000, 29
_u64xbins, _f64xbins = C.c_uint64 * HISTOGRAM_BINS, C.c_double * HISTOGRAM_BINS


class CProgramHistogram(C.Structure):
    """omx_program_histogram (include/omx/program_histogram.h)"""
    _fields_ = [("gating_count", _u64xbins), ("gating_sum", _f64xbins), ("short_term_count", _u64xbins), ("short_term_sum", _f64xbins),
                ("tail", C.c_double * HISTOGRAM_TAIL), ("segments", C.c_uint64), ("tail_count", C.c_uint32), ("_pad", C.c_uint32)]


assert C.sizeof(CProgramHistogram) == 32248


@dataclass
class ProgramHistogram:
    """omx_program_histogram: what a stream of a bank with bounded storage keeps instead of its segments"""
    gating_count: np.ndarray       # uint64[1000]
    gating_sum: np.ndarray         # float64[1000]: sum of the block energies binned there
    short_term_count: np.ndarray
    short_term_sum: np.ndarray
    tail: np.ndarray               # float64[tail_count]: the newest segment energies, oldest first
    segments: int

    def tobytes(self) -> bytes:
        """every field, bit for bit"""
        return b"".join([self.gating_count.tobytes(), self.gating_sum.tobytes(), self.short_term_count.tobytes(),
                         self.short_term_sum.tobytes(), self.tail.tobytes(), np.uint64(self.segments).tobytes()])


def histogram_boundaries(api: Api) -> np.ndarray:
    """B[0 .. 1000] of include/omx/program_histogram.h: bin i is (B[i], B[i + 1]], B[0] the absolute gate.  Needs no device."""
    out = np.zeros((HISTOGRAM_BINS + 1,), np.float64)
    api.check(api.fn("program_histogram_boundaries", C.c_int, [C.c_void_p])(out.ctypes.data))
    return out


FORM_BY_SHAPE, FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL = 0, 1, 2


class CProgramFilterSection(C.Structure):
    """omx_program_filter_section (include/omx/program_filter.h)"""
    _fields_ = [("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("a1", C.c_double), ("a2", C.c_double)]


FILTER_MAX_SECTIONS = 2
FILTER_MAX_FILTERS = 256
FILTER_BYPASS = 0xFFFFFFFF
# omx_program_filter_spec.kind
(FILTER_HIGHPASS, FILTER_LOWPASS, FILTER_LOW_SHELF, FILTER_HIGH_SHELF, FILTER_PEAKING, FILTER_NOTCH, FILTER_DC_BLOCK, FILTER_DEEMPHASIS,
 FILTER_PREEMPHASIS) = range(9)


class CProgramFilter(C.Structure):
    """omx_program_filter (include/omx/program_filter.h)"""
    _fields_ = [("n_sections", C.c_uint32), ("_pad", C.c_uint32), ("section", CProgramFilterSection * FILTER_MAX_SECTIONS)]


class CProgramFilterSpec(C.Structure):
    """omx_program_filter_spec (include/omx/program_filter.h)"""
    _fields_ = [("kind", C.c_uint32), ("order", C.c_uint32), ("frequency_hz", C.c_double), ("q", C.c_double), ("gain_db", C.c_double),
                ("time_constant_us", C.c_double), ("time_constant_zero_us", C.c_double)]


class CProgramFilterInfo(C.Structure):
    """omx_program_filter_info (include/omx/program_filter.h)"""
    _fields_ = [("chunk_frames", C.c_uint32), ("tile_frames", C.c_uint32), ("channels", C.c_uint32), ("streams_per_wavefront", C.c_uint32)]


class CProgramFilterRecord(C.Structure):
    """omx_program_filter_record (include/omx/program_filter.h)"""
    _fields_ = [("frames", C.c_uint64), ("frames_total", C.c_uint64), ("samples_over", C.c_uint64), ("samples_nonfinite", C.c_uint64),
                ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float), ("form", C.c_uint32), ("_pad", C.c_uint32)]


FILTER_SECTION_DTYPE = np.dtype([("b0", "<f8"), ("b1", "<f8"), ("b2", "<f8"), ("a1", "<f8"), ("a2", "<f8")])
FILTER_DTYPE = np.dtype([("n_sections", "<u4"), ("_pad", "<u4"), ("section", FILTER_SECTION_DTYPE, (FILTER_MAX_SECTIONS,))])
FILTER_INFO_DTYPE = np.dtype([("chunk_frames", "<u4"), ("tile_frames", "<u4"), ("channels", "<u4"), ("streams_per_wavefront", "<u4")])
FILTER_RECORD_DTYPE = np.dtype([("frames", "<u8"), ("frames_total", "<u8"), ("samples_over", "<u8"), ("samples_nonfinite", "<u8"),
                                ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("form", "<u4"), ("_pad", "<u4")])
assert C.sizeof(CProgramFilterSection) == 40 and C.sizeof(CProgramFilter) == 88 and C.sizeof(CProgramFilterSpec) == 48
assert C.sizeof(CProgramFilterInfo) == 16 and C.sizeof(CProgramFilterRecord) == 48
assert FILTER_DTYPE.itemsize == 88 and FILTER_INFO_DTYPE.itemsize == 16 and FILTER_RECORD_DTYPE.itemsize == 48


@dataclass
class FilterSpec:
    """omx_program_filter_spec: the kind (FILTER_*), the order (FILTER_HIGHPASS / FILTER_LOWPASS: 1, 2 or 4), the corner or centre
    frequency, q (0: 1/sqrt(2)), the gain of a shelf or peak, and for the emphasis kinds the time constant in microseconds with the
    other one of a pair (50 / 15) as time_constant_zero_us."""
    kind: int = FILTER_HIGHPASS
    order: int = 0
    frequency_hz: float = 0.0
    q: float = 0.0
    gain_db: float = 0.0
    time_constant_us: float = 0.0
    time_constant_zero_us: float = 0.0

    def to_c(self) -> CProgramFilterSpec:
        return CProgramFilterSpec(self.kind, self.order, self.frequency_hz, self.q, self.gain_db, self.time_constant_us,
                                  self.time_constant_zero_us)


def filter_table(filters) -> np.ndarray:
    """Filters as a contiguous FILTER_DTYPE array: one FILTER_DTYPE scalar or array, or a sequence whose entries are FILTER_DTYPE
    scalars or lists of one or two (b0, b1, b2, a1, a2)."""
    if isinstance(filters, np.ndarray) and filters.dtype == FILTER_DTYPE:
        return np.ascontiguousarray(filters).reshape(-1)
    out = np.zeros((len(filters),), FILTER_DTYPE)
    for k, f in enumerate(filters):
        if isinstance(f, (np.ndarray, np.void)) and f.dtype == FILTER_DTYPE:
            out[k] = f
        else:
            out[k]["n_sections"] = len(f)
            for i, sec in enumerate(list(f)[:FILTER_MAX_SECTIONS]):
                out[k]["section"][i] = tuple(sec)
    return out


def filter_design(api: Api, spec: FilterSpec, sample_rate: float) -> np.ndarray:
    """The filter of a spec at a sample rate (omx_program_filter_design) as a FILTER_DTYPE scalar.  Needs no device."""
    out, c = np.zeros((1,), FILTER_DTYPE), spec.to_c()
    api.check(api.fn("program_filter_design", C.c_int, [C.c_void_p, C.c_double, C.c_void_p])(C.byref(c), sample_rate, out.ctypes.data))
    return out[0]


def filter_cascade(api: Api, a, b) -> np.ndarray:
    """The sections of a, then those of b (omx_program_filter_cascade) as a FILTER_DTYPE scalar.  Needs no device."""
    fa, fb, out = filter_table([a]), filter_table([b]), np.zeros((1,), FILTER_DTYPE)
    api.check(api.fn("program_filter_cascade", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])(fa.ctypes.data, fb.ctypes.data, out.ctypes.data))
    return out[0]


def filter_check(api: Api, filt) -> int:
    """0 for a filter the bank takes (omx_program_filter_check); raises OmxError with status -3 for an invalid one, -2 for one that is
    not strictly stable.  Needs no device."""
    f = filter_table([filt])
    return api.check(api.fn("program_filter_check", C.c_int, [C.c_void_p])(f.ctypes.data))


def filter_response(api: Api, filt, sample_rate: float, frequency_hz: float):
    """(magnitude in dB, phase in radians) of H(e^{jw}) (omx_program_filter_response).  Needs no device."""
    f, mag, ph = filter_table([filt]), C.c_double(), C.c_double()
    api.check(api.fn("program_filter_response", C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p])(
        f.ctypes.data, sample_rate, frequency_hz, C.byref(mag), C.byref(ph)))
    return mag.value, ph.value


def filter_plan(api: Api, channels: int, sample_rate: float) -> np.ndarray:
    """The plan of a channel count and rate (omx_program_filter_plan) as a FILTER_INFO_DTYPE scalar: the work item of the
    time-parallel form and the kernels' tile, in frames.  Needs no device."""
    out = np.zeros((1,), FILTER_INFO_DTYPE)
    api.check(api.fn("program_filter_plan", C.c_int, [C.c_uint32, C.c_double, C.c_void_p])(channels, sample_rate, out.ctypes.data))
    return out[0]


class CProgramFir(C.Structure):
    """omx_program_fir (include/omx/program_convolve.h)"""
    _fields_ = [("taps", C.c_void_p), ("n_taps", C.c_uint32), ("flags", C.c_uint32)]


class CProgramConvolveSpec(C.Structure):
    """omx_program_convolve_spec (include/omx/program_convolve.h)"""
    _fields_ = [("kind", C.c_uint32), ("n_taps", C.c_uint32), ("f_lo_hz", C.c_double), ("f_hi_hz", C.c_double), ("beta", C.c_double)]


class CProgramConvolveInfo(C.Structure):
    """omx_program_convolve_info (include/omx/program_convolve.h)"""
    _fields_ = [("tile_frames", C.c_uint32), ("frames_per_thread", C.c_uint32), ("tap_block", C.c_uint32), ("channels", C.c_uint32)]


class CProgramConvolveRecord(C.Structure):
    """omx_program_convolve_record (include/omx/program_convolve.h)"""
    _fields_ = [("frames_in", C.c_uint64), ("frames_out", C.c_uint64), ("frames_written", C.c_uint64), ("samples_over", C.c_uint64),
                ("samples_nonfinite", C.c_uint64), ("out_sample_peak", C.c_float), ("out_sample_peak_db", C.c_float),
                ("state", C.c_uint32), ("delay_frames", C.c_uint32), ("max_taps", C.c_uint32), ("_pad", C.c_uint32)]


CONVOLVE_INFO_DTYPE = np.dtype([("tile_frames", "<u4"), ("frames_per_thread", "<u4"), ("tap_block", "<u4"), ("channels", "<u4")])
CONVOLVE_RECORD_DTYPE = np.dtype([("frames_in", "<u8"), ("frames_out", "<u8"), ("frames_written", "<u8"), ("samples_over", "<u8"),
                                  ("samples_nonfinite", "<u8"), ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"),
                                  ("state", "<u4"), ("delay_frames", "<u4"), ("max_taps", "<u4"), ("_pad", "<u4")])
assert C.sizeof(CProgramFir) == 16 and C.sizeof(CProgramConvolveSpec) == 32 and C.sizeof(CProgramConvolveInfo) == 16
assert C.sizeof(CProgramConvolveRecord) == 64 and CONVOLVE_INFO_DTYPE.itemsize == 16 and CONVOLVE_RECORD_DTYPE.itemsize == 64
CONVOLVE_MAX_TAPS = 4096
CONVOLVE_MAX_FIRS = 64
CONVOLVE_BYPASS = 0xFFFFFFFF
CONVOLVE_LOWPASS, CONVOLVE_HIGHPASS, CONVOLVE_BANDPASS, CONVOLVE_BANDSTOP = range(4)   # omx_program_convolve_spec.kind
CONVOLVE_IDLE, CONVOLVE_RUNNING, CONVOLVE_FLUSHED = 0, 1, 2                             # omx_program_convolve_record.state


@dataclass
class ConvolveSpec:
    """omx_program_convolve_spec: the kind (CONVOLVE_*), the odd tap count, the band edges (LOWPASS uses f_hi_hz, HIGHPASS f_lo_hz,
    the band kinds both) and Kaiser beta."""
    kind: int = CONVOLVE_LOWPASS
    n_taps: int = 255
    f_lo_hz: float = 0.0
    f_hi_hz: float = 0.0
    beta: float = 9.0

    def to_c(self) -> CProgramConvolveSpec:
        return CProgramConvolveSpec(self.kind, self.n_taps, self.f_lo_hz, self.f_hi_hz, self.beta)


def _fir_table(firs, flags: int = 0):
    """(C array of omx_program_fir, the f32 arrays it points into) of a sequence of tap sequences"""
    keep = [np.ascontiguousarray(t, np.float32).reshape(-1) for t in firs]
    table = (CProgramFir * max(len(keep), 1))()
    for k, t in enumerate(keep):
        table[k] = CProgramFir(t.ctypes.data if t.size else None, t.size, flags)
    return table, keep


def convolve_plan(api: Api, channels: int, max_taps: int = 1) -> np.ndarray:
    """The plan of a channel count (omx_program_convolve_plan) as a CONVOLVE_INFO_DTYPE scalar: the main kernel's tile, the frames a
    thread keeps in registers and the tap block.  Needs no device."""
    out = np.zeros((1,), CONVOLVE_INFO_DTYPE)
    api.check(api.fn("program_convolve_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p])(channels, max_taps, out.ctypes.data))
    return out[0]


def convolve_frames(api: Api, delay_frames: int, frames_in_before: int, frames_out_before: int, frames: int, flush: bool = False) -> int:
    """Frames a stream emits in a call that brings `frames` frames under delay_frames, after frames_in_before taken and
    frames_out_before emitted (omx_program_convolve_frames): what d_out has to hold.  Needs no device."""
    out = C.c_uint64()
    api.check(api.fn("program_convolve_frames", C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])(
        delay_frames, frames_in_before, frames_out_before, frames, 1 if flush else 0, C.byref(out)))
    return int(out.value)


def convolve_check(api: Api, taps, flags: int = 0) -> int:
    """0 for a FIR the bank takes (omx_program_convolve_check); raises OmxError with status -3 otherwise.  Needs no device."""
    table, _keep = _fir_table([taps], flags)
    return api.check(api.fn("program_convolve_check", C.c_int, [C.c_void_p])(C.byref(table[0])))


def convolve_design(api: Api, spec: ConvolveSpec, sample_rate: float) -> np.ndarray:
    """The f32 taps of a spec at a sample rate (omx_program_convolve_design): a Kaiser-windowed linear-phase FIR.  Needs no device."""
    out, c = np.zeros((max(int(spec.n_taps), 0),), np.float32), spec.to_c()
    api.check(api.fn("program_convolve_design", C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_uint32])(
        C.byref(c), sample_rate, out.ctypes.data, out.size))
    return out


def convolve_response(api: Api, taps, sample_rate: float, frequency_hz: float):
    """(magnitude in dB, phase in radians) of the FIR's H(e^{jw}) (omx_program_convolve_response).  Needs no device."""
    (table, _keep), mag, ph = _fir_table([taps]), C.c_double(), C.c_double()
    api.check(api.fn("program_convolve_response", C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p])(
        C.byref(table[0]), sample_rate, frequency_hz, C.byref(mag), C.byref(ph)))
    return mag.value, ph.value


class CProgramDynamicsCurve(C.Structure):
    """omx_program_dynamics_curve (include/omx/program_dynamics.h)"""
    _fields_ = [("T", C.c_int32 * 769), ("detector_mask", C.c_uint32), ("attack_frames", C.c_uint32), ("hold_frames", C.c_uint32),
                ("release_step", C.c_int64)]


class CProgramDynamicsSpec(C.Structure):
    """omx_program_dynamics_spec (include/omx/program_dynamics.h)"""
    _fields_ = [("threshold_db", C.c_double), ("ratio", C.c_double), ("knee_db", C.c_double), ("expander_threshold_db", C.c_double),
                ("expander_ratio", C.c_double), ("range_db", C.c_double), ("makeup_db", C.c_double)]


class CProgramDynamicsPoint(C.Structure):
    """omx_program_dynamics_point (include/omx/program_dynamics.h)"""
    _fields_ = [("in_db", C.c_double), ("out_db", C.c_double)]


class CProgramDynamicsInfo(C.Structure):
    """omx_program_dynamics_info (include/omx/program_dynamics.h)"""
    _fields_ = [("level_tile", C.c_uint32), ("hold_tile", C.c_uint32), ("hold_max_window", C.c_uint32), ("release_tile", C.c_uint32),
                ("smooth_tile", C.c_uint32), ("chain_threads", C.c_uint32), ("channels", C.c_uint32), ("_pad", C.c_uint32)]


class CProgramDynamicsRecord(C.Structure):
    """omx_program_dynamics_record (include/omx/program_dynamics.h)"""
    _fields_ = [("frames_in", C.c_uint64), ("frames_out", C.c_uint64), ("frames_written", C.c_uint64), ("frames_reduced", C.c_uint64),
                ("frames_boosted", C.c_uint64), ("samples_over", C.c_uint64), ("samples_nonfinite", C.c_uint64), ("min_gain", C.c_int64),
                ("max_gain", C.c_int64), ("min_gain_db", C.c_float), ("max_gain_db", C.c_float), ("out_sample_peak", C.c_float),
                ("out_sample_peak_db", C.c_float), ("state", C.c_uint32), ("latency_frames", C.c_uint32), ("curve_index", C.c_uint32),
                ("_pad", C.c_uint32)]


DYNAMICS_INFO_DTYPE = np.dtype([("level_tile", "<u4"), ("hold_tile", "<u4"), ("hold_max_window", "<u4"), ("release_tile", "<u4"),
                                ("smooth_tile", "<u4"), ("chain_threads", "<u4"), ("channels", "<u4"), ("_pad", "<u4")])
DYNAMICS_RECORD_DTYPE = np.dtype([("frames_in", "<u8"), ("frames_out", "<u8"), ("frames_written", "<u8"), ("frames_reduced", "<u8"),
                                  ("frames_boosted", "<u8"), ("samples_over", "<u8"), ("samples_nonfinite", "<u8"), ("min_gain", "<i8"),
                                  ("max_gain", "<i8"), ("min_gain_db", "<f4"), ("max_gain_db", "<f4"), ("out_sample_peak", "<f4"),
                                  ("out_sample_peak_db", "<f4"), ("state", "<u4"), ("latency_frames", "<u4"), ("curve_index", "<u4"),
                                  ("_pad", "<u4")])
assert C.sizeof(CProgramDynamicsCurve) == 3096 and C.sizeof(CProgramDynamicsSpec) == 56 and C.sizeof(CProgramDynamicsPoint) == 16
assert C.sizeof(CProgramDynamicsInfo) == 32 and C.sizeof(CProgramDynamicsRecord) == 104
assert DYNAMICS_INFO_DTYPE.itemsize == 32 and DYNAMICS_RECORD_DTYPE.itemsize == 104
DYNAMICS_CURVE_POINTS = 769
DYNAMICS_TABLE_ENTRIES = 257
DYNAMICS_MAX_CURVES = 64
DYNAMICS_MAX_POINTS = 16
DYNAMICS_MAX_ATTACK = 4096
DYNAMICS_MAX_HOLD = 16384
DYNAMICS_L_MIN, DYNAMICS_L_MAX = -40 * 65536, 8 * 65536
DYNAMICS_MAX_GAIN = 40 * 65536
DYNAMICS_MAX_STEP = 40 << 32
DYNAMICS_OCTAVE_DB = 6.020599913279624
DYNAMICS_BYPASS = 0xFFFFFFFF
DYNAMICS_IDLE, DYNAMICS_RUNNING, DYNAMICS_FLUSHED = 0, 1, 2                             # omx_program_dynamics_record.state


@dataclass
class DynamicsSpec:
    """omx_program_dynamics_spec: a compressor (threshold, ratio, soft knee), an optional downward expander below it (its threshold,
    ratio and largest reduction) and the make-up gain, all in dB."""
    threshold_db: float = -20.0
    ratio: float = 4.0
    knee_db: float = 0.0
    expander_threshold_db: float = -60.0
    expander_ratio: float = 1.0
    range_db: float = float("inf")
    makeup_db: float = 0.0

    def to_c(self) -> CProgramDynamicsSpec:
        return CProgramDynamicsSpec(self.threshold_db, self.ratio, self.knee_db, self.expander_threshold_db, self.expander_ratio,
                                    self.range_db, self.makeup_db)


@dataclass
class DynamicsCurve:
    """omx_program_dynamics_curve: the table T[769] (gain in 2^-16 octave at level L_MIN + 4096 k), the channels the level is taken
    from, the attack and hold in frames and the release step in 2^-32 octave per frame."""
    T: Sequence[int]
    detector_mask: int = 1
    attack_frames: int = 1
    hold_frames: int = 0
    release_step: int = DYNAMICS_MAX_STEP

    def to_c(self) -> CProgramDynamicsCurve:
        c = CProgramDynamicsCurve()
        t = np.ascontiguousarray(self.T, np.int32).reshape(-1)
        if t.size != DYNAMICS_CURVE_POINTS:
            raise ValueError(f"a dynamics curve has {DYNAMICS_CURVE_POINTS} entries, not {t.size}")
        C.memmove(c.T, t.ctypes.data, t.nbytes)
        c.detector_mask, c.attack_frames, c.hold_frames, c.release_step = self.detector_mask, self.attack_frames, self.hold_frames, self.release_step
        return c


def _dynamics_c(curve) -> CProgramDynamicsCurve:
    return curve if isinstance(curve, CProgramDynamicsCurve) else curve.to_c()


def dynamics_plan(api: Api, channels: int) -> np.ndarray:
    """The tiles of the dynamics passes (omx_program_dynamics_plan) as a DYNAMICS_INFO_DTYPE scalar.  Needs no device."""
    out = np.zeros((1,), DYNAMICS_INFO_DTYPE)
    api.check(api.fn("program_dynamics_plan", C.c_int, [C.c_uint32, C.c_void_p])(channels, out.ctypes.data))
    return out[0]


def dynamics_tables(api: Api):
    """(LOG int32 [257], EXP uint64 [257]) as the library holds them (omx_program_dynamics_tables).  Needs no device."""
    lg, ex = np.zeros((DYNAMICS_TABLE_ENTRIES,), np.int32), np.zeros((DYNAMICS_TABLE_ENTRIES,), np.uint64)
    api.check(api.fn("program_dynamics_tables", C.c_int, [C.c_void_p, C.c_void_p])(lg.ctypes.data, ex.ctypes.data))
    return lg, ex


def dynamics_check(api: Api, curve) -> int:
    """0 for a curve the bank takes (omx_program_dynamics_check); raises OmxError with status -3 otherwise.  Needs no device."""
    c = _dynamics_c(curve)
    return api.check(api.fn("program_dynamics_check", C.c_int, [C.c_void_p])(C.byref(c)))


def dynamics_latency(api: Api, curve) -> int:
    """The latency in frames of a stream on the curve, attack_frames - 1 (omx_program_dynamics_latency).  Needs no device."""
    c, out = _dynamics_c(curve), C.c_uint32()
    api.check(api.fn("program_dynamics_latency", C.c_int, [C.c_void_p, C.c_void_p])(C.byref(c), C.byref(out)))
    return int(out.value)


def dynamics_design(api: Api, spec: DynamicsSpec) -> np.ndarray:
    """The table int32 [769] of a spec (omx_program_dynamics_design).  Needs no device."""
    c, s = CProgramDynamicsCurve(), spec.to_c()
    api.check(api.fn("program_dynamics_design", C.c_int, [C.c_void_p, C.c_void_p])(C.byref(s), C.byref(c)))
    return np.array(c.T, np.int32)


def dynamics_from_points(api: Api, points) -> np.ndarray:
    """The table int32 [769] of up to 16 (in_db, out_db) pairs, piecewise linear in dB with slope 1 outside them: the transfer
    function of sox compand (omx_program_dynamics_from_points).  Needs no device."""
    pts = list(points)
    arr, c = (CProgramDynamicsPoint * max(len(pts), 1))(), CProgramDynamicsCurve()
    for k, (a, b) in enumerate(pts):
        arr[k] = CProgramDynamicsPoint(a, b)
    api.check(api.fn("program_dynamics_from_points", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p])(arr, len(pts), C.byref(c)))
    return np.array(c.T, np.int32)


def dynamics_gain_db(api: Api, T, level_db: float) -> float:
    """The table's gain in dB at a level in dB, evaluated as the kernel evaluates it (omx_program_dynamics_gain_db).  Needs no device."""
    c, out = DynamicsCurve(T).to_c(), C.c_double()
    api.check(api.fn("program_dynamics_gain_db", C.c_int, [C.c_void_p, C.c_double, C.c_void_p])(C.byref(c), level_db, C.byref(out)))
    return out.value


def dynamics_time(api: Api, sample_rate: float, attack_ms: float, hold_ms: float, release_db_per_s: float):
    """(attack_frames, hold_frames, release_step) of times at a sample rate (omx_program_dynamics_time).  Needs no device."""
    a, h, d = C.c_uint32(), C.c_uint32(), C.c_int64()
    api.check(api.fn("program_dynamics_time", C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p])(
        sample_rate, attack_ms, hold_ms, release_db_per_s, C.byref(a), C.byref(h), C.byref(d)))
    return int(a.value), int(h.value), int(d.value)


def dynamics_frames(api: Api, latency_frames: int, frames_in_before: int, frames_out_before: int, frames: int, flush: bool = False) -> int:
    """Frames a stream emits in a call that brings `frames` frames under a latency, after frames_in_before taken and
    frames_out_before emitted (omx_program_dynamics_frames): what d_out has to hold.  Needs no device."""
    out = C.c_uint64()
    api.check(api.fn("program_dynamics_frames", C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])(
        latency_frames, frames_in_before, frames_out_before, frames, 1 if flush else 0, C.byref(out)))
    return int(out.value)


# ---- include/omx/program_spectrum.h
class CProgramSpectrumRule(C.Structure):
    """omx_program_spectrum_rule (include/omx/program_spectrum.h)"""
    _fields_ = [("fft_size", C.c_uint32), ("flags", C.c_uint32)]


class CProgramSpectrumInfo(C.Structure):
    """omx_program_spectrum_info (include/omx/program_spectrum.h)"""
    _fields_ = [("fft_size", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("threads", C.c_uint32),
                ("transforms_per_workgroup", C.c_uint32), ("run", C.c_uint32), ("lds_bytes", C.c_uint32), ("channels", C.c_uint32),
                ("scratch_bytes", C.c_uint64), ("state_bytes", C.c_uint64)]


class CProgramSpectrumRecord(C.Structure):
    """omx_program_spectrum_record (include/omx/program_spectrum.h)"""
    _fields_ = [("frames", C.c_uint64), ("transforms", C.c_uint64 * 8), ("skipped", C.c_uint64 * 8), ("fft_size", C.c_uint32),
                ("channels", C.c_uint32), ("finished", C.c_uint32), ("_pad", C.c_uint32)]


SPECTRUM_MAX_PROBES = 8


class CProgramSpectrumQc(C.Structure):
    """omx_program_spectrum_qc (include/omx/program_spectrum.h)"""
    _fields_ = [("occupied_fraction", C.c_double), ("bandwidth_min_ratio", C.c_double), ("tone_db", C.c_double),
                ("probe_hz", C.c_double * SPECTRUM_MAX_PROBES), ("n_probes", C.c_uint32), ("flags", C.c_uint32)]


class CProgramSpectrumSummary(C.Structure):
    """omx_program_spectrum_summary (include/omx/program_spectrum.h)"""
    _fields_ = [("verdict", C.c_uint32), ("n_probes", C.c_uint32), ("total_db", C.c_double), ("peak_hz", C.c_double),
                ("peak_db", C.c_double), ("occupied_hz", C.c_double), ("prominence_db", C.c_double * SPECTRUM_MAX_PROBES)]


class CProgramSpectrumMatchSpec(C.Structure):
    """omx_program_spectrum_match_spec (include/omx/program_spectrum.h)"""
    _fields_ = [("max_boost_db", C.c_double), ("max_cut_db", C.c_double), ("low_hz", C.c_double), ("high_hz", C.c_double),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


SPECTRUM_INFO_DTYPE = np.dtype([("fft_size", "<u4"), ("hop", "<u4"), ("bins", "<u4"), ("threads", "<u4"),
                                ("transforms_per_workgroup", "<u4"), ("run", "<u4"), ("lds_bytes", "<u4"), ("channels", "<u4"),
                                ("scratch_bytes", "<u8"), ("state_bytes", "<u8")])
SPECTRUM_RECORD_DTYPE = np.dtype([("frames", "<u8"), ("transforms", "<u8", (8,)), ("skipped", "<u8", (8,)), ("fft_size", "<u4"),
                                  ("channels", "<u4"), ("finished", "<u4"), ("_pad", "<u4")])
SPECTRUM_SUMMARY_DTYPE = np.dtype([("verdict", "<u4"), ("n_probes", "<u4"), ("total_db", "<f8"), ("peak_hz", "<f8"), ("peak_db", "<f8"),
                                   ("occupied_hz", "<f8"), ("prominence_db", "<f8", (SPECTRUM_MAX_PROBES,))])
assert C.sizeof(CProgramSpectrumRule) == 8 and C.sizeof(CProgramSpectrumInfo) == 48 and C.sizeof(CProgramSpectrumRecord) == 152
assert C.sizeof(CProgramSpectrumQc) == 96 and C.sizeof(CProgramSpectrumSummary) == 104 and C.sizeof(CProgramSpectrumMatchSpec) == 40
assert SPECTRUM_INFO_DTYPE.itemsize == 48 and SPECTRUM_RECORD_DTYPE.itemsize == 152 and SPECTRUM_SUMMARY_DTYPE.itemsize == 104
SPECTRUM_RUN, SPECTRUM_MAX_BANDS, SPECTRUM_MAX_TAPS, SPECTRUM_DB_FLOOR = 16, 48, 4095, -400.0
SPECTRUM_BANDLIMITED, SPECTRUM_TONE = 1, 2      # omx_program_spectrum_summary.verdict


@dataclass
class SpectrumRule:
    """omx_program_spectrum_rule: Welch's method with a periodic Hann of fft_size points (2048, 4096 or 8192) at half overlap."""
    fft_size: int = 4096
    flags: int = 0

    def to_c(self) -> CProgramSpectrumRule:
        return CProgramSpectrumRule(self.fft_size, self.flags)


@dataclass
class SpectrumQc:
    """omx_program_spectrum_qc: the fraction of the power the occupied bandwidth holds, the share of fs/2 below which a programme
    counts as band-limited, the prominence in dB at which a probe counts as a tone, the probe frequencies."""
    occupied_fraction: float = 0.9999
    bandwidth_min_ratio: float = 0.8
    tone_db: float = 20.0
    probe_hz: Sequence[float] = (50.0, 100.0, 150.0, 60.0, 120.0, 180.0)
    flags: int = 0
    n_probes: Optional[int] = None      # None: len(probe_hz)

    def to_c(self) -> CProgramSpectrumQc:
        probes = list(self.probe_hz)[:SPECTRUM_MAX_PROBES]
        n = len(self.probe_hz) if self.n_probes is None else self.n_probes
        return CProgramSpectrumQc(self.occupied_fraction, self.bandwidth_min_ratio, self.tone_db,
                                  (C.c_double * SPECTRUM_MAX_PROBES)(*probes), n, self.flags)


@dataclass
class SpectrumMatchSpec:
    """omx_program_spectrum_match_spec: the most a match FIR boosts and cuts, and the band outside which its gain is held."""
    max_boost_db: float = 12.0
    max_cut_db: float = 12.0
    low_hz: float = 40.0
    high_hz: float = 0.45 * 48000.0
    flags: int = 0

    def to_c(self) -> CProgramSpectrumMatchSpec:
        return CProgramSpectrumMatchSpec(self.max_boost_db, self.max_cut_db, self.low_hz, self.high_hz, self.flags, 0)


def _density_arg(density, fft_size: int) -> np.ndarray:
    d = np.ascontiguousarray(density, np.float64).reshape(-1)
    if fft_size in (2048, 4096, 8192) and d.size != fft_size // 2 + 1:
        raise ValueError(f"density: {d.size} entries for {fft_size // 2 + 1} bins")
    return d


def spectrum_rule_default(api: Api) -> SpectrumRule:
    """The header's default rule as the library fills it (omx_program_spectrum_rule_default).  Needs no device."""
    c = CProgramSpectrumRule()
    api.check(api.fn("program_spectrum_rule_default", C.c_int, [C.c_void_p])(C.byref(c)))
    return SpectrumRule(c.fft_size, c.flags)


def spectrum_qc_default(api: Api) -> SpectrumQc:
    """The header's default QC rule (omx_program_spectrum_qc_default).  Needs no device."""
    c = CProgramSpectrumQc()
    api.check(api.fn("program_spectrum_qc_default", C.c_int, [C.c_void_p])(C.byref(c)))
    return SpectrumQc(c.occupied_fraction, c.bandwidth_min_ratio, c.tone_db, tuple(c.probe_hz[:c.n_probes]), c.flags)


def spectrum_match_spec_default(api: Api, sample_rate: float) -> SpectrumMatchSpec:
    """The header's default match spec at a sample rate (omx_program_spectrum_match_spec_default).  Needs no device."""
    c = CProgramSpectrumMatchSpec()
    api.check(api.fn("program_spectrum_match_spec_default", C.c_int, [C.c_double, C.c_void_p])(sample_rate, C.byref(c)))
    return SpectrumMatchSpec(c.max_boost_db, c.max_cut_db, c.low_hz, c.high_hz, c.flags)


def spectrum_plan(api: Api, rule: SpectrumRule, channels: int, n_streams: int = 1, frames: int = 0) -> np.ndarray:
    """The transform kernel's tile and the memory of a bank (omx_program_spectrum_plan) as a SPECTRUM_INFO_DTYPE scalar.  Needs no
    device."""
    out, c = np.zeros((1,), SPECTRUM_INFO_DTYPE), rule.to_c()
    api.check(api.fn("program_spectrum_plan", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p])(
        C.byref(c), channels, n_streams, frames, out.ctypes.data))
    return out[0]


def spectrum_window(api: Api, fft_size: int) -> np.ndarray:
    """The window of a transform size as the kernels take it, f32 [fft_size] (omx_program_spectrum_window).  Needs no device."""
    out = np.zeros((max(int(fft_size), 1),), np.float32)
    api.check(api.fn("program_spectrum_window", C.c_int, [C.c_uint32, C.c_void_p])(fft_size, out.ctypes.data))
    return out


def spectrum_transforms(api: Api, frames: int, finished: bool, fft_size: int) -> int:
    """Transforms a stream of `frames` frames has taken (omx_program_spectrum_transforms).  Needs no device."""
    out = C.c_uint64()
    api.check(api.fn("program_spectrum_transforms", C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p])(
        frames, 1 if finished else 0, fft_size, C.byref(out)))
    return int(out.value)


def spectrum_density(api: Api, record: np.ndarray, sums: np.ndarray, channel: int) -> np.ndarray:
    """The one-sided mean square per bin of one channel, f64 [fft_size / 2 + 1], from a SPECTRUM_RECORD_DTYPE record and its sums
    [channels][bins] (omx_program_spectrum_density).  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(record, SPECTRUM_RECORD_DTYPE).reshape(1))
    s = np.ascontiguousarray(sums, np.float64)
    bins = int(rec["fft_size"][0]) // 2 + 1
    if s.size != int(rec["channels"][0]) * bins:
        raise ValueError(f"sums: {s.size} entries for {int(rec['channels'][0])} channels of {bins} bins")
    out = np.zeros((bins,), np.float64)
    api.check(api.fn("program_spectrum_density", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])(
        rec.ctypes.data, s.ctypes.data, channel, out.ctypes.data))
    return out


def spectrum_bands(api: Api, density, fft_size: int, sample_rate: float, fraction: int = 3):
    """(centre_hz, level_db) of the octave (fraction 1) or third-octave (3) bands of IEC 61260-1 that lie inside the spectrum
    (omx_program_spectrum_bands); a full-scale sine reads 0 dB.  Needs no device."""
    d = _density_arg(density, fft_size)
    centre, level, n = np.zeros((SPECTRUM_MAX_BANDS,)), np.zeros((SPECTRUM_MAX_BANDS,)), C.c_uint32(SPECTRUM_MAX_BANDS)
    api.check(api.fn("program_spectrum_bands", C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])(
        d.ctypes.data, fft_size, sample_rate, fraction, centre.ctypes.data, level.ctypes.data, C.byref(n)))
    return centre[:n.value].copy(), level[:n.value].copy()


def spectrum_summarize(api: Api, qc: SpectrumQc, density, fft_size: int, sample_rate: float) -> np.ndarray:
    """The QC figures of one density as a SPECTRUM_SUMMARY_DTYPE scalar: total level, peak, occupied bandwidth, the prominence of
    every probe and the verdict bits (omx_program_spectrum_summarize).  Needs no device."""
    d, c, out = _density_arg(density, fft_size), qc.to_c(), np.zeros((1,), SPECTRUM_SUMMARY_DTYPE)
    api.check(api.fn("program_spectrum_summarize", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p])(
        C.byref(c), d.ctypes.data, fft_size, sample_rate, out.ctypes.data))
    return out[0]


def spectrum_match(api: Api, density_source, density_target, fft_size: int, sample_rate: float, spec: SpectrumMatchSpec,
                   n_taps: int) -> np.ndarray:
    """The taps, f32 [n_taps], of a linear-phase FIR for the convolve stage that brings the source's tonal balance to the target's
    (omx_program_spectrum_match).  Needs no device."""
    ds, dt, c = _density_arg(density_source, fft_size), _density_arg(density_target, fft_size), spec.to_c()
    out = np.zeros((max(int(n_taps), 1),), np.float32)
    api.check(api.fn("program_spectrum_match", C.c_int,
                     [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_uint32])(
        ds.ctypes.data, dt.ctypes.data, fft_size, sample_rate, C.byref(c), out.ctypes.data, n_taps))
    return out[:n_taps]


class ProgramLoudnessBank:
    """S programme meters.  `process` takes device PCM f32 [n_streams][frames_capacity][channels], any frame count per stream."""

    def __init__(self, api: Api, config: capi.LoudnessConfig, n_streams: int, channels: int = 2, capacity_seconds: int = 3600,
                 storage: str = "segments"):
        """storage "segments": one f64 per 100 ms segment, capacity_seconds per stream.  storage "histogram": bounded storage
        (include/omx/program_histogram.h), about 32 KB per stream whatever the length, no overflow; capacity_seconds is not used."""
        if storage not in ("segments", "histogram"):
            raise ValueError(f"storage: {storage!r} is neither 'segments' nor 'histogram'")
        self.api = api
        self.n_streams = n_streams
        self._h = C.c_void_p()
        c = config.to_c()
        if storage == "histogram":
            api.check(api.fn("program_loudness_bank_create_bounded", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)])(
                C.byref(c), n_streams, channels, C.byref(self._h)))
            return
        api.check(api.fn("program_loudness_bank_create", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)])(
            C.byref(c), n_streams, channels, capacity_seconds, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            self.api.fn("program_loudness_bank_destroy", None, [C.c_void_p])(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _per_stream(self, values, dtype, what):
        if values is None:
            return None
        arr = np.ascontiguousarray(values, dtype).reshape(-1)
        if arr.size != self.n_streams:
            raise ValueError(f"{what}: {arr.size} entries for a bank of {self.n_streams} streams")
        return arr

    def reset(self, reset_mask: Optional[Sequence[int]] = None):
        """R 128 start / reset of the flagged streams (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def set_option(self, option: int, value: int):
        self.api.check(self.api.fn("program_loudness_bank_set_option", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64])(self._h, option, value))

    def last_form(self) -> int:
        """1 = the last call ran the reference-order segment pass, 2 = the time-parallel one."""
        return self.api.fn("debug_program_loudness_bank_last_form", C.c_int, [C.c_void_p])(self._h)

    def process(self, device_ptr: int, frames_capacity: int, channels: int, sample_rate: float, positions: Sequence[int],
                frames: Optional[Sequence[int]] = None, reset_mask: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        fr = self._per_stream(frames, np.uint32, "frames")
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        f = self.api.fn("program_loudness_bank_process", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, _u8x8, C.c_void_p])
        return self.api.check(f(self._h, C.c_void_p(device_ptr), frames_capacity, fr.ctypes.data if fr is not None else None,
                                mask.ctypes.data if mask is not None else None, channels, sample_rate, _u8x8(*positions),
                                C.c_void_p(stream or 0)))

    def note_snapshots(self, d_snapshots: int, n_blocks: int, d_n_blocks: int = 0, stream: int = 0):
        """Fold the true peaks of the snapshots a LoudnessBank call left on the device ([n_streams][n_blocks]) into the running maxima."""
        self.api.check(self.api.fn("program_loudness_bank_note_snapshots", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p])(
            self._h, C.c_void_p(d_snapshots), n_blocks, C.c_void_p(d_n_blocks or 0), C.c_void_p(stream or 0)))

    def results(self, stream: int = 0) -> int:
        """Run the result pass on `stream`; returns the device pointer to omx_program_loudness_record[n_streams]."""
        out = C.c_void_p()
        self.api.check(self.api.fn("program_loudness_bank_results", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])(
            self._h, C.c_void_p(stream or 0), C.byref(out)))
        return out.value

    def fetch(self, stream_index: int) -> ProgramLoudnessRecord:
        r = CProgramLoudnessRecord()
        self.api.check(self.api.fn("program_loudness_bank_fetch", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, C.byref(r)))
        return ProgramLoudnessRecord(*[getattr(r, n) for n in _ENERGIES + _COUNTS + _LEVELS], bool(r.overflow))

    def set_peaks(self, on: bool = True):
        """Measure true peak and sample peak inside `process` (include/omx/program_peaks.h); off by default.  Only while no stream
        holds samples: a new bank, or after reset() of every stream."""
        self.api.check(self.api.fn("program_loudness_bank_set_peaks", C.c_int, [C.c_void_p, C.c_uint32])(self._h, 1 if on else 0))

    def peaks(self, stream: int = 0) -> int:
        """Device pointer to omx_program_peak_record[n_streams], valid until the next call on the bank."""
        out = C.c_void_p()
        self.api.check(self.api.fn("program_loudness_bank_peaks", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])(
            self._h, C.c_void_p(stream or 0), C.byref(out)))
        return out.value

    def fetch_peaks(self, stream_index: int) -> ProgramPeakRecord:
        r = CProgramPeakRecord()
        self.api.check(self.api.fn("program_loudness_bank_fetch_peaks", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, C.byref(r)))
        return ProgramPeakRecord(int(r.frames), np.array(r.true_peak_frame[:], np.uint64), np.array(r.sample_peak_frame[:], np.uint64),
                                 np.array(r.true_peak[:], np.float32), np.array(r.sample_peak[:], np.float32),
                                 np.array(r.true_peak_db[:], np.float32), np.array(r.sample_peak_db[:], np.float32),
                                 float(r.max_true_peak_db), float(r.max_sample_peak_db), int(r.max_true_peak_channel),
                                 int(r.oversampling), int(r.channels))

    def fetch_segments(self, stream_index: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Stored segment energies e[first : first + count] of one stream (count None: up to the last stored one)."""
        if count is None:
            count = self.fetch(stream_index).segments - first
        out = np.zeros((max(count, 0),), np.float64)
        self.api.check(self.api.fn("program_loudness_bank_fetch_segments", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])(
            self._h, stream_index, first, count, out.ctypes.data))
        return out

    # ---- include/omx/program_histogram.h
    def is_bounded(self) -> bool:
        return bool(self.api.check(self.api.fn("program_loudness_bank_is_bounded", C.c_int, [C.c_void_p])(self._h)))

    def fetch_histogram(self, stream_index: int) -> ProgramHistogram:
        """One stream's histograms, tail and segment count (banks made with storage="histogram" only); synchronises."""
        h = CProgramHistogram()
        self.api.check(self.api.fn("program_loudness_bank_fetch_histogram", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, C.byref(h)))
        return ProgramHistogram(np.array(h.gating_count[:], np.uint64), np.array(h.gating_sum[:], np.float64),
                                np.array(h.short_term_count[:], np.uint64), np.array(h.short_term_sum[:], np.float64),
                                np.array(h.tail[:h.tail_count], np.float64), int(h.segments))

    # ---- include/omx/program_timeline.h
    def timeline(self, d_rows: int, first: int = 0, stride: int = 1, count: int = 0, stream: int = 0) -> int:
        """Rows j = first + i * stride, i < count, of every stream into the device buffer d_rows: omx_program_timeline_row
        [n_streams][count] (TIMELINE_ROW_DTYPE, 40 bytes each), enqueued on `stream`.  Rows beyond a stream's end are the empty row."""
        f = self.api.fn("program_loudness_bank_timeline", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p])
        return self.api.check(f(self._h, first, stride, count, C.c_void_p(d_rows or 0), C.c_void_p(stream or 0)))

    def fetch_timeline(self, stream_index: int, first: int = 0, stride: int = 1, count: Optional[int] = None) -> np.ndarray:
        """The same rows of one stream as a numpy structured array (count None: up to the last stored segment); synchronises."""
        if count is None:
            segments = self.fetch(stream_index).segments
            count = (segments - first + stride - 1) // stride if stride > 0 and segments > first else 0
        out = np.zeros((max(count, 0),), TIMELINE_ROW_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_timeline", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, stream_index, first, stride, count, out.ctypes.data if count else None))
        return out

    @staticmethod
    def _intervals(intervals) -> np.ndarray:
        """(stream, first_segment, segment_count) triples, or an INTERVAL_DTYPE array, as omx_program_interval[n]"""
        if isinstance(intervals, np.ndarray) and intervals.dtype == INTERVAL_DTYPE:
            return np.ascontiguousarray(intervals)
        out = np.zeros((len(intervals),), INTERVAL_DTYPE)
        for i, (s, first, count) in enumerate(intervals):
            out[i] = (s, 0, first, count)
        return out

    def measure_intervals(self, intervals, stream: int = 0) -> int:
        """The programme record of every interval (stream, first_segment, segment_count), on `stream`; returns the device pointer to
        omx_program_loudness_record[n] (0 for no interval), valid until the next call on the bank."""
        arr = self._intervals(intervals)
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_measure_intervals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, arr.ctypes.data if len(arr) else None, len(arr), C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_intervals(self, intervals) -> np.ndarray:
        """The same records as a numpy structured array (RECORD_DTYPE: the fields of omx_program_loudness_record); synchronises."""
        arr = self._intervals(intervals)
        out = np.zeros((len(arr),), RECORD_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_intervals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, arr.ctypes.data if len(arr) else None, len(arr), out.ctypes.data if len(arr) else None))
        return out

    # ---- include/omx/program_groups.h
    @staticmethod
    def _groups(groups) -> np.ndarray:
        """(first_member, member_count) pairs, or a GROUP_DTYPE array, as omx_program_group[n]"""
        if isinstance(groups, np.ndarray) and groups.dtype == GROUP_DTYPE:
            return np.ascontiguousarray(groups)
        out = np.zeros((len(groups),), GROUP_DTYPE)
        for i, (first, count) in enumerate(groups):
            out[i] = (first, count)
        return out

    def measure_groups(self, members, groups, stream: int = 0) -> int:
        """The record of every group measured as ONE programme (album loudness and range), on `stream`.  members: (stream,
        first_segment, segment_count) triples or an INTERVAL_DTYPE array, segment_count may be TO_END; groups: (first_member,
        member_count) pairs or a GROUP_DTYPE array, ranges of the member table that may overlap.  Returns the device pointer to
        omx_program_loudness_record[n_groups] (0 for no group), valid until the next call on the bank."""
        m, g = self._intervals(members), self._groups(groups)
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_measure_groups", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_groups(self, members, groups) -> np.ndarray:
        """The same records as a numpy structured array (RECORD_DTYPE), one per group; synchronises."""
        m, g = self._intervals(members), self._groups(groups)
        out = np.zeros((len(g),), RECORD_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_groups", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         out.ctypes.data if len(g) else None))
        return out

    # ---- include/omx/program_normalize.h
    def plan_gains(self, rule: GainRule, stream: int = 0) -> int:
        """One gain per stream (track gain) from the bank's own records, on `stream`; returns the device pointer to
        omx_program_gain_record[n_streams] (GAIN_RECORD_DTYPE), valid until the next plan call on the bank."""
        out, c = C.c_void_p(), rule.to_c()
        self.api.check(self.api.fn("program_loudness_bank_plan_gains", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])(
            self._h, C.byref(c), C.c_void_p(stream or 0), C.byref(out)))
        self._planned = self.n_streams
        return out.value or 0

    def plan_group_gains(self, rule: GainRule, members, groups, stream: int = 0) -> int:
        """One gain per group (album gain): measure_groups of `members` / `groups`, then the gain of every group record with the
        largest true peak of the group's member streams.  Returns the device pointer to omx_program_gain_record[n_groups] (0 for no
        group), valid until the next plan call on the bank."""
        m, g = self._intervals(members), self._groups(groups)
        out, c = C.c_void_p(), rule.to_c()
        f = self.api.fn("program_loudness_bank_plan_group_gains", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.byref(c), m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         C.c_void_p(stream or 0), C.byref(out)))
        if len(g):
            self._planned = len(g)
        return out.value or 0

    def fetch_gains(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Records [first, first + count) of the last plan as a GAIN_RECORD_DTYPE array (count None: up to the plan's last record);
        synchronises."""
        if count is None:
            count = max(getattr(self, "_planned", 0) - first, 0)
        out = np.zeros((count,), GAIN_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_gains", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p])(
            self._h, first, count, out.ctypes.data if count else None))
        return out

    # ---- include/omx/program_peak_timeline.h
    def set_peak_timeline(self, on: bool = True):
        """Keep true peak and sample peak per 100 ms segment as well (include/omx/program_peak_timeline.h); off by default.  Needs
        set_peaks(True), and only while no stream holds samples.  set_peaks(False) switches it off too."""
        self.api.check(self.api.fn("program_loudness_bank_set_peak_timeline", C.c_int, [C.c_void_p, C.c_uint32])(self._h, 1 if on else 0))

    def peak_rows(self, d_rows: int, first: int = 0, stride: int = 1, count: int = 0, stream: int = 0) -> int:
        """Row i < count of every stream = the peaks over the segments [first + i * stride, first + (i + 1) * stride), into the device
        buffer d_rows: omx_program_peak_row [n_streams][count] (PEAK_ROW_DTYPE, 136 bytes each), enqueued on `stream`."""
        f = self.api.fn("program_loudness_bank_peak_rows", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p])
        return self.api.check(f(self._h, first, stride, count, C.c_void_p(d_rows or 0), C.c_void_p(stream or 0)))

    def fetch_peak_rows(self, stream_index: int, first: int = 0, stride: int = 1, count: Optional[int] = None) -> np.ndarray:
        """The same rows of one stream as a PEAK_ROW_DTYPE array (count None: up to the stream's last frame, the open segment
        included); synchronises."""
        if count is None:
            frames = int(self.fetch_peaks(stream_index).frames)
            segments = 1 if frames else 0   # no complete segment yet: everything lies in the open one
            if int(self.fetch(stream_index).segments):
                length = int(self.fetch_peak_rows(stream_index, 0, 1, 1)[0]["frames"])   # row 0 is a complete segment: its frames are L
                segments = (frames + length - 1) // length
            count = (segments - first + stride - 1) // stride if stride > 0 and segments > first else 0
        out = np.zeros((max(count, 0),), PEAK_ROW_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_peak_rows", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, stream_index, first, stride, count, out.ctypes.data if count else None))
        return out

    def measure_interval_peaks(self, intervals, stream: int = 0) -> int:
        """The peaks of every interval (stream, first_segment, segment_count; the count may be TO_END), on `stream`; returns the device
        pointer to omx_program_part_peak[n] (0 for no interval), valid until the next call on the bank."""
        arr = self._intervals(intervals)
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_measure_interval_peaks", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, arr.ctypes.data if len(arr) else None, len(arr), C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_interval_peaks(self, intervals) -> np.ndarray:
        """The same records as a PART_PEAK_DTYPE array; synchronises."""
        arr = self._intervals(intervals)
        out = np.zeros((len(arr),), PART_PEAK_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_interval_peaks", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, arr.ctypes.data if len(arr) else None, len(arr), out.ctypes.data if len(arr) else None))
        return out

    def measure_group_peaks(self, members, groups, stream: int = 0) -> int:
        """The peaks of every group of members (tables as for measure_groups), on `stream`; returns the device pointer to
        omx_program_part_peak[n_groups] (0 for no group), valid until the next call on the bank."""
        m, g = self._intervals(members), self._groups(groups)
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_measure_group_peaks", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_group_peaks(self, members, groups) -> np.ndarray:
        """The same records as a PART_PEAK_DTYPE array, one per group; synchronises."""
        m, g = self._intervals(members), self._groups(groups)
        out = np.zeros((len(g),), PART_PEAK_DTYPE)
        f = self.api.fn("program_loudness_bank_fetch_group_peaks", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p])
        self.api.check(f(self._h, m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         out.ctypes.data if len(g) else None))
        return out

    def plan_part_gains(self, rule: GainRule, members, groups, stream: int = 0) -> int:
        """plan_group_gains with the true peak of the group's own segments (the peak timeline) as the source peak, not that of the
        members' whole streams.  Same records, buffer and fetch_gains."""
        m, g = self._intervals(members), self._groups(groups)
        out, c = C.c_void_p(), rule.to_c()
        f = self.api.fn("program_loudness_bank_plan_part_gains", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.byref(c), m.ctypes.data if len(m) else None, len(m), g.ctypes.data if len(g) else None, len(g),
                         C.c_void_p(stream or 0), C.byref(out)))
        if len(g):
            self._planned = len(g)
        return out.value or 0

    def apply_gains(self, d_in: int, d_out: int, frames_capacity: int, channels: int, d_gains: int, n_gains: int,
                    frames: Optional[Sequence[int]] = None, gain_of_stream: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """d_out[s][f][c] = d_in[s][f][c] * gain of stream s, for f < frames[s], on `stream` (d_out == d_in: in place).  d_gains:
        device pointer to n_gains omx_program_gain_record (a plan call's, or the caller's own); gain_of_stream[s]: the record of
        stream s, UNITY_GAIN for factor 1, None: stream s uses record s.  Returns the device pointer to
        omx_program_apply_record[n_streams] (APPLY_RECORD_DTYPE), written fresh by every call."""
        fr = self._per_stream(frames, np.uint32, "frames")
        gi = self._per_stream(gain_of_stream, np.uint32, "gain_of_stream")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_apply_gains", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                         C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), C.c_void_p(d_out or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                         channels, C.c_void_p(d_gains or 0), n_gains, gi.ctypes.data if gi is not None else None, C.c_void_p(stream or 0),
                         C.byref(out)))
        return out.value or 0

    def fetch_applied(self, stream_index: int) -> np.ndarray:
        """One stream's record of the last apply_gains call as an APPLY_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), APPLY_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_applied", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_limit.h
    def configure_limiter(self, rule: LimitRule, channels: int, sample_rate: float):
        """Set the limiter's rule and the format of the PCM it takes; allocates its state.  Only while no stream of the limiter holds
        frames: a new bank, or after reset_limiter() of every stream."""
        c = rule.to_c()
        self.api.check(self.api.fn("program_loudness_bank_limiter_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float])(
            self._h, C.byref(c), channels, sample_rate))

    def reset_limiter(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the limiter start over (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_limiter_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def apply_limited(self, d_in: int, frames_capacity: int, d_out: int, out_capacity: int, d_gains: int, n_gains: int,
                      frames: Optional[Sequence[int]] = None, flush_mask: Optional[Sequence[int]] = None,
                      gain_of_stream: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels]) into the look-ahead limiter and write what it
        emits to d_out[s][0 ..) (f32 [n_streams][out_capacity][channels]): the frames taken limit_latency() frames earlier, scaled by
        the stream's gain and the limiter's envelope; with the stream flagged in flush_mask, everything it still holds.  Gains and
        gain_of_stream as apply_gains; the gain is read when a stream takes its first frame after a reset.  Returns the device pointer
        to omx_program_limit_record[n_streams] (LIMIT_RECORD_DTYPE); `frames_written` says how many frames each stream got."""
        fr = self._per_stream(frames, np.uint32, "frames")
        fl = self._per_stream(flush_mask, np.uint8, "flush_mask")
        gi = self._per_stream(gain_of_stream, np.uint32, "gain_of_stream")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_apply_limited", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                         C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(d_out or 0),
                         out_capacity, fl.ctypes.data if fl is not None else None, C.c_void_p(d_gains or 0), n_gains,
                         gi.ctypes.data if gi is not None else None, C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_limited(self, stream_index: int) -> np.ndarray:
        """One stream's limiter record as a LIMIT_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), LIMIT_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_limited", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_pcm.h
    def import_pcm(self, d_in: int, format: int, d_out: int, frames_capacity: int, channels: int,
                   frames: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """d_out[s][f][c] (f32) = the integer sample d_in[s][f][c] of `format` (PCM_S16 / PCM_S24 / PCM_S32, little-endian, rows of
        frames_capacity * channels samples without padding, base 4-byte aligned) scaled to [-1, 1), for f < frames[s], on `stream`.
        Out of place.  Returns 1 when any stream brought a frame, else 0."""
        fr = self._per_stream(frames, np.uint32, "frames")
        f = self.api.fn("program_loudness_bank_import_pcm", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p])
        return self.api.check(f(self._h, C.c_void_p(d_in or 0), format, C.c_void_p(d_out or 0), frames_capacity,
                                fr.ctypes.data if fr is not None else None, channels, C.c_void_p(stream or 0)))

    def configure_export(self, rule: ExportRule, channels: int):
        """Set the export's format, dither and seed and the channel count of the PCM it takes; allocates its records.  Only while every
        stream's export position is 0: a new bank, or after reset_export() of every stream."""
        c = rule.to_c()
        self.api.check(self.api.fn("program_loudness_bank_export_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])(
            self._h, C.byref(c), channels))

    def reset_export(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the export start over at dither position 0 with a zero record (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_export_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def export_pcm(self, d_in: int, d_out: int, frames_capacity: int, frames: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """d_out[s][f][c] (integer PCM of the configured format, base 4-byte aligned) = d_in[s][f][c] (f32) scaled, dithered at the
        stream's running position, rounded and clamped, for f < frames[s], on `stream`.  Out of place; no byte beyond a stream's
        frames is written.  Returns the device pointer to omx_program_export_record[n_streams] (EXPORT_RECORD_DTYPE)."""
        fr = self._per_stream(frames, np.uint32, "frames")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_export_pcm", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), C.c_void_p(d_out or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                         C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_exported(self, stream_index: int) -> np.ndarray:
        """One stream's export record as an EXPORT_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), EXPORT_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_exported", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_resample.h
    def configure_resampler(self, rule: ResampleRule, channels: int):
        """Set the resampler's rule and the channel count of the PCM it takes; builds its table and allocates its state.  Only while
        no stream of the resampler holds frames: a new bank, or after reset_resampler() of every stream."""
        c = rule.to_c()
        self.api.check(self.api.fn("program_loudness_bank_resampler_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])(
            self._h, C.byref(c), channels))

    def reset_resampler(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the resampler start over (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_resampler_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def resample(self, d_in: int, frames_capacity: int, d_out: int, out_capacity: int, frames: Optional[Sequence[int]] = None,
                 flush_mask: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels], at rate_in) and write the frames at rate_out
        that they complete to d_out[s][0 ..) (f32 [n_streams][out_capacity][channels]); with the stream flagged in flush_mask, the
        tail as well (the input continued with zeros).  resample_frames() says how many frames a call emits.  Out of place.  Returns
        the device pointer to omx_program_resample_record[n_streams] (RESAMPLE_RECORD_DTYPE); `frames_written` says how many frames
        each stream got."""
        fr = self._per_stream(frames, np.uint32, "frames")
        fl = self._per_stream(flush_mask, np.uint8, "flush_mask")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_resample", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(d_out or 0),
                         out_capacity, fl.ctypes.data if fl is not None else None, C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_resampled(self, stream_index: int) -> np.ndarray:
        """One stream's resampler record as a RESAMPLE_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), RESAMPLE_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_resampled", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_remix.h
    def configure_remix(self, matrices, channels_in: int, channels_out: int):
        """Upload the mixing matrices, one f32 [channels_out][channels_in] array or a stack [n][channels_out][channels_in], and
        allocate the records.  Allowed at any time; remix calls still enqueued are waited for before an earlier table goes."""
        m = np.ascontiguousarray(matrices, dtype=np.float32)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1:] != (channels_out, channels_in):
            raise ValueError(f"matrices: shape {m.shape} is neither [{channels_out}][{channels_in}] nor a stack of it")
        self.api.check(self.api.fn("program_loudness_bank_remix_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32])(
            self._h, channels_in, channels_out, m.ctypes.data if m.size else None, m.shape[0]))

    def remix(self, d_in: int, d_out: int, frames_capacity: int, frames: Optional[Sequence[int]] = None,
              matrix_of_stream: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """d_out[s][f][o] (f32 [n_streams][frames_capacity][channels_out]) = the mix of d_in[s][f][:] (f32
        [n_streams][frames_capacity][channels_in]) under the matrix of stream s, for f < frames[s], on `stream`.  matrix_of_stream[s]:
        the matrix of stream s, None: matrix 0 for every stream.  Out of place; no float beyond a stream's frames is written.  Returns
        the device pointer to omx_program_remix_record[n_streams] (REMIX_RECORD_DTYPE), written fresh by every call."""
        fr = self._per_stream(frames, np.uint32, "frames")
        mi = self._per_stream(matrix_of_stream, np.uint32, "matrix_of_stream")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_remix", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(d_out or 0),
                         mi.ctypes.data if mi is not None else None, C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_remixed(self, stream_index: int) -> np.ndarray:
        """One stream's record of the last remix call as a REMIX_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), REMIX_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_remixed", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_inspect.h
    def configure_inspect(self, rule: InspectRule, channels: int, pairs: Sequence[Sequence[int]] = ()):
        """Set the inspector's rule, the channel count of the PCM it takes and up to INSPECT_MAX_PAIRS channel pairs (a, b) whose
        correlation it keeps; allocates its records.  Only while no stream of the inspector holds frames: a new bank, or after
        reset_inspect() of every stream."""
        c = rule.to_c()
        pr = np.ascontiguousarray(np.asarray(list(pairs), dtype=np.uint32).reshape(-1, 2))
        self.api.check(self.api.fn("program_loudness_bank_inspect_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])(
            self._h, C.byref(c), channels, pr.ctypes.data if pr.size else None, pr.shape[0]))

    def reset_inspect(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the inspector start over with a zero record (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_inspect_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def inspect(self, d_in: int, frames_capacity: int, frames: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels]) into the running record of stream s, on
        `stream`; d_in is only read.  Returns the device pointer to omx_program_inspect_record[n_streams] (INSPECT_RECORD_DTYPE): the
        records run since the stream's reset and have the same bytes however the programme is cut into calls."""
        fr = self._per_stream(frames, np.uint32, "frames")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_inspect", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(stream or 0),
                         C.byref(out)))
        return out.value or 0

    def fetch_inspected(self, stream_index: int) -> np.ndarray:
        """One stream's running record as an INSPECT_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), INSPECT_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_inspected", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_filter.h
    def configure_filter(self, filters, channels: int, sample_rate: float, filter_of_channel=None):
        """Set the filter table (see filter_table), the channel count and the rate of the PCM the filter stage takes, and which filter
        every channel runs: filter_of_channel [n_streams][channels] of table indices or FILTER_BYPASS, None: filter 0 everywhere.
        Builds the tables of the time-parallel form, allocates state and records and resets every stream.  Only while no stream
        holds filter state: a new bank, or after reset_filter() of every stream."""
        table = filter_table(filters)
        foc = None
        if filter_of_channel is not None:
            foc = np.ascontiguousarray(filter_of_channel, np.uint32).reshape(-1)
            if foc.size != self.n_streams * channels:
                raise ValueError(f"filter_of_channel: {foc.size} entries for {self.n_streams} streams of {channels} channels")
        self.api.check(self.api.fn("program_loudness_bank_filter_configure", C.c_int,
                                   [C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p])(
            self._h, channels, sample_rate, table.ctypes.data if table.size else None, table.size, foc.ctypes.data if foc is not None else None))

    def reset_filter(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the filter stage start over with zero state and a zero record (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_filter_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def filter(self, d_in: int, d_out: int, frames_capacity: int, frames: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """d_out[s][f][c] = d_in[s][f][c] through the filter of channel c of stream s, for f < frames[s], on `stream`; both f32
        [n_streams][frames_capacity][channels].  d_out == d_in filters in place; no float beyond a stream's frames is written.
        Returns the device pointer to omx_program_filter_record[n_streams] (FILTER_RECORD_DTYPE), written fresh by every call."""
        fr = self._per_stream(frames, np.uint32, "frames")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_filter", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(d_out or 0),
                         C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_filtered(self, stream_index: int) -> np.ndarray:
        """One stream's record of the last filter call as a FILTER_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), FILTER_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_filtered", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    def set_filter_form(self, form: int):
        """0 = by call shape, 1 = reference order, 2 = time-parallel, for filter() alone."""
        self.api.check(self.api.fn("program_loudness_bank_filter_set_form", C.c_int, [C.c_void_p, C.c_uint32])(self._h, form))

    def last_filter_form(self) -> int:
        """1 = the last filter call ran in reference order, 2 = in the time-parallel form, 0 = none yet."""
        return self.api.fn("debug_program_loudness_bank_filter_last_form", C.c_int, [C.c_void_p])(self._h)

    # ---- include/omx/program_edit.h
    def configure_edit(self, channels: int, max_outputs: int):
        """Set the channel count of the PCM the edit pass takes and the largest number of output streams of a call; allocates the
        records and uploads the curve tables.  Allowed at any time; edit calls still enqueued are waited for."""
        self.api.check(self.api.fn("program_loudness_bank_edit_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32])(
            self._h, channels, max_outputs))

    def edit(self, d_in: int, frames_capacity: int, clips, d_out: int, out_capacity: int, out_frames: Sequence[int],
             out_first: Optional[Sequence[int]] = None, frames_in: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Render the clip table (a sequence of EditClip or an EDIT_CLIP_DTYPE array, sorted by (dst_stream, dst_first)) from d_in (f32
        [n_streams][frames_capacity][channels]; frames_in[s]: the frames stream s holds, None: the whole row) into d_out (f32
        [len(out_frames)][out_capacity][channels]) on `stream`: output frames [out_first[o], out_first[o] + out_frames[o]) of output
        stream o land at d_out[o][0 ..]; out_first None: 0.  Out of place; no float beyond a window is written.  Returns the device
        pointer to omx_program_edit_record[max_outputs] (EDIT_RECORD_DTYPE), entries below len(out_frames) written fresh by every call."""
        table = edit_table(clips)
        fr = self._per_stream(frames_in, np.uint32, "frames_in")
        of = np.ascontiguousarray(out_frames, np.uint32).reshape(-1)
        first = None if out_first is None else np.ascontiguousarray(out_first, np.uint64).reshape(-1)
        if first is not None and first.size != of.size:
            raise ValueError(f"out_first: {first.size} entries for {of.size} outputs")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_edit", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                         table.ctypes.data if table.size else None, table.size, C.c_void_p(d_out or 0), out_capacity, of.size,
                         first.ctypes.data if first is not None else None, of.ctypes.data if of.size else None, C.c_void_p(stream or 0),
                         C.byref(out)))
        return out.value or 0

    def fetch_edited(self, output_index: int) -> np.ndarray:
        """One output's record of the last edit call as an EDIT_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), EDIT_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_edited", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, output_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_mix.h
    def configure_mix(self, channels: int, max_buses: int):
        """Set the channel count of the PCM the mix pass takes and the largest number of buses of a call; allocates the records.
        Allowed at any time; mix calls still enqueued are waited for."""
        self.api.check(self.api.fn("program_loudness_bank_mix_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32])(
            self._h, channels, max_buses))

    def mix(self, d_in: int, frames_capacity: int, sends, d_out: int, out_capacity: int, out_frames: Sequence[int],
            out_first: Optional[Sequence[int]] = None, frames_in: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Render the send table (a sequence of MixSend or a MIX_SEND_DTYPE array, sorted by (dst_bus, dst_first)) from d_in (f32
        [n_streams][frames_capacity][channels]; frames_in[s]: the frames stream s holds, None: the whole row) into d_out (f32
        [len(out_frames)][out_capacity][channels]) on `stream`: bus frames [out_first[o], out_first[o] + out_frames[o]) of bus o land
        at d_out[o][0 ..]; out_first None: 0.  Up to 64 sends over a frame are summed in f64 in table order and rounded once.  Out of
        place; no float beyond a window is written.  Returns the device pointer to omx_program_mix_record[max_buses]
        (MIX_RECORD_DTYPE), entries below len(out_frames) written fresh by every call."""
        table = mix_table(sends)
        fr = self._per_stream(frames_in, np.uint32, "frames_in")
        of = np.ascontiguousarray(out_frames, np.uint32).reshape(-1)
        first = None if out_first is None else np.ascontiguousarray(out_first, np.uint64).reshape(-1)
        if first is not None and first.size != of.size:
            raise ValueError(f"out_first: {first.size} entries for {of.size} buses")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_mix", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                         table.ctypes.data if table.size else None, table.size, C.c_void_p(d_out or 0), out_capacity, of.size,
                         first.ctypes.data if first is not None else None, of.ctypes.data if of.size else None, C.c_void_p(stream or 0),
                         C.byref(out)))
        return out.value or 0

    def fetch_mixed(self, bus: int) -> np.ndarray:
        """One bus's record of the last mix call as a MIX_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), MIX_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_mixed", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, bus, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_convolve.h
    def configure_convolve(self, firs, channels: int, fir_of_channel=None, delay_frames: int = 0):
        """Set the FIR table (a sequence of f32 tap sequences), the channel count of the PCM the convolve stage takes, which FIR
        every channel runs (fir_of_channel [n_streams][channels] of table indices or CONVOLVE_BYPASS, None: FIR 0 everywhere) and
        the compensated delay D in frames, at most the longest referenced FIR's taps minus one; (T - 1) / 2 leaves a symmetric FIR's
        output in place.  Only while no stream of the stage holds frames: a new bank, or after reset_convolve() of every stream."""
        table, _keep = _fir_table(firs)
        foc = None
        if fir_of_channel is not None:
            foc = np.ascontiguousarray(fir_of_channel, np.uint32).reshape(-1)
            if foc.size != self.n_streams * channels:
                raise ValueError(f"fir_of_channel: {foc.size} entries for {self.n_streams} streams of {channels} channels")
        self.api.check(self.api.fn("program_loudness_bank_convolve_configure", C.c_int,
                                   [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])(
            self._h, channels, table if len(firs) else None, len(firs), foc.ctypes.data if foc is not None else None, delay_frames))

    def reset_convolve(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the convolve stage forget their frames and are idle again (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_convolve_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def convolve(self, d_in: int, frames_capacity: int, d_out: int, out_capacity: int, frames: Optional[Sequence[int]] = None,
                 flush_mask: Optional[Sequence[int]] = None, stream: int = 0) -> int:
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels]) and write the output frames they complete to
        d_out[s][0 ..) (f32 [n_streams][out_capacity][channels]); with the stream flagged in flush_mask, the tail as well (the input
        continued with zeros).  convolve_frames() says how many frames a call emits.  Out of place.  Returns the device pointer to
        omx_program_convolve_record[n_streams] (CONVOLVE_RECORD_DTYPE); `frames_written` says how many frames each stream got."""
        fr = self._per_stream(frames, np.uint32, "frames")
        fl = self._per_stream(flush_mask, np.uint8, "flush_mask")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_convolve", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None, C.c_void_p(d_out or 0),
                         out_capacity, fl.ctypes.data if fl is not None else None, C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_convolved(self, stream_index: int) -> np.ndarray:
        """One stream's convolve record as a CONVOLVE_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), CONVOLVE_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_convolved", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_dynamics.h
    def configure_dynamics(self, curves, channels: int, curve_of_stream: Optional[Sequence[int]] = None):
        """Set the curve table (a sequence of DynamicsCurve), the channel count of the PCM the dynamics stage takes and which curve
        every stream runs (table indices or DYNAMICS_BYPASS, None: curve 0 everywhere).  A stream's latency is its curve's
        attack_frames - 1; a bypassed stream is delayed by the largest latency of the table.  Only while no stream of the stage
        holds frames: a new bank, or after reset_dynamics() of every stream."""
        curves = list(curves)
        table = (CProgramDynamicsCurve * max(len(curves), 1))()
        for k, c in enumerate(curves):
            table[k] = _dynamics_c(c)
        cos = self._per_stream(curve_of_stream, np.uint32, "curve_of_stream")
        self.api.check(self.api.fn("program_loudness_bank_dynamics_configure", C.c_int,
                                   [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])(
            self._h, channels, table if curves else None, len(curves), cos.ctypes.data if cos is not None else None))

    def reset_dynamics(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the dynamics stage forget their frames and their history and are idle again (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_dynamics_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def dynamics(self, d_in: int, frames_capacity: int, d_out: int, out_capacity: int, frames: Optional[Sequence[int]] = None,
                 flush_mask: Optional[Sequence[int]] = None, d_key: int = 0, d_gain_db: int = 0, stream: int = 0) -> int:
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels]), with the level taken from d_key (same layout;
        0: from d_in), and write the frames they complete, under the gain of each stream's curve, to d_out[s][0 ..) (f32 [n_streams]
        [out_capacity][channels]) and their gains in dB to d_gain_db[s][0 ..) (f32 [n_streams][out_capacity]; 0: no trace); with the
        stream flagged in flush_mask, the held frames as well.  dynamics_frames() says how many frames a call emits.  Out of place.
        Returns the device pointer to omx_program_dynamics_record[n_streams] (DYNAMICS_RECORD_DTYPE); `frames_written` says how many
        frames each stream got."""
        fr = self._per_stream(frames, np.uint32, "frames")
        fl = self._per_stream(flush_mask, np.uint8, "flush_mask")
        out = C.c_void_p()
        f = self.api.fn("program_loudness_bank_dynamics", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                         C.c_void_p, C.POINTER(C.c_void_p)])
        self.api.check(f(self._h, C.c_void_p(d_in or 0), C.c_void_p(d_key or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                         C.c_void_p(d_out or 0), C.c_void_p(d_gain_db or 0), out_capacity, fl.ctypes.data if fl is not None else None,
                         C.c_void_p(stream or 0), C.byref(out)))
        return out.value or 0

    def fetch_dynamics(self, stream_index: int) -> np.ndarray:
        """One stream's dynamics record as a DYNAMICS_RECORD_DTYPE scalar; synchronises."""
        out = np.zeros((1,), DYNAMICS_RECORD_DTYPE)
        self.api.check(self.api.fn("program_loudness_bank_fetch_dynamics", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(
            self._h, stream_index, out.ctypes.data))
        return out[0]

    # ---- include/omx/program_spectrum.h
    def configure_spectrum(self, rule: SpectrumRule, channels: int):
        """Set the rule and the channel count of the PCM the spectrum stage takes; allocates its records, sums and carried frames and
        resets every stream.  Only while no stream of the stage holds frames: a new bank, or after reset_spectrum() of every
        stream."""
        c = rule.to_c()
        self.api.check(self.api.fn("program_loudness_bank_spectrum_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])(
            self._h, C.byref(c), channels))
        self._spectrum_shape = (channels, rule.fft_size // 2 + 1)

    def reset_spectrum(self, reset_mask: Optional[Sequence[int]] = None):
        """The flagged streams of the spectrum stage start over with a zero record and zero sums (None: every stream)."""
        mask = self._per_stream(reset_mask, np.uint8, "reset_mask")
        self.api.check(self.api.fn("program_loudness_bank_spectrum_reset", C.c_int, [C.c_void_p, C.c_void_p])(
            self._h, mask.ctypes.data if mask is not None else None))

    def spectrum(self, d_in: int, frames_capacity: int, frames: Optional[Sequence[int]] = None,
                 finish_mask: Optional[Sequence[int]] = None, stream: int = 0):
        """Take frames[s] frames of d_in[s] (f32 [n_streams][frames_capacity][channels]) into the long-term spectrum of stream s, on
        `stream`; d_in is only read.  A stream flagged in finish_mask completes its open transforms with zeros and takes no more
        frames until reset_spectrum().  Returns (status, d_records, d_sums): status 1 when any stream brought a frame or was
        finished, the device pointers to omx_program_spectrum_record[n_streams] (SPECTRUM_RECORD_DTYPE) and to the sums, f64
        [n_streams][channels][fft_size / 2 + 1].  Both have the same bytes however the programme is cut into calls."""
        fr = self._per_stream(frames, np.uint32, "frames")
        fin = self._per_stream(finish_mask, np.uint8, "finish_mask")
        rec, sums = C.c_void_p(), C.c_void_p()
        f = self.api.fn("program_loudness_bank_spectrum", C.c_int,
                        [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
        status = self.api.check(f(self._h, C.c_void_p(d_in or 0), frames_capacity, fr.ctypes.data if fr is not None else None,
                                  fin.ctypes.data if fin is not None else None, C.c_void_p(stream or 0), C.byref(rec), C.byref(sums)))
        return status, rec.value or 0, sums.value or 0

    def fetch_spectrum(self, stream_index: int):
        """One stream's running record (a SPECTRUM_RECORD_DTYPE scalar) and its sums, f64 [channels][fft_size / 2 + 1]; synchronises."""
        channels, bins = getattr(self, "_spectrum_shape", (1, 1))
        rec, sums = np.zeros((1,), SPECTRUM_RECORD_DTYPE), np.zeros((channels, bins), np.float64)
        self.api.check(self.api.fn("program_loudness_bank_fetch_spectrum", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p])(
            self._h, stream_index, rec.ctypes.data, sums.ctypes.data))
        return rec[0], sums

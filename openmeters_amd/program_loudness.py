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

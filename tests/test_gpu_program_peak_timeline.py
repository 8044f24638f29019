"""Programme bank peak timeline on the GPU (`-m gpu`): ProgramLoudnessBank.set_peak_timeline / peak_rows / *_interval_peaks /
*_group_peaks / plan_part_gains (include/omx/program_peak_timeline.h) against the frame-by-frame numpy restatement
(tests/program_peak_timeline_ref.py, pinned by tests/test_cpu_program_peak_timeline.py).

Bars: every comparison against the restatement is on BYTES (linear peaks, offsets, frame numbers, members, counts), except the dB
fields, which hold the 1e-4 dB bar of the peak tests (numpy's f32 log stands in for logf); results of the same programme cut into
calls in different ways are bitwise equal in every field.  None of these cases can pass without the feature."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_peak_timeline_ref as ref
import program_peaks_ref as pref
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (GAIN_LIMIT_PEAK, PART_PEAK_DTYPE, PEAK_ROW_DTYPE, TO_END, GainRule, ProgramLoudnessBank,
                                             evaluate_gain)
from parity import bar

pytestmark = pytest.mark.gpu
BAR = 1e-4
FLOOR = -99.9
F32_FLOOR = np.float32(FLOOR)
PREFIX = "program loudness peak timeline: "
COEFFS = ref.coefficients()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


def new_bank(omx, fs, n_streams, ch, capacity_seconds=60, timeline=True, peaks=True):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n_streams, ch, capacity_seconds)
    if peaks:
        bank.set_peaks(True)
    if timeline:
        bank.set_peak_timeline(True)
    return bank


def feed(torch, bank, xs, fs, ch, schedule, resets=None, cursor=None):
    """schedule: per call an array of per-stream frame counts; every stream walks its own programme from `cursor`"""
    pos = capi.positions_fallback(ch)
    cursor = cursor if cursor is not None else [0] * len(xs)
    for k, counts in enumerate(schedule):
        cap = max(int(max(counts)), 1)
        host = np.zeros((len(xs), cap, ch), np.float32)
        for s, n in enumerate(counts):
            host[s, :n] = xs[s][cursor[s]:cursor[s] + int(n)]
            cursor[s] += int(n)
        d = torch.from_numpy(host).cuda()
        bank.process(d.data_ptr(), cap, ch, fs, pos, frames=np.asarray(counts, np.uint32), reset_mask=resets[k] if resets else None,
                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return bank


def whole(xs):
    return [np.array([len(x) for x in xs], np.uint32)]


def cut_at(n, cuts):
    """call lengths that cut a programme of n frames at the given positions"""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < n)) + [n]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def device_bytes(ptr, n):
    """n bytes of device memory at `ptr`, through the HIP runtime the process has already loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    raw = (C.c_uint8 * n)()
    copy = C.CDLL(path).hipMemcpy
    copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert copy(raw, C.c_void_p(ptr), n, 2) == 0      # 2 = device to host
    return bytes(raw)


def device_rows(torch, bank, first, stride, count):
    """bank.peak_rows into device memory: [n_streams][count] rows"""
    d = torch.full((max(bank.n_streams * count * PEAK_ROW_DTYPE.itemsize, 1),), 0xA5, dtype=torch.uint8).cuda()
    status = bank.peak_rows(d.data_ptr(), first, stride, count, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == (1 if count else 0)
    return d.cpu().numpy()[:bank.n_streams * count * PEAK_ROW_DTYPE.itemsize].view(PEAK_ROW_DTYPE).reshape(bank.n_streams, count)


def same_parts(got, want, tag):
    """part peaks against the restatement: bytes but for the dB fields, those within the bar"""
    g, gdb = ref.split_db(got)
    w, wdb = ref.split_db(want)
    assert g.tobytes() == w.tobytes(), (tag, got, want)
    worst = 0.0
    for a, b in zip(gdb.ravel(), wdb.ravel()):
        d = 0.0 if a == b else abs(a - b)       # (an infinite peak: inf on both sides)
        worst = max(worst, bar("program peak timeline: |d dB field| dB", d, BAR, (tag, a, b)))
    return worst


def check_identity(bank, s, L, tag):
    """interval [0, segments) joined with the open row = fetch_peaks, in value and in frame number, for every channel"""
    rec, loud = bank.fetch_peaks(s), bank.fetch(s)
    assert rec.frames == loud.frames
    part = bank.fetch_interval_peaks([(s, 0, TO_END)])[0]
    assert part["frames"] == loud.segments * L
    open_row = bank.fetch_peak_rows(s, loud.segments, 1, 1)[0]
    assert bool(open_row["valid"]) == (rec.frames > loud.segments * L) and open_row["frames"] == rec.frames - loud.segments * L
    for c in range(8):
        for kind in ("true_peak", "sample_peak"):
            value, frame = part[kind][c], int(part[kind + "_frame"][c])
            if open_row[kind][c] > value:
                value, frame = open_row[kind][c], loud.segments * L + int(open_row[kind + "_offset"][c])
            assert value.tobytes() == getattr(rec, kind)[c].tobytes() and frame == int(getattr(rec, kind + "_frame")[c]), (tag, s, c, kind)


def check_stream(bank, s, x, fs, tag, extra_rows=2):
    """rows, the whole-interval peak and the identity of one stream against the restatement of the frames it holds"""
    sp = ref.segment_peaks(x, fs, COEFFS)
    n = len(sp["true_peak"]) + extra_rows
    got = bank.fetch_peak_rows(s, 0, 1, n)
    assert got.tobytes() == ref.rows(sp, 0, 1, n).tobytes(), (tag, s)
    same_parts(bank.fetch_interval_peaks([(s, 0, TO_END)]), ref.part_peaks([sp], [(0, 0, TO_END)], None, FLOOR), (tag, s))
    check_identity(bank, s, sp["L"], tag)
    return sp


@pytest.mark.parametrize("fs,ch", [(3364.0, 1), (3364.0, 8), (8000.0, 3), (44100.0, 2), (44100.0, 6), (48000.0, 1), (48000.0, 2),
                                   (48000.0, 8), (96000.0, 2), (96000.0, 3), (192000.0, 2), (192000.0, 6)])
def test_rows_are_bit_exact_against_the_restatement(torch_dev, omx, fs, ch):
    """seven streams of one bank, one ragged call: 0, 1, L - 1, L, L + 1 and 3 L + 5 frames and one that crosses several 1024-frame
    tiles and segments, programmes with NaN, infinities, -0.0 and denormals.  3364 Hz: L = 336, five segments per tile; 96 kHz: the 2x
    interpolator; 192 kHz: none"""
    L = ref.segment_frames(fs)
    lengths = [0, 1, L - 1, L, L + 1, 3 * L + 5, max(4 * 1024 + 77, 2 * L + 1024 + 13)]
    xs = [ref.hard_programme(10 * ch + s, n, ch) for s, n in enumerate(lengths)]
    bank = feed(torch_dev, new_bank(omx, fs, len(xs), ch), xs, fs, ch, whole(xs))
    most = max(lengths) // L + 3
    on_device = device_rows(torch_dev, bank, 0, 1, most)
    for s, x in enumerate(xs):
        sp = check_stream(bank, s, x, fs, (fs, ch, lengths[s]))
        assert on_device[s].tobytes() == ref.rows(sp, 0, 1, most).tobytes(), (fs, ch, s)
        assert len(sp["true_peak"]) == -(-lengths[s] // L)
    assert np.isinf(on_device[6]["true_peak"][:, 0]).any() and np.isfinite(on_device[6]["true_peak"]).any()


@pytest.mark.parametrize("fs,ch", [(48000.0, 2), (3364.0, 3), (96000.0, 1), (192000.0, 2)])
def test_the_cut_does_not_matter(torch_dev, omx, fs, ch):
    """the same programme whole, in single frames across a segment boundary, cut at L - 1, L, L + 1, 1023, 1024, 1025 and 16, and cut at
    random points: rows and part peaks have equal bytes (and the rows equal the restatement)"""
    L = ref.segment_frames(fs)
    n = 3 * L + 1500
    x = ref.hard_programme(77 + ch, n, ch)
    rng = np.random.default_rng(5)
    schedules = {
        "whole": [n],
        "single frames across a boundary": cut_at(n, [L - 3, L - 2, L - 1, L, L + 1, L + 2, L + 3]),
        "L - 1": cut_at(n, [L - 1]), "L": cut_at(n, [L]), "L + 1": cut_at(n, [L + 1]),
        "1023": cut_at(n, [1023]), "1024": cut_at(n, [1024]), "1025": cut_at(n, [1025]), "16": cut_at(n, [16]),
        "random": cut_at(n, rng.integers(1, n, 9).tolist()),
    }
    members = [(0, 0, TO_END), (0, 1, 2), (0, 2, 1)]
    groups = [(0, 3), (1, 2)]
    got = {}
    for name, lengths in schedules.items():
        assert sum(lengths) == n
        bank = feed(torch_dev, new_bank(omx, fs, 1, ch), [x], fs, ch, [np.array([k], np.uint32) for k in lengths])
        got[name] = (bank.fetch_peak_rows(0, 0, 1, 6).tobytes(), bank.fetch_peak_rows(0, 0, 3, 2).tobytes(),
                     bank.fetch_interval_peaks(members).tobytes(), bank.fetch_group_peaks(members, groups).tobytes())
    sp = ref.segment_peaks(x, fs, COEFFS)
    assert got["whole"][0] == ref.rows(sp, 0, 1, 6).tobytes() and got["whole"][1] == ref.rows(sp, 0, 3, 2).tobytes()
    for name in schedules:
        assert got[name] == got["whole"], name


@pytest.mark.parametrize("fs", [48000.0, 96000.0])
def test_bursts_on_segment_tile_and_run_boundaries(torch_dev, omx, fs):
    """one impulse per stream: on the last frame of a segment, on the first of the next, on the last frame of a tile and the first of the
    next, on frames 15 and 16 of a run; offsets exact.  An impulse at a segment's end puts its tail into the next segment's true peak
    only"""
    L = ref.segment_frames(fs)
    n = 2 * L + 100
    places = [L - 1, L, 1023, 1024, 2048 + 15, 2048 + 16, 2 * L - 1, n - 1]
    xs = []
    for p in places:
        x = np.zeros((n, 1), np.float32)
        x[p, 0] = -0.5
        xs.append(x)
    for schedule in (whole(xs), [np.array([p + 1] * len(xs), np.uint32) for p in (L - 1,)] + [np.array([n - L] * len(xs), np.uint32)]):
        bank = feed(torch_dev, new_bank(omx, fs, len(xs), 1), xs, fs, 1, schedule)
        for s, p in enumerate(places):
            check_stream(bank, s, xs[s], fs, (fs, p))
            rows = bank.fetch_peak_rows(s, 0, 1, 3)
            j = p // L
            assert rows[j]["sample_peak"][0] == 0.5 and rows[j]["sample_peak_offset"][0] == p - j * L, (fs, p)
            assert [r["sample_peak"][0] for r in rows].count(0.5) == 1
        tail = bank.fetch_peak_rows(0, 0, 1, 2)        # the impulse on frame L - 1
        assert tail[0]["true_peak"][0] == 0.5 and tail[0]["true_peak_offset"][0] == L - 1
        assert 0 < tail[1]["true_peak"][0] < 0.5 and tail[1]["sample_peak"][0] == 0 and tail[1]["sample_peak_offset"][0] == 0
        assert tail[1]["true_peak_offset"][0] == (4 if fs < 96000 else 10)   # the largest tap sits 5 / 11 frames behind the sample


def test_ties_and_silence(torch_dev, omx):
    """equal peaks in two segments: the earliest frame wins in a row over both; equal peaks in two members: the first member in table
    order wins, within it the earliest frame; an all-zero programme has peaks of 0 and offsets of 0"""
    fs, ch = 48000.0, 2
    L = ref.segment_frames(fs)
    x = np.zeros((4 * L, ch), np.float32)
    for p in (L + 9, L + 700, 3 * L + 2):
        x[p:p + 3, 0] = 0.25                     # the same burst three times: equal true peaks and sample peaks
    x[2 * L + 5, 1] = x[5, 1] = -0.125
    xs = [x, np.zeros((2 * L + 7, ch), np.float32)]
    bank = feed(torch_dev, new_bank(omx, fs, 2, ch), xs, fs, ch, whole(xs))
    sps = [check_stream(bank, s, xs[s], fs, "ties") for s in range(2)]
    row = bank.fetch_peak_rows(0, 0, 4, 1)[0]
    assert row["sample_peak_offset"][0] == L + 9 and row["sample_peak_offset"][1] == 5 and row["true_peak"][0] > 0.25
    assert L + 9 <= row["true_peak_offset"][0] < L + 9 + 12
    members = [(0, 3, 1), (0, 1, 1), (0, 2, 1), (0, 0, 1), (0, 1, 1)]
    groups = [(0, 2), (1, 4), (1, 1)]
    got = bank.fetch_group_peaks(members, groups)
    same_parts(got, ref.part_peaks(sps, members, groups, FLOOR), "tied members")
    assert got[0]["sample_peak_member"][0] == 0 and got[0]["sample_peak_frame"][0] == 3 * L + 2       # first in table order, later in time
    assert got[1]["sample_peak_member"][0] == 0 and got[1]["sample_peak_frame"][0] == L + 9           # of the twice-listed part, the first
    assert got[1]["sample_peak_member"][1] == 1 and got[1]["sample_peak_frame"][1] == 2 * L + 5
    silent = bank.fetch_peak_rows(1, 0, 1, 3)
    assert silent["valid"].tolist() == [1, 1, 1] and silent["frames"].tolist() == [L, L, 7]
    for f in ("true_peak", "sample_peak", "true_peak_offset", "sample_peak_offset"):
        assert not silent[f].any()
    part = bank.fetch_interval_peaks([(1, 0, TO_END)])[0]
    assert part["frames"] == 2 * L and part["channels"] == ch and not part["true_peak"].any() and not part["true_peak_frame"].any()
    assert (part["true_peak_db"] == F32_FLOOR).all() and part["max_true_peak_db"] == F32_FLOOR and part["max_true_peak_channel"] == 0


def test_ragged_calls_resets_and_overflow(torch_dev, omx):
    """ragged calls with streams that bring 0 frames, a reset_mask inside a call while the neighbours go on (the rows of the reset
    stream start again from zero), reset() between calls, and overflow at capacity_seconds = 1; the identity holds throughout"""
    fs, ch = 48000.0, 2
    L = ref.segment_frames(fs)
    xs = [ref.hard_programme(40 + s, 5 * L + 333, ch) for s in range(3)]
    bank = new_bank(omx, fs, 3, ch)
    cursor = [0, 0, 0]
    feed(torch_dev, bank, xs, fs, ch, [np.array([L + 10, 0, 2 * L + 1], np.uint32), np.array([0, 17, L - 1], np.uint32)], cursor=cursor)
    for s in range(3):
        check_stream(bank, s, xs[s][:cursor[s]], fs, ("ragged", s))
    # stream 2 is reset by the mask of this call, before its samples are taken; stream 1 brings nothing; stream 0 goes on
    at = cursor[2]
    feed(torch_dev, bank, xs, fs, ch, [np.array([L, 0, L + 40], np.uint32)], resets=[[0, 0, 1]], cursor=cursor)
    check_stream(bank, 0, xs[0][:cursor[0]], fs, "goes on")
    check_stream(bank, 1, xs[1][:cursor[1]], fs, "no frames")
    check_stream(bank, 2, xs[2][at:cursor[2]], fs, "reset by the call's mask", extra_rows=4)
    feed(torch_dev, bank, xs, fs, ch, [np.array([0, 0, L + 7], np.uint32)], cursor=cursor)   # into a segment it held before the reset
    check_stream(bank, 2, xs[2][at:cursor[2]], fs, "goes on after the reset", extra_rows=4)
    before = bank.fetch_peak_rows(2, 0, 1, 4).tobytes()
    bank.reset([1, 0, 0])
    assert not bank.fetch_peak_rows(0, 0, 1, 4)["valid"].any() and bank.fetch_peak_rows(0, 0, 1, 4).tobytes() == bytes(4 * 136)
    assert bank.fetch_peak_rows(2, 0, 1, 4).tobytes() == before
    check_identity(bank, 0, L, "after reset()")
    at = cursor[0]
    feed(torch_dev, bank, xs, fs, ch, [np.array([L // 2, 0, 0], np.uint32)], cursor=cursor)
    check_stream(bank, 0, xs[0][at:cursor[0]], fs, "starts over after reset()", extra_rows=4)
    # capacity 1 s = 10 segments: the peaks cover the stored part only
    y = ref.hard_programme(50, 11 * L + 9, ch)
    small = feed(torch_dev, new_bank(omx, fs, 1, ch, capacity_seconds=1), [y], fs, ch, [np.array([k], np.uint32) for k in cut_at(len(y), [4 * L + 1, 9 * L + 500])])
    assert small.fetch(0).overflow and small.fetch(0).frames == 10 * L
    check_stream(small, 0, y[:10 * L], fs, "overflow")


def test_aggregated_rows(torch_dev, omx):
    """strides 1, 3 and 10, windows beyond the end (invalid rows), `first` inside the programme, before and after a later append: a row
    of complete segments keeps its bytes"""
    fs, ch = 8000.0, 3
    L = ref.segment_frames(fs)
    x = ref.hard_programme(60, 23 * L + 11, ch)
    first_part = 12 * L + 400
    bank = feed(torch_dev, new_bank(omx, fs, 1, ch), [x], fs, ch, [np.array([first_part], np.uint32)])
    sp = ref.segment_peaks(x[:first_part], fs, COEFFS)
    early = {}
    for first, stride, count in ((0, 1, 15), (0, 3, 6), (0, 10, 3), (5, 3, 4), (7, 10, 2), (13, 1, 2), (40, 10, 2)):
        got = bank.fetch_peak_rows(0, first, stride, count)
        assert got.tobytes() == ref.rows(sp, first, stride, count).tobytes(), (first, stride, count)
        early[(first, stride, count)] = got
    assert early[(0, 3, 6)]["valid"].tolist() == [1, 1, 1, 1, 1, 0] and early[(0, 10, 3)]["frames"].tolist() == [10 * L, 2 * L + 400, 0]
    feed(torch_dev, bank, [x], fs, ch, [np.array([len(x) - first_part], np.uint32)], cursor=[first_part])
    sp = ref.segment_peaks(x, fs, COEFFS)
    for (first, stride, count), before in early.items():
        got = bank.fetch_peak_rows(0, first, stride, count)
        assert got.tobytes() == ref.rows(sp, first, stride, count).tobytes(), (first, stride, count)
        for i in range(count):
            if first + (i + 1) * stride <= 12:       # a row of segments that were complete before the append
                assert got[i].tobytes() == before[i].tobytes(), (first, stride, i)
    assert device_rows(torch_dev, bank, 5, 3, 4)[0].tobytes() == bank.fetch_peak_rows(0, 5, 3, 4).tobytes()


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_rows_up_to_the_last_frame_without_a_count(torch_dev, omx, fs):
    """fetch_peak_rows with no count: every row up to the stream's last frame, the open segment included, for streams whose open
    segment holds most of a segment, half of one, a single frame, nothing (a whole number of segments), everything (no complete
    segment yet) and for a stream without frames; with `first` inside the programme and strides 1, 3 and 10"""
    ch = 2
    L = ref.segment_frames(fs)
    lengths = [2 * L + (5 * L) // 6, 2 * L + L // 2, 7 * L + 1, 3 * L, L - 1, 1, 0, 23 * L + L // 3]
    xs = [ref.hard_programme(90 + s, n, ch) for s, n in enumerate(lengths)]
    bank = feed(torch_dev, new_bank(omx, fs, len(xs), ch), xs, fs, ch, whole(xs))
    for s, x in enumerate(xs):
        sp = ref.segment_peaks(x, fs, COEFFS)
        segments = -(-lengths[s] // L)
        assert len(sp["true_peak"]) == segments
        for first, stride in ((0, 1), (1, 1), (2, 1), (3, 1), (0, 3), (1, 3), (2, 3), (0, 10), (5, 10), (segments, 1), (segments + 4, 3)):
            got = bank.fetch_peak_rows(s, first, stride)
            count = max(-(-(segments - first) // stride), 0)        # rows with at least one segment that exists
            assert len(got) == count, (fs, s, first, stride)
            assert got.tobytes() == ref.rows(sp, first, stride, count).tobytes(), (fs, s, first, stride)
            assert got["valid"].all()
            if count and first == 0:
                assert got["frames"].sum() == lengths[s]            # the open segment's frames are in the last row
        assert bank.fetch_peak_rows(s).tobytes() == bank.fetch_peak_rows(s, 0, 1, segments).tobytes()


def test_a_reset_clears_a_long_stream_and_nothing_else(torch_dev, omx):
    """a stream with more stored keys than one run of the clear pass (1100 segments x 8 channels x 2 kinds) is reset by a call's mask
    and fed silence of the same length: every row reads 0, so no key of before the reset is left, while its neighbours, one before
    and one behind it in the bank, keep the bytes of their rows and go on"""
    fs, ch = 3364.0, 8
    L = ref.segment_frames(fs)
    n, short = 1100 * L + 7, 3 * L + 5
    rng = np.random.default_rng(77)
    xs = [ref.hard_programme(95, 2 * short, ch), (0.25 * rng.standard_normal((n, ch))).astype(np.float32), ref.hard_programme(96, 2 * short, ch)]
    bank = new_bank(omx, fs, 3, ch, capacity_seconds=120)
    cursor = [0, 0, 0]
    feed(torch_dev, bank, xs, fs, ch, [np.array([short, n, short], np.uint32)], cursor=cursor)
    rows = bank.fetch_peak_rows(1)
    assert len(rows) == 1101 and (rows["true_peak"][:, :ch] > 0).all() and rows["frames"][-1] == 7
    kept = [bank.fetch_peak_rows(s, 0, 1, 3).tobytes() for s in (0, 2)]
    xs[1] = np.zeros((n, ch), np.float32)
    cursor[1] = 0
    feed(torch_dev, bank, xs, fs, ch, [np.array([short, n, short], np.uint32)], resets=[[0, 1, 0]], cursor=cursor)
    rows = bank.fetch_peak_rows(1)
    assert len(rows) == 1101 and rows["valid"].all() and rows["frames"].sum() == n
    for field in ("true_peak", "sample_peak", "true_peak_offset", "sample_peak_offset"):
        assert not rows[field].any(), field
    for s, before in zip((0, 2), kept):
        assert bank.fetch_peak_rows(s, 0, 1, 3).tobytes() == before
        check_stream(bank, s, xs[s], fs, ("beside the reset", s))
    check_identity(bank, 1, L, "silence after the reset")


def test_interval_and_group_peaks(torch_dev, omx):
    """overlapping groups, a stream that appears twice, OMX_PROGRAM_TO_END, an empty group, a group of one member (the bytes of the
    interval), the device arrays against the fetch functions"""
    fs, ch = 44100.0, 6
    L = ref.segment_frames(fs)
    xs = [pref.programme(20 + s, fs, ch, seconds).astype(np.float32) for s, seconds in enumerate((1.27, 0.83, 0.5))]
    bank = feed(torch_dev, new_bank(omx, fs, 3, ch), xs, fs, ch, whole(xs))
    sps = [ref.segment_peaks(x, fs, COEFFS) for x in xs]
    members = [(0, 0, TO_END), (1, 2, 5), (0, 3, 4), (2, 0, TO_END), (1, 0, 0), (0, 12, 0), (0, 0, TO_END)]
    groups = [(0, 4), (1, 3), (0, 7), (4, 0), (4, 2), (2, 1), (6, 1), (7, 0)]
    want = ref.part_peaks(sps, members, groups, FLOOR)
    got = bank.fetch_group_peaks(members, groups)
    same_parts(got, want, "groups")
    assert got[3]["frames"] == 0 and got[3]["channels"] == 0 and got[3]["max_true_peak_db"] == F32_FLOOR and got[4].tobytes() == got[3].tobytes()
    intervals = bank.fetch_interval_peaks(members)
    same_parts(intervals, ref.part_peaks(sps, members, None, FLOOR), "intervals")
    assert got[5].tobytes() == intervals[2].tobytes() and got[6].tobytes() == intervals[0].tobytes()
    assert intervals[0]["frames"] == (len(xs[0]) // L) * L and intervals[1]["frames"] == 5 * L
    stream = torch_dev.cuda.current_stream().cuda_stream
    d = bank.measure_group_peaks(members, groups, stream=stream)
    torch_dev.cuda.synchronize()
    assert device_bytes(d, len(groups) * 344) == got.tobytes()
    d = bank.measure_interval_peaks(members, stream=stream)
    torch_dev.cuda.synchronize()
    assert device_bytes(d, len(members) * 344) == intervals.tobytes()
    assert bank.measure_interval_peaks([]) == 0 and bank.measure_group_peaks(members, []) == 0
    # the peak of the first second per row and per interval agree
    row = bank.fetch_peak_rows(0, 0, 10, 1)[0]
    part = bank.fetch_interval_peaks([(0, 0, 10)])[0]
    assert row["true_peak"].tobytes() == part["true_peak"].tobytes() and row["true_peak_offset"].tolist() == part["true_peak_frame"].tolist()


def test_part_gains(torch_dev, omx):
    """plan_part_gains against omx_program_gain_evaluate fed the group record's loudness and the group peak: every field equal, `gain`
    within 1 ulp.  A peak outside the part holds plan_group_gains below plan_part_gains; with the peak inside both agree"""
    fs, ch = 48000.0, 2
    L = ref.segment_frames(fs)
    x = (0.1 * pref.programme(30, fs, ch, 3.0)).astype(np.float32)
    x[int(0.55 * fs), 0] = 0.9                                           # segment 5
    bank = feed(torch_dev, new_bank(omx, fs, 1, ch), [x], fs, ch, whole([x]))
    members = [(0, 10, 20), (0, 0, 20), (0, 0, TO_END)]
    groups = [(0, 1), (1, 1), (0, 3), (2, 0)]
    rule = GainRule(target_lufs=-10.0, true_peak_ceiling_db=-1.0, flags=GAIN_LIMIT_PEAK)
    stream = torch_dev.cuda.current_stream().cuda_stream
    bank.plan_group_gains(rule, members, groups, stream=stream)
    by_stream = bank.fetch_gains()
    d = bank.plan_part_gains(rule, members, groups, stream=stream)
    torch_dev.cuda.synchronize()
    by_part = bank.fetch_gains()
    assert device_bytes(d, 4 * 32) == by_part.tobytes()
    loud, peak = bank.fetch_groups(members, groups), bank.fetch_group_peaks(members, groups)
    for k in range(len(groups)):
        want = evaluate_gain(omx, rule, float(loud[k]["integrated_lufs"]), int(loud[k]["gating_above_relative"]),
                             float(peak[k]["max_true_peak_db"]), FLOOR)
        for f in want.dtype.names:
            if f == "gain":
                assert abs(int(by_part[k][f].view(np.uint32)) - int(want[f].view(np.uint32))) <= 1, (k, by_part[k], want)
            else:
                assert by_part[k][f].tobytes() == want[f].tobytes(), (k, f, by_part[k], want)
    assert peak[0]["max_true_peak_db"] < -10 and peak[1]["max_true_peak_db"] > -1.5
    assert by_stream[0]["limited_by"] == 1 and by_stream[0]["gain_db"] < by_part[0]["gain_db"]      # held down by a peak that is not in it
    assert by_stream[0]["source_peak_db"] == bank.fetch_peaks(0).max_true_peak_db and by_part[0]["source_peak_db"] == peak[0]["max_true_peak_db"]
    assert by_stream[1].tobytes() == by_part[1].tobytes() and by_stream[2].tobytes() == by_part[2].tobytes()
    assert by_part[3]["limited_by"] == 4 and by_part[3]["source_peak_db"] == F32_FLOOR             # an empty group: no measurement


def snapshot(bank, n_streams, members, groups, rule):
    stream_records = [(bank.fetch(s), bank.fetch_peaks(s).tobytes(), bank.fetch_segments(s).tobytes()) for s in range(n_streams)]
    bank.plan_group_gains(rule, members, groups)
    return stream_records, bank.fetch_intervals(members).tobytes(), bank.fetch_groups(members, groups).tobytes(), bank.fetch_gains().tobytes()


def test_everything_else_keeps_its_bytes(torch_dev, omx):
    """fetch, fetch_peaks, fetch_intervals, fetch_groups, plan_group_gains and the segment energies with the timeline on equal those with
    it off on the same input; the interval record's max_true_peak_db is still the floor; the timeline is off by default"""
    fs, ch = 48000.0, 2
    xs = [pref.programme(70 + s, fs, ch, 1.3 + 0.4 * s).astype(np.float32) for s in range(2)]
    members, groups = [(0, 0, 13), (1, 2, 6), (0, 4, 5)], [(0, 3), (1, 1)]     # (fetch_intervals takes no OMX_PROGRAM_TO_END)
    rule = GainRule(target_lufs=-16.0, flags=GAIN_LIMIT_PEAK)
    schedule = [np.array([5000, 0], np.uint32), np.array([len(xs[0]) - 5000, len(xs[1])], np.uint32)]
    got = {}
    for on in (False, True):
        bank = feed(torch_dev, new_bank(omx, fs, 2, ch, timeline=on), xs, fs, ch, schedule)
        got[on] = snapshot(bank, 2, members, groups, rule)
        assert (bank.fetch_intervals(members)["max_true_peak_db"] == F32_FLOOR).all()
        if not on:
            with pytest.raises(capi.OmxError) as e:
                bank.fetch_peak_rows(0, 0, 1, 1)            # off by default
            assert e.value.status == capi.ERR_INVALID and str(e.value).split(": ", 1)[1].startswith(PREFIX)
    assert got[True] == got[False]


def raw(omx, name, argtypes):
    return omx.fn("program_loudness_bank_" + name, C.c_int, argtypes)


def refused(omx, status, call):
    rc = call()
    assert rc == status, (rc, status)
    message = omx.fn("last_error", C.c_char_p, [])().decode()
    assert message.startswith(PREFIX), message
    return message


def test_refusals_leave_everything_as_it_was(torch_dev, omx):
    """timeline off, peaks off, samples held, a bounded bank (UNSUPPORTED), bad ranges, null pointers: the status, the message's prefix,
    sentinels in the outputs; set_peaks(0) switches the timeline off"""
    fs, ch = 48000.0, 2
    L = ref.segment_frames(fs)
    x = pref.programme(80, fs, ch, 0.45).astype(np.float32)
    P, U64 = C.c_void_p, C.c_uint64
    set_timeline = raw(omx, "set_peak_timeline", [P, C.c_uint32])
    fetch_rows = raw(omx, "fetch_peak_rows", [P, U64, U64, U64, U64, P])
    peak_rows = raw(omx, "peak_rows", [P, U64, U64, U64, P, P])
    fetch_intervals = raw(omx, "fetch_interval_peaks", [P, P, U64, P])
    measure_intervals = raw(omx, "measure_interval_peaks", [P, P, U64, P, P])
    fetch_groups = raw(omx, "fetch_group_peaks", [P, P, U64, P, U64, P])
    measure_groups = raw(omx, "measure_group_peaks", [P, P, U64, P, U64, P, P])
    plan = raw(omx, "plan_part_gains", [P, P, P, U64, P, U64, P, P])
    INVALID, UNSUPPORTED = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    rows = np.full(4, 0xA5, np.uint8).repeat(136).view(PEAK_ROW_DTYPE)
    parts = np.full(2 * 344, 0xA5, np.uint8).view(PART_PEAK_DTYPE)
    sentinel_rows, sentinel_parts = rows.tobytes(), parts.tobytes()
    out = C.c_void_p(0x1234)
    members = ProgramLoudnessBank._intervals([(0, 0, 2), (0, 1, TO_END)])
    groups = ProgramLoudnessBank._groups([(0, 2), (1, 1)])
    rule = GainRule(flags=GAIN_LIMIT_PEAK).to_c()

    bounded = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, storage="histogram")
    assert "bounded" in refused(omx, UNSUPPORTED, lambda: set_timeline(bounded._h, 1))

    bank = new_bank(omx, fs, 1, ch, timeline=False, peaks=False)
    assert "peaks are off" in refused(omx, INVALID, lambda: set_timeline(bank._h, 1))
    bank.set_peaks(True)
    feed(torch_dev, bank, [x], fs, ch, whole([x]))
    assert "holds samples" in refused(omx, INVALID, lambda: set_timeline(bank._h, 1))
    # the timeline is off: every function of the header refuses
    for call in (lambda: fetch_rows(bank._h, 0, 0, 1, 4, rows.ctypes.data), lambda: peak_rows(bank._h, 0, 1, 4, rows.ctypes.data, None),
                 lambda: fetch_intervals(bank._h, members.ctypes.data, 2, parts.ctypes.data),
                 lambda: measure_intervals(bank._h, members.ctypes.data, 2, None, C.byref(out)),
                 lambda: fetch_groups(bank._h, members.ctypes.data, 2, groups.ctypes.data, 2, parts.ctypes.data),
                 lambda: measure_groups(bank._h, members.ctypes.data, 2, groups.ctypes.data, 2, None, C.byref(out)),
                 lambda: plan(bank._h, C.byref(rule), members.ctypes.data, 2, groups.ctypes.data, 2, None, C.byref(out))):
        assert "timeline is off" in refused(omx, INVALID, call)
    assert rows.tobytes() == sentinel_rows and parts.tobytes() == sentinel_parts and out.value == 0x1234
    with pytest.raises(capi.OmxError):
        bank.fetch_gains()                                  # the refused plan planned nothing

    bank.reset()
    bank.set_peak_timeline(True)
    feed(torch_dev, bank, [x], fs, ch, whole([x]))
    segments = bank.fetch(0).segments
    assert segments == len(x) // L == 4
    assert "holds samples" in refused(omx, INVALID, lambda: set_timeline(bank._h, 0))
    good_rows, good_parts = bank.fetch_peak_rows(0, 0, 1, 5).tobytes(), bank.fetch_group_peaks(members, groups).tobytes()
    bad_members = ProgramLoudnessBank._intervals([(0, 0, 2), (0, 3, 2)])
    far_members = ProgramLoudnessBank._intervals([(0, 0, 2), (1, 0, 1)])
    bad_groups = ProgramLoudnessBank._groups([(0, 2), (1, 2)])
    bad_rule = GainRule(min_gain_db=1.0, max_gain_db=0.0).to_c()
    for call in (lambda: fetch_rows(bank._h, 1, 0, 1, 4, rows.ctypes.data),                       # stream index out of range
                 lambda: fetch_rows(bank._h, 0, 0, 0, 4, rows.ctypes.data),                       # stride 0
                 lambda: fetch_rows(bank._h, 0, 0, 2 ** 32 // L + 1, 4, rows.ctypes.data),        # stride * L beyond 2^32 - 1
                 lambda: fetch_rows(bank._h, 0, 2 ** 64 - 2, 1, 4, rows.ctypes.data),             # first + (count - 1) * stride beyond 64 bits
                 lambda: fetch_rows(bank._h, 0, 0, 1, 4, None),                                   # null rows
                 lambda: peak_rows(bank._h, 0, 1, 4, None, None),
                 lambda: peak_rows(bank._h, 0, 0, 4, rows.ctypes.data, None),
                 lambda: peak_rows(bank._h, 0, 1, 2 ** 32, rows.ctypes.data, None),               # n_streams * count beyond 2^32 - 1
                 lambda: fetch_intervals(bank._h, bad_members.ctypes.data, 2, parts.ctypes.data),  # beyond the stored segments
                 lambda: fetch_intervals(bank._h, far_members.ctypes.data, 2, parts.ctypes.data),  # stream out of range
                 lambda: fetch_intervals(bank._h, None, 2, parts.ctypes.data),
                 lambda: fetch_intervals(bank._h, members.ctypes.data, 2, None),
                 lambda: measure_intervals(bank._h, members.ctypes.data, 2, None, None),           # null d_peaks
                 lambda: measure_intervals(bank._h, bad_members.ctypes.data, 2, None, C.byref(out)),
                 lambda: fetch_groups(bank._h, members.ctypes.data, 2, bad_groups.ctypes.data, 2, parts.ctypes.data),   # group outside the table
                 lambda: fetch_groups(bank._h, bad_members.ctypes.data, 2, groups.ctypes.data, 2, parts.ctypes.data),
                 lambda: fetch_groups(bank._h, members.ctypes.data, 2, None, 2, parts.ctypes.data),
                 lambda: fetch_groups(bank._h, members.ctypes.data, 2, groups.ctypes.data, 2, None),
                 lambda: measure_groups(bank._h, members.ctypes.data, 2, groups.ctypes.data, 2, None, None),
                 lambda: plan(bank._h, C.byref(bad_rule), members.ctypes.data, 2, groups.ctypes.data, 2, None, C.byref(out)),
                 lambda: plan(bank._h, None, members.ctypes.data, 2, groups.ctypes.data, 2, None, C.byref(out)),
                 lambda: plan(bank._h, C.byref(rule), bad_members.ctypes.data, 2, groups.ctypes.data, 2, None, C.byref(out)),
                 lambda: plan(bank._h, C.byref(rule), members.ctypes.data, 2, groups.ctypes.data, 2, None, None)):
        refused(omx, INVALID, call)
    assert rows.tobytes() == sentinel_rows and parts.tobytes() == sentinel_parts and out.value == 0x1234
    assert bank.fetch_peak_rows(0, 0, 1, 5).tobytes() == good_rows and bank.fetch_group_peaks(members, groups).tobytes() == good_parts
    with pytest.raises(capi.OmxError):
        bank.fetch_gains()
    # counts of 0 produce nothing and touch nothing
    assert fetch_rows(bank._h, 0, 0, 1, 0, None) == 0 and fetch_intervals(bank._h, None, 0, None) == 0
    assert fetch_groups(bank._h, None, 0, None, 0, None) == 0
    # set_peaks(0) takes the timeline with it
    bank.reset()
    bank.set_peaks(False)
    bank.set_peaks(True)
    assert "timeline is off" in refused(omx, INVALID, lambda: fetch_rows(bank._h, 0, 0, 1, 4, rows.ctypes.data))
    bank.set_peak_timeline(True)
    feed(torch_dev, bank, [x], fs, ch, whole([x]))
    assert bank.fetch_peak_rows(0, 0, 1, 5).tobytes() == good_rows


def test_c99_host_prints_the_rows_of_the_ebu_tone(tmp_path, omx):
    """tests/c_abi/program_peak_timeline_demo.c: fs/4 at 45 degrees, amplitude 0.25 then 0.5, a peak log per second from a plain C host"""
    from test_cpu_program_peak_timeline import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    v = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)}
    assert abs(v["row1_sample_peak"] + 9.03) <= 0.01 and -6.4 <= v["row1_true_peak"] <= -5.8, v
    # the first second is the same tone 6.02 dB lower, inside the same EBU tolerance (+0.2 / -0.4 dB): each second has an onset of its
    # own (from silence, from half the amplitude), so the two readings are not exactly 6.02 dB apart
    assert abs(v["row0_sample_peak"] + 15.05) <= 0.01 and -12.42 <= v["row0_true_peak"] <= -11.82, v
    assert v["row1_frames"] == 48000 and v["row1_valid"] == 1 and v["part_frames"] == 48000 and 48000 <= v["part_first_frame"] < 48024
    assert abs(v["part_true_peak"] - v["row1_true_peak"]) <= 1e-4 and v["whole_true_peak"] == v["part_true_peak"], v

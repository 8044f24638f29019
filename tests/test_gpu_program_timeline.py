"""Programme bank timeline and intervals on the GPU (`-m gpu`): openmeters_amd.program_loudness against the numpy restatement
(tests/program_timeline_ref.py, pinned to program_loudness_ref.results by tests/test_cpu_program_timeline.py).

Every comparison feeds the restatement the bank's own fetch_segments, as the result-pass checks of
tests/test_gpu_program_loudness_matrix.py do.  Bars: 1e-4 LU on every LUFS / LU field; on CLEAN rows (gate margin of the programme
e[0 .. j] at least ref.RESULT_PASS_MARGIN_MIN) both counts exact and both energies within ref.energy_bound(j), relative; rows that
are not clean are counted and may be at most 1 % of a case.  Determinism, window independence and the append property are bitwise."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_loudness_ref as ref
import program_timeline_ref as tl
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, INTERVAL_DTYPE, RECORD_DTYPE, TIMELINE_ROW_DTYPE,
                                             ProgramLoudnessBank, ProgramLoudnessRecord)
from parity import bar
from test_cpu_program_timeline import build_demo
from test_gpu_program_loudness import BAR, FLOOR, coefficients, run_once, run_schedule, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
EMPTY = tl.empty_row(FLOOR).tobytes()
NOT_IN_AN_INTERVAL = ("frames", "overflow", "max_true_peak_db", "_pad")


FLOAT_FIELDS = ("integrated_energy", "relative_threshold_energy", "momentary_lufs", "short_term_lufs", "integrated_lufs")


def device_bytes(ptr, n):
    """n bytes of device memory at `ptr`, through the HIP runtime the process has already loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    raw = (C.c_uint8 * n)()
    copy = C.CDLL(path).hipMemcpy
    copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert copy(raw, C.c_void_p(ptr), n, 2) == 0      # 2 = device to host
    return bytes(raw)


def device_timeline(torch, bank, first, stride, count):
    """bank.timeline into device memory: [n_streams][count] rows"""
    d = torch.full((max(bank.n_streams * count * TIMELINE_ROW_DTYPE.itemsize, 1),), 0xA5, dtype=torch.uint8).cuda()
    status = bank.timeline(d.data_ptr(), first, stride, count, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == (1 if count else 0)
    return d.cpu().numpy()[:bank.n_streams * count * TIMELINE_ROW_DTYPE.itemsize].view(TIMELINE_ROW_DTYPE).reshape(bank.n_streams, count)


def check_rows(got, e, first, stride, tag, measured):
    """rows `got` of a stream whose stored energies are e against the restatement; returns (rows that are not clean, rows that exist)"""
    want, p = tl.timeline(e, first, stride, len(got), FLOOR), tl.Prefixes(e)
    unclean = exist = 0
    worst = {"momentary_lufs": 0.0, "short_term_lufs": 0.0, "integrated_lufs": 0.0, "integrated_energy": 0.0, "relative_threshold_energy": 0.0}
    failures = []
    for i, j in enumerate(tl.row_indices(first, stride, len(got))):
        g, w = got[i], want[i]
        if j >= len(e):
            assert g.tobytes() == EMPTY, (tag, j, g)
            continue
        exist += 1
        assert g["valid"] == 1, (tag, j)
        for f in FLOAT_FIELDS:      # (a NaN would slip through every comparison below)
            assert np.isfinite(g[f]), (tag, j, f, g[f])
        for f in ("momentary_lufs", "short_term_lufs"):
            worst[f] = max(worst[f], abs(float(g[f]) - float(w[f])))
            measured["block bits equal"] = measured.get("block bits equal", 0) + (g[f].tobytes() == w[f].tobytes())
            measured["block fields"] = measured.get("block fields", 0) + 1
        if p.margin(int(j)) < ref.RESULT_PASS_MARGIN_MIN:
            unclean += 1
            continue
        worst["integrated_lufs"] = max(worst["integrated_lufs"], abs(float(g["integrated_lufs"]) - float(w["integrated_lufs"])))
        for f in ("gating_above_absolute", "gating_above_relative"):
            if g[f] != w[f]:
                failures.append((tag, j, f, int(g[f]), int(w[f])))
        for f in ("integrated_energy", "relative_threshold_energy"):
            exp = float(w[f])
            rel = abs(float(g[f]) - exp) / exp if exp > 0.0 else abs(float(g[f]))
            worst[f] = max(worst[f], rel)
            if rel > ref.energy_bound(int(j)):
                failures.append((tag, j, f, float(g[f]), exp, rel, ref.energy_bound(int(j))))
    for f, v in worst.items():
        measured[f] = max(measured.get(f, 0.0), v)
    assert not failures, failures[:5]
    for f in ("momentary_lufs", "short_term_lufs", "integrated_lufs"):
        bar(f"program timeline: |d {f}| LU", worst[f], BAR, tag)
    assert unclean <= tl.UNCLEAN_SHARE_MAX * exist, (tag, unclean, exist)
    return unclean, exist


def fmt(measured):
    return {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in measured.items()}


def bank_8k(torch, omx, xs, capacity_seconds=200, peaks=False, form=0):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=tl.EDGE_RATE), len(xs), 1, capacity_seconds)
    bank.set_option(capi.OPT_KERNEL_FORM, form)
    if peaks:
        bank.set_peaks(True)
    feed(torch, bank, xs, tl.EDGE_RATE)
    return bank


def feed(torch, bank, xs, fs, ch=1, reset_mask=None):
    longest = max(max(len(x) for x in xs), 1)
    host = np.zeros((len(xs), longest, ch), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    d = torch.from_numpy(host).cuda()
    bank.process(d.data_ptr(), longest, ch, fs, capi.positions_fallback(ch), frames=[len(x) for x in xs], reset_mask=reset_mask,
                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 1. rows against the restatement
@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_timeline_rows_against_the_restatement_in_both_forms(torch_dev, omx, fs, ch, seeds):
    """every row at stride 1, both segment-pass forms.  Measured on an MI355X: momentary / short-term equal bits in all 27 200 fields,
    0 rows not clean, integrated_lufs 0.0 LU apart, relative_threshold_energy <= 7.3e-16 and integrated_energy <= 1.5e-15 relative"""
    pos = capi.positions_fallback(ch)
    xs = [ref.programme(seed, fs, ch, ref.SEEDED_SECONDS) for seed in seeds]
    measured, unclean, rows = {}, 0, 0
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_once(torch_dev, omx, xs, fs, ch, pos, form)
        n = max(bank.fetch(s).segments for s in range(len(xs)))
        got = device_timeline(torch_dev, bank, 0, 1, n)
        for s in range(len(xs)):
            u, k = check_rows(got[s], bank.fetch_segments(s), 0, 1, (fs, ch, seeds[s], form), measured)
            unclean, rows = unclean + u, rows + k
            assert bank.fetch_timeline(s).tobytes() == got[s][:bank.fetch(s).segments].tobytes()
    print(f"{fs} Hz {ch} ch: {rows} rows, {unclean} not clean; measured (LU / relative): {fmt(measured)}")
    # (both sides add a block oldest first, so the blocks are the same f64; the dB fields then differ at most by the two log10)


# ---------------------------------------------------------------- 2. determinism and window independence, bitwise
def test_rows_do_not_depend_on_the_window_the_call_or_later_appends(torch_dev, omx):
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    xs = [ref.programme(seed, fs, ch, ref.SEEDED_SECONDS) for seed in (0, 1, 3)]
    xs[1] = xs[1][:len(xs[1]) // 3]
    T = max(len(x) for x in xs)
    cuts = [0, 7 * 4800 + 100, 7 * 4800 + 101, 20 * 4800, 31 * 4800 + 2400, T]
    schedule = [np.array([max(min(len(x), hi) - min(len(x), lo), 0) for x in xs], np.uint32) for lo, hi in zip(cuts[:-1], cuts[1:])]
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, 200)
    bank.set_option(capi.OPT_KERNEL_FORM, FORM_REFERENCE_ORDER)
    cursor, earlier = [0] * len(xs), None
    for counts in schedule:
        host = np.zeros((len(xs), int(counts.max()), ch), np.float32)
        for s, n in enumerate(counts):
            host[s, :n] = xs[s][cursor[s]:cursor[s] + n]
            cursor[s] += int(n)
        d = torch_dev.from_numpy(host).cuda()
        bank.process(d.data_ptr(), int(counts.max()), ch, fs, pos, frames=counts, stream=torch_dev.cuda.current_stream().cuda_stream)
        torch_dev.cuda.synchronize()
        now = [bank.fetch_timeline(s) for s in range(len(xs))]
        assert [len(r) for r in now] == [c // 4800 for c in cursor]
        if earlier is not None:      # the rows after call k are a prefix of the rows after call k + 1
            for s in range(len(xs)):
                assert now[s][:len(earlier[s])].tobytes() == earlier[s].tobytes(), s
        earlier = now
    n = len(earlier[0])
    assert n == 400 and len(earlier[1]) == 133
    whole = device_timeline(torch_dev, bank, 0, 1, n)
    assert device_timeline(torch_dev, bank, 0, 1, n).tobytes() == whole.tobytes()          # the same call twice
    for s in range(len(xs)):
        assert whole[s][:len(earlier[s])].tobytes() == earlier[s].tobytes()                  # device rows and fetch_timeline agree
        assert whole[s][len(earlier[s]):].tobytes() == EMPTY * (n - len(earlier[s]))
    for first, stride, count in ((0, 3, 134), (1, 3, 133), (5, 7, 57), (13, 7, 70), (3, 64, 7), (63, 64, 6), (129, 1, 271), (399, 1, 1), (255, 1, 2),
                                 (256, 3, 5), (131, 64, 9)):
        got = device_timeline(torch_dev, bank, first, stride, count)
        for s in range(len(xs)):
            want = np.full((count,), tl.empty_row(FLOOR), TIMELINE_ROW_DTYPE)
            js = tl.row_indices(first, stride, count)
            want[js < n] = whole[s][js[js < n]]
            assert got[s].tobytes() == want.tobytes(), (first, stride, count, s)
            assert bank.fetch_timeline(s, first, stride, count).tobytes() == want.tobytes(), (first, stride, count, s)


# ---------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("n_streams", [1, 5, 65])
def test_banks_of_short_and_long_streams_in_one_call(torch_dev, omx, n_streams):
    xs = tl.edge_programmes(n_streams)
    measured = {}
    for peaks in (False, True):
        bank = bank_8k(torch_dev, omx, xs, peaks=peaks)
        segments = [bank.fetch(s).segments for s in range(n_streams)]
        assert segments == [tl.EDGE_SEGMENTS[s % len(tl.EDGE_SEGMENTS)] for s in range(n_streams)]
        count = max(segments) + 3
        got = device_timeline(torch_dev, bank, 0, 1, count)
        if not peaks:
            plain = got
        assert got.tobytes() == plain.tobytes()                               # a bank with peaks on gives the same rows
        for s in range(n_streams):
            check_rows(got[s], bank.fetch_segments(s), 0, 1, ("edges", n_streams, s), measured)
            rec = bank.fetch(s)
            if segments[s]:       # the last row and the record of the result pass
                last = got[s][segments[s] - 1]
                assert (last["gating_above_absolute"], last["gating_above_relative"]) == (rec.gating_above_absolute, rec.gating_above_relative)
                for f in ("momentary_lufs", "short_term_lufs", "integrated_lufs"):
                    bar(f"program timeline: last row vs record, |d {f}| LU", abs(float(last[f]) - float(getattr(rec, f))), BAR, (n_streams, s))
    print(f"{n_streams} streams: measured (LU / relative): {fmt(measured)}")


def test_reset_empties_the_rows_of_the_flagged_streams_only(torch_dev, omx):
    xs = tl.edge_programmes(9)
    bank = bank_8k(torch_dev, omx, xs)
    before = device_timeline(torch_dev, bank, 0, 1, 500)
    mask = [1 if s in (0, 7) else 0 for s in range(9)]
    bank.reset(mask)
    after = device_timeline(torch_dev, bank, 0, 1, 500)
    for s in range(9):
        assert after[s].tobytes() == (EMPTY * 500 if mask[s] else before[s].tobytes()), s
    feed(torch_dev, bank, [x[:len(x) // 2] if mask[s] else x[:0] for s, x in enumerate(xs)], tl.EDGE_RATE)
    again, measured = device_timeline(torch_dev, bank, 0, 1, 500), {}
    for s in range(9):
        if mask[s]:
            assert again[s][0]["valid"] == 1
            check_rows(again[s], bank.fetch_segments(s), 0, 1, ("after reset", s), measured)
        else:
            assert again[s].tobytes() == before[s].tobytes()


def test_rows_stop_at_capacity(torch_dev, omx):
    x = ref.programme(3, tl.EDGE_RATE, 1, 12.0)
    bank = bank_8k(torch_dev, omx, [x, x[:4000]], capacity_seconds=10)
    rec = bank.fetch(0)
    assert rec.overflow and rec.segments == 100 and not bank.fetch(1).overflow
    got, measured = device_timeline(torch_dev, bank, 90, 1, 20), {}
    assert got[0][9]["valid"] == 1 and got[0][10:].tobytes() == EMPTY * 10
    check_rows(got[0], bank.fetch_segments(0), 90, 1, "overflow", measured)
    check_rows(got[1], bank.fetch_segments(1), 90, 1, "overflow, short", measured)
    assert len(bank.fetch_timeline(0)) == 100


# ---------------------------------------------------------------- 4. long programmes
def test_timeline_over_one_hour_programmes(torch_dev, omx):
    fs, seg = ref.HOUR_RATE, ref.segment_frames(ref.HOUR_RATE)
    xs = [ref.hour_programme("tone")[:36000 * seg - seg - seg // 2], ref.hour_programme("steps")]
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 2, 1, ref.HOUR_SECONDS)
    feed(torch_dev, bank, xs, fs)
    count = (36000 + tl.HOUR_STRIDE - 1) // tl.HOUR_STRIDE
    got, measured = device_timeline(torch_dev, bank, 0, tl.HOUR_STRIDE, count), {}
    for s, kind in enumerate(("tone", "steps")):
        u, k = check_rows(got[s], bank.fetch_segments(s), 0, tl.HOUR_STRIDE, ("one hour", kind), measured)
        print(f"one hour, {kind}: {u} rows of {k} not clean")
        rec, last = bank.fetch(s), bank.fetch_timeline(s, bank.fetch(s).segments - 1, 1, 1)[0]
        assert (last["gating_above_absolute"], last["gating_above_relative"]) == (rec.gating_above_absolute, rec.gating_above_relative)
        bar("program timeline: last row vs record, |d integrated_lufs| LU", abs(float(last["integrated_lufs"]) - rec.integrated_lufs), BAR, kind)
    assert got[0][-1]["valid"] == 1 and got[1][-1]["valid"] == 1      # j = 35994 exists in both
    print(f"one hour at 8 kHz, stride {tl.HOUR_STRIDE}: measured (LU / relative): {fmt(measured)}")


def test_timeline_over_four_hours(torch_dev, omx):
    fs = ref.HOUR_RATE
    x = ref.hour_programme("steps", seconds=ref.FOUR_HOURS_SECONDS, seed=ref.FOUR_HOURS_SEED)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, 1, ref.FOUR_HOURS_SECONDS)
    feed(torch_dev, bank, [x], fs)
    assert bank.fetch(0).segments == 144000
    measured = {}
    got = device_timeline(torch_dev, bank, 0, tl.FOUR_HOURS_STRIDE, 2400)
    u, k = check_rows(got[0], bank.fetch_segments(0), 0, tl.FOUR_HOURS_STRIDE, "four hours", measured)
    tail = bank.fetch_timeline(0, 143990, 1, 12)
    assert tail[:10]["valid"].all() and tail[10:].tobytes() == EMPTY * 2 and tail[0].tobytes() != got[0][-1].tobytes()
    assert bank.fetch_timeline(0, 143940, 1, 1).tobytes() == got[0][-1].tobytes()       # j = 2399 * 60 through another window
    print(f"four hours at 8 kHz, stride {tl.FOUR_HOURS_STRIDE}: {u} rows of {k} not clean; measured (LU / relative): {fmt(measured)}")


# ---------------------------------------------------------------- 5. intervals
def record_array(rec):
    """a fetched ProgramLoudnessRecord as one RECORD_DTYPE element"""
    out = np.zeros((), RECORD_DTYPE)
    for f in ProgramLoudnessRecord.ENERGY_FIELDS + ProgramLoudnessRecord.COUNT_FIELDS + ProgramLoudnessRecord.LEVEL_FIELDS:
        out[f] = getattr(rec, f)
    out["overflow"] = rec.overflow
    return out


def check_interval(got, want, tag, measured):
    for f in tl.RECORD_LEVELS + tl.RECORD_ENERGIES:
        assert np.isfinite(got[f]), (tag, f, got[f])
    for f in tl.RECORD_COUNTS + ("frames", "overflow"):
        assert int(got[f]) == int(want[f]), (tag, f, int(got[f]), int(want[f]))
    assert got["max_true_peak_db"] == np.float32(FLOOR), tag
    for f in tl.RECORD_LEVELS:
        d = bar(f"program intervals: |d {f}| LU", abs(float(got[f]) - float(want[f])), BAR, (tag, got[f], want[f]))
        measured[f] = max(measured.get(f, 0.0), d)
    means = {"integrated_energy": "gating_above_relative", "relative_threshold_energy": "gating_above_absolute"}
    for f in tl.RECORD_ENERGIES:
        exp, bound = float(want[f]), ref.energy_bound(int(want[means[f]]) if f in means else 0)
        assert abs(float(got[f]) - exp) <= bound * exp, (tag, f, float(got[f]), exp, bound)
        if exp > 0.0:
            measured[f] = max(measured.get(f, 0.0), abs(float(got[f]) - exp) / exp)


def test_whole_stream_intervals_have_the_bits_of_fetch(torch_dev, omx):
    for n_streams, peaks in ((9, False), (9, True), (65, False)):
        xs = tl.edge_programmes(n_streams)
        bank = bank_8k(torch_dev, omx, xs, peaks=peaks)
        recs = [bank.fetch(s) for s in range(n_streams)]
        got = bank.fetch_intervals([(s, 0, recs[s].segments) for s in range(n_streams)])
        for s in range(n_streams):
            want = record_array(recs[s])
            for f in RECORD_DTYPE.names:
                if f not in NOT_IN_AN_INTERVAL:
                    assert got[s][f].tobytes() == want[f].tobytes(), (n_streams, s, f, got[s][f], want[f])
            assert got[s]["frames"] == recs[s].segments * 800 and got[s]["overflow"] == 0 and got[s]["max_true_peak_db"] == np.float32(FLOOR)
            assert recs[s].frames == len(xs[s]) and (not peaks or recs[s].segments < 200 or recs[s].max_true_peak_db > FLOOR)


def test_seeded_intervals_over_a_bank_of_64_streams(torch_dev, omx):
    xs = [tl.interval_bank_programme(s) for s in range(tl.INTERVAL_STREAMS)]
    bank = bank_8k(torch_dev, omx, xs, capacity_seconds=200)
    es = [bank.fetch_segments(s) for s in range(len(xs))]
    drawn = tl.draw_intervals([len(e) for e in es])
    got, measured = bank.fetch_intervals(drawn), {}
    assert len(got) == len(drawn) >= 3900
    for i, (s, a, c) in enumerate(drawn):
        want = tl.intervals(es[s], a, c, 800, FLOOR)
        assert want["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN, (s, a, c, want["gate_margin"])
        check_interval(got[i], want, (s, a, c), measured)
    d = bank.measure_intervals(drawn, stream=torch_dev.cuda.current_stream().cuda_stream)      # the device array and the fetch form agree
    torch_dev.cuda.synchronize()
    assert device_bytes(d, len(drawn) * RECORD_DTYPE.itemsize) == got.tobytes()
    assert bank.fetch_intervals(drawn).tobytes() == got.tobytes()
    print(f"{len(drawn)} intervals: measured (LU / relative): {fmt(measured)}")


def test_ebu_known_answers_through_the_product(torch_dev, omx):
    """EBU Tech 3341 #3 / #4 (running integrated loudness at the end of the first -36 dBFS span and at the end; #4's middle minute
    alone) and Tech 3342 #1 (halves and whole) through the bank"""
    fs, pos = 48000.0, capi.positions_fallback(2)
    cases = {name: spans for name, spans, _ in ref.EBU_3341 + ref.EBU_3342}
    xs = [ref.tone_programme(fs, cases[name]) for name in tl.EBU_THROUGH_THE_PRODUCT]
    bank = run_once(torch_dev, omx, xs, fs, 2, pos, FORM_REFERENCE_ORDER)
    rows, measured = device_timeline(torch_dev, bank, 0, 1, 1000), {}
    for s, name in enumerate(tl.EBU_THROUGH_THE_PRODUCT):
        check_rows(rows[s], bank.fetch_segments(s), 0, 1, name, measured)
    for s, span_end, n in ((0, 100, 800), (1, 200, 1000)):
        print(tl.EBU_THROUGH_THE_PRODUCT[s], rows[s][span_end - 1]["integrated_lufs"], rows[s][n - 1]["integrated_lufs"])
        assert abs(float(rows[s][span_end - 1]["integrated_lufs"]) + 36.0) <= 0.1 and abs(float(rows[s][n - 1]["integrated_lufs"]) + 23.0) <= 0.1
        rec = bank.fetch(s)
        assert (rows[s][n - 1]["gating_above_absolute"], rows[s][n - 1]["gating_above_relative"]) == (rec.gating_above_absolute, rec.gating_above_relative)
    middle, first, second, whole = bank.fetch_intervals([(1, 200, 600), (2, 0, 200), (2, 200, 200), (2, 0, 400)])
    print("3341-4 middle", middle["integrated_lufs"], "3342-1 halves", first["integrated_lufs"], first["loudness_range_lu"],
          second["integrated_lufs"], second["loudness_range_lu"], "whole LRA", whole["loudness_range_lu"])
    assert abs(float(middle["integrated_lufs"]) + 23.0) <= 0.1
    assert abs(float(first["integrated_lufs"]) + 20.0) <= 0.1 and abs(float(second["integrated_lufs"]) + 30.0) <= 0.2
    assert float(first["loudness_range_lu"]) < 1.0 and float(second["loudness_range_lu"]) < 1.0 and abs(float(whole["loudness_range_lu"]) - 10.0) <= 1.0
    for (s, a, c), got in (((1, 200, 600), middle), ((2, 0, 200), first), ((2, 200, 200), second), ((2, 0, 400), whole)):
        check_interval(got, tl.intervals(bank.fetch_segments(s), a, c, 4800, FLOOR), (s, a, c), measured)


# ---------------------------------------------------------------- 6. errors
def test_refused_calls_change_nothing(torch_dev, omx):
    xs = tl.edge_programmes(9)
    bank = bank_8k(torch_dev, omx, xs)
    segments = [bank.fetch(s).segments for s in range(9)]
    good_intervals = [(0, 10, 300), (7, 0, 211), (8, 400, 87), (1, 0, 0)]

    def state():
        return (device_timeline(torch_dev, bank, 5, 3, 100).tobytes(), bank.fetch_timeline(8).tobytes(), bank.fetch_intervals(good_intervals).tobytes(),
                [bank.fetch(s) for s in range(9)], [bank.fetch_segments(s).tobytes() for s in range(9)])

    before = state()
    rows = torch_dev.zeros((9 * 100 * 40,), dtype=torch_dev.uint8).cuda()
    canary = rows.clone()

    def refused(call, *args, **kw):
        with pytest.raises(capi.OmxError) as err:
            call(*args, **kw)
        assert err.value.status == capi.ERR_INVALID, (args, kw, err.value.status)
        torch_dev.cuda.synchronize()
        assert torch_dev.equal(rows, canary)
        assert state() == before, (args, kw)

    refused(bank.timeline, 0, 0, 1, 100)                                  # null rows with count > 0
    refused(bank.timeline, rows.data_ptr(), 0, 0, 100)                    # stride 0
    refused(bank.timeline, rows.data_ptr(), 2 ** 64 - 50, 1, 100)         # first + (count - 1) * stride beyond 64 bits
    refused(bank.timeline, rows.data_ptr(), 0, 2 ** 62, 100)
    refused(bank.timeline, rows.data_ptr(), 0, 1, 2 ** 33)                # n_streams * count beyond the launch grid
    assert bank.timeline(0, 0, 1, 0) == 0 and bank.timeline(rows.data_ptr(), 0, 1, 0) == 0      # count 0: OMX_NONE, nothing written
    torch_dev.cuda.synchronize()
    assert torch_dev.equal(rows, canary)
    fetch_tl = omx.fn("program_loudness_bank_fetch_timeline", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
    host = np.zeros((100,), TIMELINE_ROW_DTYPE)
    assert fetch_tl(bank._h, 9, 0, 1, 100, host.ctypes.data) == capi.ERR_INVALID               # stream index out of range
    assert fetch_tl(bank._h, 0, 0, 0, 100, host.ctypes.data) == capi.ERR_INVALID
    assert fetch_tl(bank._h, 0, 0, 1, 100, None) == capi.ERR_INVALID
    assert fetch_tl(bank._h, 0, 2 ** 64 - 50, 1, 100, host.ctypes.data) == capi.ERR_INVALID
    assert fetch_tl(bank._h, 0, 0, 1, 0, None) == 0 and not host.view(np.uint8).any()
    assert fetch_tl(None, 0, 0, 1, 100, host.ctypes.data) == capi.ERR_INVALID
    assert state() == before
    for bad in ([(9, 0, 1)], [(0, 0, segments[0] + 1)], [(0, segments[0], 1)], [(0, 10, 300), (1, 1, 0)], [(0, 2 ** 64 - 1, 2)],
                [(2, 0, 2)], [(2 ** 32 - 1, 0, 0)]):
        refused(bank.fetch_intervals, bad)
        refused(bank.measure_intervals, bad)
    measure = omx.fn("program_loudness_bank_measure_intervals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
    fetch_iv = omx.fn("program_loudness_bank_fetch_intervals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
    out, one = C.c_void_p(), np.zeros((1,), INTERVAL_DTYPE)
    assert measure(bank._h, None, 3, None, C.byref(out)) == capi.ERR_INVALID and not out.value     # null array with n > 0
    assert measure(bank._h, one.ctypes.data, 1, None, None) == capi.ERR_INVALID
    assert measure(bank._h, None, 0, None, C.byref(out)) == 0 and not out.value                    # n == 0: OMX_NONE
    assert fetch_iv(bank._h, None, 3, np.zeros(3, RECORD_DTYPE).ctypes.data) == capi.ERR_INVALID
    assert fetch_iv(bank._h, one.ctypes.data, 1, None) == capi.ERR_INVALID
    assert fetch_iv(bank._h, None, 0, None) == 0
    assert bank.measure_intervals([]) == 0 and len(bank.fetch_intervals([])) == 0
    assert state() == before
    # a device array handed out before a refused call still holds its records
    d = bank.measure_intervals(good_intervals)
    refused(bank.measure_intervals, [(0, 0, segments[0] + 1)])
    assert device_bytes(d, len(good_intervals) * RECORD_DTYPE.itemsize) == before[2]


def test_a_bank_too_wide_for_one_launch_is_refused_up_front(torch_dev, omx):
    """more than 65 535 streams: `timeline` is OMX_ERR_INVALID before anything is launched, `fetch_timeline` serves the bank per stream"""
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=tl.EDGE_RATE), 65536, 1, 1)
    rows = torch_dev.zeros((65536 * 40,), dtype=torch_dev.uint8).cuda()
    with pytest.raises(capi.OmxError) as err:
        bank.timeline(rows.data_ptr(), 0, 1, 1)
    assert err.value.status == capi.ERR_INVALID
    torch_dev.cuda.synchronize()
    assert not rows.any()
    assert bank.fetch_timeline(65535, 0, 1, 3).tobytes() == EMPTY * 3
    bank.close()


# ---------------------------------------------------------------- 7. the C99 host
def test_c99_demo_matches_the_python_route(torch_dev, omx, tmp_path):
    out = subprocess.run([build_demo(tmp_path)], check=True, capture_output=True, text=True, timeout=300).stdout
    print(out)
    lines = out.strip().splitlines()
    assert len(lines) == 14, out
    fs = 48000.0
    x = ref.tone_programme(fs, [(-20, 6), (-30, 6)])
    bank = run_once(torch_dev, omx, [x], fs, 2, capi.positions_fallback(2), FORM_REFERENCE_ORDER, capacity_seconds=60)
    rows = bank.fetch_timeline(0, 9, 10, 12)
    for i, line in enumerate(lines[:12]):
        w = line.split()
        assert (int(w[1]), int(w[3])) == (9 + 10 * i, 1) and (int(w[11]), int(w[12])) == (rows[i]["gating_above_absolute"], rows[i]["gating_above_relative"])
        for at, f in ((5, "momentary_lufs"), (7, "short_term_lufs"), (9, "integrated_lufs")):
            assert abs(float(w[at]) - float(rows[i][f])) <= 1e-3, (line, rows[i])
    recs = bank.fetch_intervals([(0, 0, 60), (0, 60, 60)])
    for i, line in enumerate(lines[12:]):
        w = line.split()
        assert (int(w[1]), int(w[3]), int(w[5])) == (i, 60, 60 * 4800)
        for at, f in ((7, "integrated_lufs"), (9, "loudness_range_lu"), (11, "max_momentary_lufs"), (13, "max_short_term_lufs")):
            assert abs(float(w[at]) - float(recs[i][f])) <= 1e-3, (line, recs[i])
    assert abs(float(recs[0]["integrated_lufs"]) + 20.0) <= 0.1 and abs(float(recs[1]["integrated_lufs"]) + 30.0) <= 0.1

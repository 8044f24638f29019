"""Programme bank with bounded storage on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank(storage="histogram") against the
numpy restatement (tests/program_histogram_ref.py, pinned to the stored restatement by tests/test_cpu_program_histogram.py).

Every comparison uses a TWIN: a stored bank and a bounded bank get the same calls in the same form, and the restatement is fed the
twin's fetch_segments.  Then the histograms' counts, tail and segment count are exact, both sum arrays and every integer and f64
field of the record equal the restatement bit for bit, the dB fields hold the 1e-4 LU bar; against the twin's stored record the
absolute-gate counts, latest values and maxima are equal bits, integrated loudness is within 1e-4 LU (every input is bin-clean,
asserted on the CPU) and the range within 0.2 LU (each end is the mean of the 0.1 LU bin that holds the stored mode's rank element)."""
import subprocess

import numpy as np
import pytest

import program_histogram_ref as hr
import program_loudness_ref as ref
import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import FORM_BY_SHAPE, FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, ProgramLoudnessBank
from parity import bar
from test_cpu_program_histogram import build_demo
from test_gpu_program_loudness import BAR, FLOOR, device_rows, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
LEVELS = ("integrated_lufs", "relative_threshold_lufs", "loudness_range_lu", "momentary_lufs", "short_term_lufs", "max_momentary_lufs",
          "max_short_term_lufs")
SAME_AS_STORED = ("gating_above_absolute", "short_term_above_absolute", "momentary_energy", "short_term_energy", "max_momentary_energy",
                  "max_short_term_energy", "frames", "segments", "gating_blocks", "short_term_blocks", "max_true_peak_db")
FS8, POS1 = hr.EDGE_RATE, capi.positions_fallback(1)


@pytest.fixture(scope="module")
def B(omx):
    return openmeters_amd.histogram_boundaries(omx)


def bits(v):
    return np.float64(v).tobytes()


def twin(omx, fs, n_streams, ch, form=FORM_BY_SHAPE, capacity_seconds=200, peaks=False):
    """(stored bank, bounded bank) with the same options"""
    banks = (ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n_streams, ch, capacity_seconds),
             ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n_streams, ch, storage="histogram"))
    assert not banks[0].is_bounded() and banks[1].is_bounded()
    for b in banks:
        b.set_option(capi.OPT_KERNEL_FORM, form)
        if peaks:
            b.set_peaks(True)
    return banks


def feed(torch, banks, xs, fs, ch, pos, reset_mask=None):
    """one call: programme xs[s] (any length, 0 included) to stream s of every bank"""
    d, longest = device_rows(torch, [x if len(x) else np.zeros((1, ch), np.float32) for x in xs], ch)
    for b in banks:
        b.process(d.data_ptr(), longest, ch, fs, pos, frames=[len(x) for x in xs], reset_mask=reset_mask,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def feed_cuts(torch, banks, x, lengths, fs=FS8):
    """one mono stream: the programme lies on the device once and every call takes the next lengths[k] frames of it"""
    assert x.shape[1] == 1 and sum(lengths) == len(x)
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    at = 0
    for n in lengths:
        for b in banks:
            b.process(d.data_ptr() + 4 * at, n, 1, fs, POS1, stream=torch.cuda.current_stream().cuda_stream)
        at += n
    torch.cuda.synchronize()


def check_stream(stored, bounded, s, B, tag, measured=None):
    """stream s of the bounded bank against the restatement fed the twin's segments, and against the twin's record"""
    e = stored.fetch_segments(s)
    want = hr.results(e, B, FLOOR)
    h, wh = bounded.fetch_histogram(s), want["histogram"]
    assert h.segments == len(e) and h.tail.tobytes() == wh["tail"].tobytes(), (tag, h.segments, len(e))
    for f in ("gating_count", "short_term_count", "gating_sum", "short_term_sum"):      # counts exact, sums bit for bit
        differ = np.flatnonzero(getattr(h, f).view(np.uint64) != wh[f].view(np.uint64))
        assert len(differ) == 0, (tag, f, differ[:5], getattr(h, f)[differ[:5]], wh[f][differ[:5]])
    rec, twin_rec = bounded.fetch(s), stored.fetch(s)
    assert not rec.overflow and not twin_rec.overflow, tag
    for f in hr.RECORD_COUNTS:
        assert getattr(rec, f) == want[f], (tag, f, getattr(rec, f), want[f])
    for f in hr.RECORD_ENERGIES:
        assert bits(getattr(rec, f)) == bits(want[f]), (tag, f, getattr(rec, f), want[f])
    for f in LEVELS:
        assert np.isfinite(getattr(rec, f)), (tag, f)
        bar(f"program histogram: |d {f}| LU", abs(float(getattr(rec, f)) - float(want[f])), BAR, (tag, getattr(rec, f), want[f]))
    for f in SAME_AS_STORED:
        a, b = getattr(rec, f), getattr(twin_rec, f)
        assert (bits(a) == bits(b)) if isinstance(a, float) else a == b, (tag, f, a, b)
    d_i = abs(float(rec.integrated_lufs) - float(twin_rec.integrated_lufs))
    d_lra = abs(float(rec.loudness_range_lu) - float(twin_rec.loudness_range_lu))
    bar("program histogram: |d integrated_lufs| against the stored twin, LU", d_i, BAR, tag)
    assert d_lra <= hr.LRA_BOUND_LU, (tag, d_lra, rec.loudness_range_lu, twin_rec.loudness_range_lu)
    if measured is not None:
        measured["integrated vs stored, LU"] = max(measured.get("integrated vs stored, LU", 0.0), d_i)
        measured["range vs stored, LU"] = max(measured.get("range vs stored, LU", 0.0), d_lra)
    return h, rec


def fmt(measured):
    return {k: f"{v:.2e}" for k, v in measured.items()}


# ---------------------------------------------------------------- seeded programmes, both forms
@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_seeded_programmes_in_both_forms(torch_dev, omx, B, fs, ch, seeds):
    """each form against its own twin.  On the CPU, with the oracle's coefficients, the range is at most 0.040 LU from the stored mode's"""
    pos = capi.positions_fallback(ch)
    xs = [ref.programme(seed, fs, ch, ref.SEEDED_SECONDS) for seed in seeds]
    measured = {}
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        stored, bounded = twin(omx, fs, len(xs), ch, form)
        feed(torch_dev, (stored, bounded), xs, fs, ch, pos)
        assert stored.last_form() == bounded.last_form() == form
        for s in range(len(xs)):
            check_stream(stored, bounded, s, B, (fs, ch, seeds[s], form), measured)
    print(f"{fs} Hz {ch} ch:", fmt(measured))


# ---------------------------------------------------------------- cutting: bitwise the same however the programme is cut
def test_every_cut_of_a_programme_gives_the_same_bits(torch_dev, omx, B):
    x = hr.cut_programme()
    got = {}
    for name, lengths in hr.cut_schedules(len(x)).items():
        stored, bounded = twin(omx, FS8, 1, 1, FORM_REFERENCE_ORDER)
        feed_cuts(torch_dev, (stored, bounded), x, lengths)
        h, rec = check_stream(stored, bounded, 0, B, name)
        got[name] = (h.tobytes(), rec)
        print(name, len(lengths), "calls:", rec.integrated_lufs, rec.loudness_range_lu)
    first = got["one call"]
    for name, (h_bytes, rec) in got.items():
        assert h_bytes == first[0], name
        assert rec == first[1], (name, rec, first[1])


# ---------------------------------------------------------------- tiling: more new segments than any LDS tile
@pytest.mark.parametrize("kind", ["steps", "tone"])
def test_twelve_thousand_segments_in_one_call_and_in_calls_of_six(torch_dev, omx, B, kind):
    x = hr.long_programme(kind)
    assert len(x) == 12000 * hr.EDGE_SEG    # (the stored twins get one second more than that: a twin that is exactly full reports overflow)
    measured = {}
    stored, bounded = twin(omx, FS8, 1, 1, FORM_BY_SHAPE, capacity_seconds=hr.LONG_SECONDS + 1)
    feed_cuts(torch_dev, (stored, bounded), x, [len(x)])
    check_stream(stored, bounded, 0, B, (kind, "by shape"), measured)
    got = []
    for lengths in ([len(x)], [4800] * (len(x) // 4800)):
        stored, bounded = twin(omx, FS8, 1, 1, FORM_REFERENCE_ORDER, capacity_seconds=hr.LONG_SECONDS + 1)
        feed_cuts(torch_dev, (stored, bounded), x, lengths)
        h, rec = check_stream(stored, bounded, 0, B, (kind, len(lengths)), measured)
        got.append((h.tobytes(), rec))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    print(kind, fmt(measured), "largest bins:", int(h.gating_count.max()), int(h.short_term_count.max()))


# ---------------------------------------------------------------- ragged calls and resets
def test_ragged_bank_and_a_reset_in_the_middle_of_a_programme(torch_dev, omx, B):
    xs = hr.ragged_programmes()
    r, at = hr.RAGGED_RESET_STREAM, hr.RAGGED_RESET_AT
    empty = np.zeros((0, 1), np.float32)
    stored, bounded = twin(omx, FS8, len(xs), 1, FORM_REFERENCE_ORDER)
    feed(torch_dev, (stored, bounded), [x[:at] if s == r else x for s, x in enumerate(xs)], FS8, 1, POS1)
    before = [check_stream(stored, bounded, s, B, ("first part", s))[0].tobytes() for s in range(len(xs))]
    assert [bounded.fetch(s).segments for s in range(len(xs))] == [0, 2, 3, 31, at // hr.EDGE_SEG]
    mask = [1 if s == r else 0 for s in range(len(xs))]
    feed(torch_dev, (stored, bounded), [xs[s][at:] if s == r else empty for s in range(len(xs))], FS8, 1, POS1, reset_mask=mask)
    for s in range(len(xs)):
        h, rec = check_stream(stored, bounded, s, B, ("second part", s))
        if s != r:
            assert h.tobytes() == before[s], s
    fresh_stored, fresh = twin(omx, FS8, 1, 1, FORM_REFERENCE_ORDER)
    feed(torch_dev, (fresh_stored, fresh), [xs[r][at:]], FS8, 1, POS1)
    fh, frec = check_stream(fresh_stored, fresh, 0, B, "fresh bank, second part")
    assert h.tobytes() == fh.tobytes() and rec == frec and rec.frames == len(xs[r]) - at
    # a reset without samples (bank.reset): the flagged stream is empty again, the others keep their bits
    after = [bounded.fetch_histogram(s).tobytes() for s in range(len(xs))]
    for b in (stored, bounded):
        b.reset([0, 0, 0, 1, 0])
    for s in range(len(xs)):
        h, rec = check_stream(stored, bounded, s, B, ("after the bare reset", s))
        assert (h.segments == 0 and not h.gating_count.any() and not h.gating_sum.any() and len(h.tail) == 0 and rec.frames == 0
                and rec.max_momentary_energy == 0.0) if s == 3 else h.tobytes() == after[s], s


@pytest.mark.parametrize("n_streams", [3, 65])
def test_banks_of_3_and_65_streams(torch_dev, omx, B, n_streams):
    xs = hr.bank_programmes(n_streams)
    stored, bounded = twin(omx, FS8, n_streams, 1)
    feed(torch_dev, (stored, bounded), xs, FS8, 1, POS1)
    for s in range(n_streams):
        check_stream(stored, bounded, s, B, (n_streams, s))
    # a second call brings stream 1 one more segment and nothing to the rest
    more = [ref.programme(9, FS8, 1, 1)[:hr.EDGE_SEG] if s == 1 else np.zeros((0, 1), np.float32) for s in range(n_streams)]
    before = [bounded.fetch_histogram(s).tobytes() for s in range(n_streams)]
    feed(torch_dev, (stored, bounded), more, FS8, 1, POS1)
    for s in range(n_streams):
        h, _ = check_stream(stored, bounded, s, B, (n_streams, s, "second call"))
        assert (h.tobytes() != before[s]) if s == 1 else (h.tobytes() == before[s]), s


# ---------------------------------------------------------------- the ends of the bins' range
def test_range_of_the_bins(torch_dev, omx, B):
    progs = hr.range_programmes()
    names = list(progs)
    stored, bounded = twin(omx, FS8, len(names), 1, capacity_seconds=400)
    feed(torch_dev, (stored, bounded), [progs[n] for n in names], FS8, 1, POS1)
    got = {n: check_stream(stored, bounded, s, B, n) for s, n in enumerate(names)}
    h, rec = got["top bin"]                     # a 1 kHz sine of amplitude 64: above +30 LUFS
    assert rec.integrated_lufs > 30.0 and h.gating_count[999] == rec.gating_above_absolute == rec.gating_blocks and h.gating_count[:999].sum() == 0
    assert h.short_term_count[999] == rec.short_term_blocks > 0
    h, rec = got["below the gate"]              # -80 dBFS: blocks are counted, none is binned
    assert rec.gating_blocks == 47 and rec.gating_above_absolute == 0 and not h.gating_count.any() and not h.short_term_count.any()
    assert rec.integrated_lufs == np.float32(FLOOR) and rec.loudness_range_lu == 0.0 and rec.max_momentary_energy > 0.0
    h, rec = got["equal blocks"]                # whole periods per segment: thousands of blocks in one bin
    assert h.gating_count.max() >= 2990 and h.short_term_count.max() >= 2960, (h.gating_count.max(), h.short_term_count.max())
    h, rec = got["silence, then a tone"]
    assert 0 < rec.gating_above_absolute < rec.gating_blocks and abs(rec.integrated_lufs - rec.max_momentary_lufs) < 0.5


# ---------------------------------------------------------------- no overflow
def test_a_bounded_stream_goes_on_where_a_stored_one_is_full(torch_dev, omx, B):
    x = hr.overflow_programme()
    third = len(x) // 3
    small = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS8), 1, 1, hr.OVERFLOW_CAPACITY)
    small.set_option(capi.OPT_KERNEL_FORM, FORM_REFERENCE_ORDER)
    stored, bounded = twin(omx, FS8, 1, 1, FORM_REFERENCE_ORDER)
    feed_cuts(torch_dev, (small, stored, bounded), x, [third, third, len(x) - 2 * third])
    full = small.fetch(0)
    assert full.overflow and full.frames == hr.OVERFLOW_CAPACITY * int(FS8) and full.segments == hr.OVERFLOW_CAPACITY * 10
    _, rec = check_stream(stored, bounded, 0, B, "60 s")
    assert not rec.overflow and rec.frames == len(x) == hr.OVERFLOW_SECONDS * int(FS8) and rec.segments == 600


# ---------------------------------------------------------------- peaks
def test_peaks_of_a_bounded_bank_are_the_stored_twins(torch_dev, omx, B):
    xs = [hr.cut_programme(), hr.overflow_programme()[:123457]]
    stored, bounded = twin(omx, FS8, 2, 1, FORM_REFERENCE_ORDER, peaks=True)
    for lo, hi in ((0, 50001), (50001, 10 ** 9)):
        feed(torch_dev, (stored, bounded), [x[lo:hi] for x in xs], FS8, 1, POS1)
    for s in range(2):
        assert bounded.fetch_peaks(s).tobytes() == stored.fetch_peaks(s).tobytes(), s
        _, rec = check_stream(stored, bounded, s, B, ("peaks", s))
        assert rec.max_true_peak_db == stored.fetch_peaks(s).max_true_peak_db > FLOOR


# ---------------------------------------------------------------- refusals
def test_what_needs_the_segments_is_refused_and_changes_nothing(torch_dev, omx, B):
    stored, bounded = twin(omx, FS8, 1, 1)
    feed(torch_dev, (stored, bounded), [hr.cut_programme()[:100 * hr.EDGE_SEG]], FS8, 1, POS1)
    h0, rec0 = check_stream(stored, bounded, 0, B, "before")
    rows = torch_dev.zeros((40 * 16,), dtype=torch_dev.uint8).cuda()
    calls = {"fetch_segments": lambda: bounded.fetch_segments(0, 0, 4), "timeline": lambda: bounded.timeline(rows.data_ptr(), 0, 1, 4),
             "fetch_timeline": lambda: bounded.fetch_timeline(0, 0, 1, 4), "measure_intervals": lambda: bounded.measure_intervals([(0, 0, 50)]),
             "fetch_intervals": lambda: bounded.fetch_intervals([(0, 0, 50)])}
    for name, call in calls.items():
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_UNSUPPORTED, (name, err.value.status)
        assert bounded.fetch(0) == rec0 and bounded.fetch_histogram(0).tobytes() == h0.tobytes(), name
    assert not rows.cpu().numpy().any()
    with pytest.raises(capi.OmxError) as err:
        stored.fetch_histogram(0)
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as err:
        bounded.fetch_histogram(1)
    assert err.value.status == capi.ERR_INVALID


# ---------------------------------------------------------------- EBU cases through the product
def test_ebu_3341_3_and_3342_3_through_the_product(torch_dev, omx, B):
    fs, pos = 48000.0, capi.positions_fallback(2)
    cases = [(name, spans, want) for name, spans, want in ref.EBU_3341 + ref.EBU_3342 if name in hr.EBU_THROUGH_THE_PRODUCT]
    assert len(cases) == 2
    xs = [ref.tone_programme(fs, spans) for _, spans, _ in cases]
    stored, bounded = twin(omx, fs, 2, 2)
    feed(torch_dev, (stored, bounded), xs, fs, 2, pos)
    for s, (name, _, want) in enumerate(cases):
        _, rec = check_stream(stored, bounded, s, B, name)
        print(name, rec.integrated_lufs, rec.loudness_range_lu)
        if name.startswith("3341"):
            assert abs(rec.integrated_lufs - want) <= 0.1, (name, rec.integrated_lufs)
        else:
            assert abs(rec.loudness_range_lu - want) <= 1.0, (name, rec.loudness_range_lu)


def test_c99_demo_runs(torch_dev, omx, tmp_path):
    out = subprocess.run([build_demo(tmp_path)], check=True, capture_output=True, text=True, timeout=300).stdout
    print(out)
    lines = out.strip().splitlines()
    assert lines[1].startswith("stored  capacity 1 s: overflow 1 frames 48000 segments 10")
    assert lines[2].startswith("bounded             : overflow 0 frames 288000 segments 60")
    assert lines[-1] == "histogram: segments 60 tail 29" and sum(line.startswith("gating bin") for line in lines) >= 2

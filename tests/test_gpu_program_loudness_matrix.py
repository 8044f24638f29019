"""Programme loudness bank on the GPU (`-m gpu`), the wider matrix: every accepted rate and channel count in both evaluation orders,
inputs that are hard for the time-parallel scan (DC, rumble, a 100 dB drop, 90 s at full scale), the low end of the rate range, bank
shapes that do not fill a lane group, ragged calls that change form inside open segments, the result pass on its own up to one hour
of segments, and the error returns.

The referee is the numpy restatement (tests/program_loudness_ref.py: scipy's sequential f64 lfilter).  Bars: 1e-4 LU on every LUFS /
LU field, counts exact; 1e-4 dB between the two forms on gating blocks above -70 LUFS.  Every input keeps a gate margin of 2e-3 LU in
the restatement: tests/test_cpu_program_loudness_inputs.py asserts that without a device."""
import ctypes as C

import numpy as np
import pytest

import program_loudness_ref as ref
from openmeters_amd import banks, capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import FORM_BY_SHAPE, FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, ProgramLoudnessBank, ProgramLoudnessRecord
from parity import bar
from test_gpu_program_loudness import (BAR, FLOOR, check_record, coefficients, ragged_schedule, run_once, run_schedule,  # noqa: F401
                                       torch_dev)

pytestmark = pytest.mark.gpu
ENERGY_MEANS = {"integrated_energy": "gating_above_relative", "relative_threshold_energy": "gating_above_absolute"}


def check_result_pass(bank, s, tag, measured=None):
    """the result pass on its own: ref.results of the stored e[] must reproduce the record — counts exact, LUFS / LU fields at the
    bar, energies within ref.energy_bound (a mean of n blocks: n + 30 roundings; any other energy field is a single block)"""
    rec, e = bank.fetch(s), bank.fetch_segments(s)
    want = ref.results(e, FLOOR)
    assert want["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN, (tag, want["gate_margin"])
    want["frames"] = rec.frames
    check_record(rec, want, ("result pass", tag))
    for f in ProgramLoudnessRecord.ENERGY_FIELDS:
        got, exp = float(getattr(rec, f)), float(want[f])
        bound = ref.energy_bound(want[ENERGY_MEANS[f]] if f in ENERGY_MEANS else 0)
        assert abs(got - exp) <= bound * exp, (tag, f, got, exp, abs(got - exp) / max(exp, 1e-300), bound)
        if measured is not None and exp > 0.0:
            measured[f] = max(measured.get(f, 0.0), abs(got - exp) / exp)
    return rec


def gating_distance(e_a, e_b):
    """largest |L(a) - L(b)| over the gating blocks of a above -70 LUFS, dB"""
    a, b = ref.sliding_mean(np.asarray(e_a), 4), ref.sliding_mean(np.asarray(e_b), 4)
    keep = a > ref.ABSOLUTE_GATE
    return float(np.abs(ref.level(a[keep]) - ref.level(b[keep])).max()) if keep.any() else 0.0


def upload(torch, xs, ch, pad=0, fill=0.0):
    longest = max(len(x) for x in xs) + pad
    host = np.full((len(xs), longest, ch), fill, np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    return torch.from_numpy(host).cuda(), longest


def fmt(measured):
    return {k: f"{v:.2e}" for k, v in measured.items()}


# ---------------------------------------------------------------- 1. rates and layouts, both forms
BIT_IDENTITY = {(9000.0, 3), (11025.0, 5)}   # a low rate (item = segment = 900 frames) and an odd segment (1103 frames)


@pytest.mark.parametrize("fs,ch,seconds,seeds", ref.MATRIX_CASES)
def test_rates_and_layouts_against_the_restatement_in_both_forms(torch_dev, omx, oracle, fs, ch, seconds, seeds):
    """each pinned form against the restatement, form against form on gating blocks, last_form(), the result pass on its own; at
    9 kHz / 3 ch and 11 025 Hz / 5 ch also the reference order's bit-identical segments for one call and 256-frame calls"""
    pos, co = capi.positions_fallback(ch), coefficients(oracle, fs)
    xs = [ref.programme(seed, fs, ch, seconds) for seed in seeds]
    want = [ref.restate(x, fs, pos, co) for x in xs]
    segs, measured, energies = {}, {}, {}
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_once(torch_dev, omx, xs, fs, ch, pos, form)
        assert bank.last_form() == ref.expected_form(form, fs)
        for s in range(len(xs)):
            assert want[s]["gate_margin"] >= ref.GATE_MARGIN_MIN
            check_record(bank.fetch(s), want[s], (fs, ch, seeds[s], form), measured)
            check_result_pass(bank, s, (fs, ch, seeds[s], form), energies)
        segs[form] = [bank.fetch_segments(s) for s in range(len(xs))]
    worst = max(gating_distance(segs[FORM_REFERENCE_ORDER][s], segs[FORM_TIME_PARALLEL][s]) for s in range(len(xs)))
    vs_ref = max(gating_distance(want[s]["e"], segs[form][s]) for s in range(len(xs)) for form in segs)
    print(f"{fs} Hz {ch} ch: time-parallel vs reference order, gating blocks above -70 LUFS: {worst:.2e} dB; either form vs restatement, "
          f"gating blocks: {vs_ref:.2e} dB; records vs restatement (LU): {fmt(measured)}; result pass, energies (relative): {fmt(energies)}")
    bar("program loudness: time-parallel vs reference-order gating blocks, dB", worst, BAR, (fs, ch))
    if (fs, ch) in BIT_IDENTITY:
        T = len(xs[0])
        blocks = [np.full(len(xs), min(256, T - t), np.uint32) for t in range(0, T, 256)]
        bank = run_schedule(torch_dev, omx, xs, fs, ch, pos, blocks)
        assert bank.last_form() == FORM_REFERENCE_ORDER
        for s in range(len(xs)):
            got = bank.fetch_segments(s)
            assert got.tobytes() == segs[FORM_REFERENCE_ORDER][s].tobytes(), (fs, ch, s, np.abs(got - segs[FORM_REFERENCE_ORDER][s]).max())


# ---------------------------------------------------------------- 2. hard inputs for the scan
def hard_run(torch, omx, oracle, xs, names, fs, ch, pos):
    """each programme whole in one call: pinned reference order, pinned time-parallel, and by shape (which must pick the
    time-parallel form: a small bank, a long call) — every form against the restatement, time-parallel against reference order"""
    co = coefficients(oracle, fs)
    want = [ref.restate(x, fs, pos, co) for x in xs]
    for w in want:
        assert w["gate_margin"] >= ref.GATE_MARGIN_MIN
    d, longest = upload(torch, xs, ch)
    segs, banks_, ran = {}, {}, {}
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, FORM_BY_SHAPE):
        bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, 200)
        bank.set_option(capi.OPT_KERNEL_FORM, form)
        bank.process(d.data_ptr(), longest, ch, fs, pos, frames=[len(x) for x in xs], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        banks_[form], ran[form], segs[form] = bank, bank.last_form(), [bank.fetch_segments(s) for s in range(len(xs))]
    # every figure first, then the assertions
    for s in range(len(xs)):
        rec = {form: banks_[form].fetch(s) for form in banks_}
        print(f"{fs:.0f} Hz {ch} ch {names[s]}:", "; ".join(
            f"form {form} (ran {ran[form]}) vs restatement: gating blocks {gating_distance(want[s]['e'], segs[form][s]):.2e} dB, momentary "
            f"{abs(float(rec[form].momentary_lufs) - float(want[s]['momentary_lufs'])):.2e} LU, integrated "
            f"{abs(float(rec[form].integrated_lufs) - float(want[s]['integrated_lufs'])):.2e} LU" for form in banks_),
            "; vs reference order, gating blocks above -70 LUFS:", ", ".join(
            f"form {form} {gating_distance(segs[FORM_REFERENCE_ORDER][s], segs[form][s]):.2e} dB" for form in (FORM_TIME_PARALLEL, FORM_BY_SHAPE)))
    for form in banks_:
        # by shape: S <= 4 streams of <= 8 channels are one wavefront of slots and the call brings hundreds of work items, so the rule
        # picks the time-parallel form; above ref.TIME_PARALLEL_MAX_RATE the reference order runs whatever is asked (documented)
        assert ran[form] == ref.expected_form(form or FORM_TIME_PARALLEL, fs), (fs, ch, form, ran[form])
        for s in range(len(xs)):
            check_record(banks_[form].fetch(s), want[s], (fs, ch, names[s], form))
            check_result_pass(banks_[form], s, (fs, ch, names[s], form))
    for form in (FORM_TIME_PARALLEL, FORM_BY_SHAPE):
        for s in range(len(xs)):
            bar("program loudness: time-parallel vs reference-order gating blocks, dB",
                gating_distance(segs[FORM_REFERENCE_ORDER][s], segs[form][s]), BAR, (fs, ch, names[s], form))


@pytest.mark.parametrize("ch", [1, 8])
@pytest.mark.parametrize("fs", ref.HARD_RATES)
def test_hard_inputs_for_the_scan(torch_dev, omx, oracle, fs, ch):
    """a DC offset of 0.5, a 5 Hz and a 15 Hz sine of 0.5 under noise at -60 dBFS (the filter state is large, the output small), and
    full-scale noise followed by a 100 dB drop: at 48 / 96 / 192 kHz, at the highest rate of the time-parallel form and at the highest
    rate the bank accepts, mono and 7.1"""
    pos = ref.SURROUND_71 if ch == 8 else capi.positions_fallback(ch)
    hard_run(torch_dev, omx, oracle, [ref.hard_input(kind, fs, ch) for kind in ref.HARD_KINDS], ref.HARD_KINDS, fs, ch, pos)


@pytest.mark.parametrize("ch", [1, 8])
def test_ninety_seconds_at_full_scale_then_a_quiet_passage(torch_dev, omx, oracle, ch):
    fs, pos = 48000.0, ref.SURROUND_71 if ch == 8 else capi.positions_fallback(ch)
    hard_run(torch_dev, omx, oracle, [ref.long_loud_then_quiet(fs, ch)], ["90 s loud, then quiet"], fs, ch, pos)


# ---------------------------------------------------------------- 3. the low end of the rate range
def test_rates_below_the_limit_are_refused_and_leave_a_running_programme_untouched(torch_dev, omx, oracle):
    """below ref.MIN_RATE the K-weighting filter is unstable: OMX_ERR_UNSUPPORTED, with and without a reset in the same call, on a fresh
    bank and on a running one, whose records and segments do not change and which goes on as if nothing had been asked"""
    fs, ch, pos = 8000.0, 1, capi.positions_fallback(1)
    x = ref.programme(1, fs, ch, 40)
    d = torch_dev.from_numpy(x[None]).cuda()
    half = len(x) // 2 + 321
    fresh = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, 60)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, 60)
    bank.process(d.data_ptr(), len(x), ch, fs, pos, frames=[half])
    before, segs, form = bank.fetch(0), bank.fetch_segments(0), bank.last_form()
    for rate in (ref.MIN_RATE - 1.0, ref.MIN_RATE - 0.5, 3000.0, 1681.0, 1000.0, 999.0, 1.0):
        for mask in (None, [1]):
            for b in (fresh, bank):
                with pytest.raises(capi.OmxError) as err:
                    b.process(d.data_ptr(), len(x), ch, rate, pos, frames=[100], reset_mask=mask)
                assert err.value.status == capi.ERR_UNSUPPORTED, (rate, mask)
        assert bank.fetch(0) == before and bank.fetch_segments(0).tobytes() == segs.tobytes() and bank.last_form() == form
        assert fresh.fetch(0).frames == 0 and fresh.last_form() == 0
    rest = torch_dev.from_numpy(np.ascontiguousarray(x[None, half:])).cuda()
    bank.process(rest.data_ptr(), len(x) - half, ch, fs, pos)
    check_record(bank.fetch(0), ref.restate(x, fs, pos, coefficients(oracle, fs)), "after the refusals")
    fresh.process(d.data_ptr(), len(x), ch, ref.MIN_RATE, pos, frames=[1000])       # the limit itself is accepted
    assert fresh.fetch(0).frames == 1000 and fresh.fetch(0).segments == 1000 // ref.segment_frames(ref.MIN_RATE)


# ---------------------------------------------------------------- 4. bank shapes and ragged calls
def play(torch, omx, xs, fs, ch, pos, schedule, forms, positions=None, capacity_seconds=60):
    """run_schedule with a form per call; after EVERY call each stream's frames and block counts are checked exactly"""
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, capacity_seconds)
    cursor, seg = [0] * len(xs), ref.segment_frames(fs)
    for k, counts in enumerate(schedule):
        cap = max(int(max(counts)), 1)
        host = np.zeros((len(xs), cap, ch), np.float32)
        for s, n in enumerate(counts):
            host[s, :n] = xs[s][cursor[s]:cursor[s] + int(n)]
            cursor[s] += int(n)
        d = torch.from_numpy(host).cuda()
        bank.set_option(capi.OPT_KERNEL_FORM, int(forms[k]))
        bank.process(d.data_ptr(), cap, ch, fs, positions[k] if positions else pos, frames=np.asarray(counts, np.uint32),
                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if max(counts) > 0:
            assert bank.last_form() == forms[k], (k, counts, forms[k], bank.last_form())
        for s in range(len(xs)):
            rec = bank.fetch(s)
            n = cursor[s] // seg
            assert (rec.frames, rec.segments, rec.gating_blocks, rec.short_term_blocks, rec.overflow) == \
                (cursor[s], n, max(n - 3, 0), max(n - 29, 0), False), (k, s, counts, rec)
    return bank


@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("S", [1, 5, 33, 65])
def test_time_parallel_bank_shapes_never_read_past_a_streams_frames(torch_dev, omx, oracle, S, ch):
    """banks that do not fill the last lane group (G = 32 streams per wavefront at 2 ch, 16 at 3 ch), streams of five different lengths,
    frames_capacity beyond every one of them: the padding (memory the call owns) holds zeros, then 1e30, then NaN — the records and
    segments must be the same bits, and those of the restatement at the bar"""
    fs, pos, co = ref.SHAPE_RATE, capi.positions_fallback(ch), coefficients(oracle, ref.SHAPE_RATE)
    xs = ref.shape_programmes(ch, S)
    want = [ref.restate(x, fs, pos, co) for x in xs[:len(ref.SHAPE_POOL[ch])]]
    seen = {}
    for name, fill in (("zeros", 0.0), ("1e30", 1e30), ("NaN", np.nan)):
        d, cap = upload(torch_dev, xs, ch, pad=2500, fill=fill)
        assert cap > max(len(x) for x in xs)
        bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch, 60)
        bank.set_option(capi.OPT_KERNEL_FORM, FORM_TIME_PARALLEL)
        bank.process(d.data_ptr(), cap, ch, fs, pos, frames=[len(x) for x in xs], stream=torch_dev.cuda.current_stream().cuda_stream)
        torch_dev.cuda.synchronize()
        assert bank.last_form() == FORM_TIME_PARALLEL
        seen[name] = [(bank.fetch(s), bank.fetch_segments(s).tobytes()) for s in range(S)]
        for s in range(S):
            assert seen[name][s] == seen["zeros"][s], (name, S, ch, s, seen[name][s][0], seen["zeros"][s][0])
        if name == "zeros":
            for s in range(S):
                w = want[s % len(want)]
                assert w["gate_margin"] >= ref.GATE_MARGIN_MIN
                check_record(bank.fetch(s), w, ("bank shape", S, ch, s))
                check_result_pass(bank, s, ("bank shape", S, ch, s))


@pytest.mark.parametrize("open_segment", [False, True])
@pytest.mark.parametrize("form", [FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL])
@pytest.mark.parametrize("ch", [2, 3])
def test_one_call_with_no_frames_one_frame_and_counts_around_a_work_item(torch_dev, omx, oracle, ch, form, open_segment):
    """streams of one call bring 0, 1, item - 1, item, item + 1 and 20 items + 17 frames, into a fresh bank or into one whose streams have
    an open segment of 1234 frames; then the rest of every programme: counts exact after every call, final records against the
    restatement"""
    fs, pos, item = ref.SHAPE_RATE, capi.positions_fallback(ch), 1024
    assert item < ref.segment_frames(fs)
    xs = ref.shape_programmes(ch, 6)
    schedule = ([[1234] * 6] if open_segment else []) + [[0, 1, item - 1, item, item + 1, 20 * item + 17]]
    taken = np.sum(np.asarray(schedule), axis=0)
    schedule.append([len(x) - int(t) for x, t in zip(xs, taken)])
    bank = play(torch_dev, omx, xs, fs, ch, pos, schedule, [form] * len(schedule))
    for s in range(6):
        want = ref.restate(xs[s], fs, pos, coefficients(oracle, fs))
        assert want["gate_margin"] >= ref.GATE_MARGIN_MIN
        check_record(bank.fetch(s), want, ("item edges", ch, form, open_segment, s))
        check_result_pass(bank, s, ("item edges", ch, form, open_segment, s))


@pytest.mark.parametrize("ch", [2, 3])
def test_ragged_calls_that_change_form_inside_open_segments(torch_dev, omx, oracle, ch):
    """random per-stream frame counts per call (0 included), the form of every call drawn from {reference order, time-parallel}: counts
    exact after every call, final records against the restatement"""
    fs, pos = ref.SHAPE_RATE, capi.positions_fallback(ch)
    xs = ref.shape_programmes(ch, 5)
    rng = np.random.default_rng(40 + ch)
    schedule = ragged_schedule(rng, [len(x) for x in xs], 1, 9000)
    forms = rng.integers(1, 3, len(schedule))
    assert len(schedule) > 30 and 0.25 < np.mean(forms == 1) < 0.75
    bank = play(torch_dev, omx, xs, fs, ch, pos, schedule, forms)
    measured = {}
    for s in range(5):
        want = ref.restate(xs[s], fs, pos, coefficients(oracle, fs))
        assert want["gate_margin"] >= ref.GATE_MARGIN_MIN
        check_record(bank.fetch(s), want, ("ragged, mixed forms", ch, s), measured)
        check_result_pass(bank, s, ("ragged, mixed forms", ch, s))
        print(f"{ch} ch stream {s}: gating blocks vs restatement {gating_distance(want['e'], bank.fetch_segments(s)):.2e} dB")
    print(f"ragged calls, mixed forms, {ch} ch, {len(schedule)} calls: records vs restatement (LU): {fmt(measured)}")


@pytest.mark.parametrize("ch", [2, 3])
def test_a_stream_in_a_mixed_time_parallel_bank_equals_the_stream_alone(torch_dev, omx, ch):
    fs, pos, S = ref.SHAPE_RATE, capi.positions_fallback(ch), 33
    xs = ref.shape_programmes(ch, S)
    mixed = run_once(torch_dev, omx, xs, fs, ch, pos, FORM_TIME_PARALLEL, capacity_seconds=60)
    for s in (0, 7, 18, 32):
        alone = run_once(torch_dev, omx, xs[s:s + 1], fs, ch, pos, FORM_TIME_PARALLEL, capacity_seconds=60)
        assert alone.last_form() == mixed.last_form() == FORM_TIME_PARALLEL
        assert alone.fetch(0) == mixed.fetch(s), (ch, s)
        d = gating_distance(alone.fetch_segments(0), mixed.fetch_segments(s))
        bar("program loudness: a stream alone vs in a mixed bank, gating blocks, dB", d, BAR, (ch, s))


@pytest.mark.parametrize("form", [FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL])
def test_positions_that_change_between_two_calls(torch_dev, omx, oracle, form):
    """no reset: a sample takes the weights of the call it arrived in (rear weights 1.41 in the first call, front weights in the second;
    the call boundary lies inside a segment)"""
    fs, ch, seconds, seed = ref.WEIGHT_CHANGE_CASE
    x = ref.programme(seed, fs, ch, seconds)
    half = len(x) // 2 + 777
    assert half % ref.segment_frames(fs) != 0
    calls = [(half, ref.REAR_POSITIONS), (len(x) - half, ref.FRONT_POSITIONS)]
    bank = play(torch_dev, omx, [x], fs, ch, None, [[n] for n, _ in calls], [form, form], positions=[p for _, p in calls])
    want = ref.results(ref.segment_energies_per_call(x, fs, calls, coefficients(oracle, fs)), FLOOR)
    assert want["gate_margin"] >= ref.GATE_MARGIN_MIN
    want["frames"] = len(x)
    check_record(bank.fetch(0), want, ("positions change", form))
    check_result_pass(bank, 0, ("positions change", form))


# ---------------------------------------------------------------- 5. the result pass on its own, one hour of segments
def test_result_pass_over_one_hour_programmes_and_overflow_at_the_last_segment(torch_dev, omx):
    """8 kHz mono, capacity 3600 s, two streams in calls of very different lengths (form by shape): a programme of steady tones (runs of
    thousands of equal short-term blocks: equal keys in the radix select, ranks inside a run) that ends 1.5 segments short, and one of
    stepped levels that fills the storage exactly with its last segment and then gets one more call"""
    torch = torch_dev
    fs, ch, pos, seg = ref.HOUR_RATE, 1, capi.positions_fallback(1), ref.segment_frames(ref.HOUR_RATE)
    full = 36000 * seg
    xs = [ref.hour_programme("tone")[:full - seg - seg // 2], ref.hour_programme("steps")]
    assert len(xs[1]) == full
    counts = [list(c) for c in ref.HOUR_CALLS]
    assert [sum(c[s] for c in counts) for s in range(2)] == [len(xs[0]), full]
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 2, ch, ref.HOUR_SECONDS)
    cursor, measured, forms = [0, 0], {}, []
    for k, c in enumerate(counts):
        host = np.zeros((2, max(c), ch), np.float32)
        for s in range(2):
            host[s, :c[s]] = xs[s][cursor[s]:cursor[s] + c[s]]
            cursor[s] += c[s]
        d = torch.from_numpy(host).cuda()
        bank.process(d.data_ptr(), max(c), ch, fs, pos, frames=c, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        forms.append(bank.last_form())
        for s in range(2):
            rec = check_result_pass(bank, s, ("one hour", k, s), measured)
            assert rec.frames == cursor[s] and rec.segments == cursor[s] // seg
            assert rec.overflow == (rec.segments == 36000)
    # by shape: a call is time-parallel from four work items (4 x 800 frames) on
    assert forms == [FORM_TIME_PARALLEL, FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, FORM_TIME_PARALLEL], forms
    last = [bank.fetch(s) for s in range(2)]
    assert last[1].overflow and last[1].segments == 36000 and last[1].frames == full and not last[0].overflow and last[0].segments == 35998
    assert last[0].lra_low_energy < last[0].lra_high_energy and last[1].gating_blocks > last[1].gating_above_absolute > last[1].gating_above_relative > 0
    d = torch.from_numpy(np.full((2, 5000, ch), 0.25, np.float32)).cuda()       # one more call: the full stream takes nothing
    bank.process(d.data_ptr(), 5000, ch, fs, pos, frames=[100, 5000])
    assert bank.fetch(1) == last[1]
    rec = check_result_pass(bank, 0, ("one hour", "after", 0), measured)
    assert rec.frames == last[0].frames + 100 and rec.segments == 35998 and not rec.overflow
    check_result_pass(bank, 1, ("one hour", "after", 1), measured)
    print(f"one hour at 8 kHz: I {last[0].integrated_lufs:.3f} / {last[1].integrated_lufs:.3f} LUFS, LRA {last[0].loudness_range_lu:.3f} / "
          f"{last[1].loudness_range_lu:.3f} LU; result pass vs ref.results of the same e[], energies (relative): {fmt(measured)}")


def test_result_pass_over_four_hours(torch_dev, omx):
    """144 000 segments in one stream (8 kHz mono, 115 M frames in one call, time-parallel by shape): the size DESIGN.md quotes a time
    for — 563 strides of the 256 threads, a radix select over 68 000 keys"""
    fs, ch, pos = ref.HOUR_RATE, 1, capi.positions_fallback(1)
    x = ref.hour_programme("steps", seconds=ref.FOUR_HOURS_SECONDS, seed=ref.FOUR_HOURS_SEED)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, ref.FOUR_HOURS_SECONDS)
    d = torch_dev.from_numpy(x[None]).cuda()
    bank.process(d.data_ptr(), len(x), ch, fs, pos, stream=torch_dev.cuda.current_stream().cuda_stream)
    torch_dev.cuda.synchronize()
    assert bank.last_form() == FORM_TIME_PARALLEL
    measured = {}
    rec = check_result_pass(bank, 0, "four hours", measured)
    assert rec.segments == 144000 and rec.overflow and rec.frames == len(x)
    assert rec.gating_blocks > rec.gating_above_absolute > rec.gating_above_relative > 0 and rec.short_term_above_relative > 30000
    print(f"four hours at 8 kHz: I {rec.integrated_lufs:.3f} LUFS, LRA {rec.loudness_range_lu:.3f} LU, {rec.gating_above_relative} / {rec.gating_blocks} "
          f"gating blocks above both gates; result pass vs ref.results of the same e[], energies (relative): {fmt(measured)}")


# ---------------------------------------------------------------- 6. small things
def test_note_snapshots_with_per_stream_block_counts_on_the_device(torch_dev, omx):
    """d_n_blocks: 0, 1, n_blocks and a count above n_blocks (clamped) — against the maximum over the snapshots fetched on the host"""
    fs, ch, pos, S, blocks = 48000.0, 2, capi.positions_fallback(2), 4, 16
    xs = np.stack([ref.programme(seed, fs, ch, 1)[:256 * blocks] for seed in (1, 3, 4, 5)])
    meter = banks.LoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch, 60)
    d = torch_dev.from_numpy(np.ascontiguousarray(xs)).cuda()
    snaps = meter.process_device(d.data_ptr(), 256, blocks, ch, fs, pos)
    counts = [0, 1, blocks, 40]
    d_counts = torch_dev.tensor(counts, dtype=torch_dev.int32).cuda()
    bank.note_snapshots(snaps, blocks, d_n_blocks=d_counts.data_ptr())
    torch_dev.cuda.synchronize()
    for s in range(S):
        want = np.float32(FLOOR)
        for k in range(min(counts[s], blocks)):
            want = max(want, meter.fetch(s, k).true_peak_db[:ch].max())
        assert bank.fetch(s).max_true_peak_db == want, (s, bank.fetch(s).max_true_peak_db, want)
    assert bank.fetch(0).max_true_peak_db == np.float32(FLOOR) and bank.fetch(2).max_true_peak_db > bank.fetch(0).max_true_peak_db


def test_error_returns_leave_the_records_unchanged(torch_dev, omx):
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    xs = [ref.programme(seed, fs, ch, 2) for seed in (0, 1)]
    bank = run_once(torch_dev, omx, xs, fs, ch, pos, FORM_TIME_PARALLEL, capacity_seconds=60)
    d = torch_dev.from_numpy(np.stack(xs)).cuda()
    before = [(bank.fetch(s), bank.fetch_segments(s).tobytes()) for s in range(2)]
    n = before[0][0].segments
    assert n == 20

    def refused(status, call, *args, **kw):
        with pytest.raises(capi.OmxError) as err:
            call(*args, **kw)
        assert err.value.status == status, (args, kw, err.value.status)
        assert [(bank.fetch(s), bank.fetch_segments(s).tobytes()) for s in range(2)] == before and bank.last_form() == FORM_TIME_PARALLEL

    refused(capi.ERR_INVALID, bank.fetch_segments, 0, n + 1, 0)           # first > segments
    refused(capi.ERR_INVALID, bank.fetch_segments, 0, 0, n + 1)           # count too large
    refused(capi.ERR_INVALID, bank.fetch_segments, 0, n, 1)
    raw = omx.fn("program_loudness_bank_fetch_segments", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
    assert raw(bank._h, 0, 5, 2 ** 64 - 3, np.zeros(8).ctypes.data) == capi.ERR_INVALID      # first + count wraps around
    assert len(bank.fetch_segments(0, n, 0)) == 0 and bank.fetch_segments(1, n - 1, 1).tobytes() == before[1][1][-8:]
    refused(capi.ERR_INVALID, bank.fetch_segments, 2, 0, 0)               # stream index out of range
    refused(capi.ERR_INVALID, bank.fetch, 2)
    refused(capi.ERR_INVALID, bank.set_option, capi.OPT_KERNEL_TIMING, 1)  # another option
    refused(capi.ERR_INVALID, bank.set_option, capi.OPT_KERNEL_FORM, 3)
    refused(capi.ERR_INVALID, bank.process, d.data_ptr(), 1000, ch, fs, pos, frames=[1001, 0])       # frames[s] > frames_capacity
    refused(capi.ERR_INVALID, bank.process, 0, 1000, ch, fs, pos, frames=[0, 10])                    # null pcm with frames
    refused(capi.ERR_INVALID, bank.process, d.data_ptr(), 2 ** 32, ch, fs, pos, frames=[10, 10])     # frames_capacity above 2^32 - 1
    for channels in (0, 9, 255):                                                                     # channels outside 1 .. 8
        refused(capi.ERR_INVALID, bank.process, d.data_ptr(), 1000, channels, fs, pos, frames=[10, 10])
        refused(capi.ERR_INVALID, bank.process, d.data_ptr(), 1000, channels, fs, pos, frames=[10, 10], reset_mask=[1, 1])
    for args in ((0, 2, 60), (2, 2, 0)):                                                             # create: 0 streams, 0 seconds
        with pytest.raises(capi.OmxError) as err:
            ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), *args)
        assert err.value.status == capi.ERR_INVALID, args
    create = omx.fn("program_loudness_bank_create", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
    cfg, handle = LoudnessConfig(sample_rate=fs).to_c(), C.c_void_p()
    assert create(None, 2, 2, 60, C.byref(handle)) == capi.ERR_INVALID and not handle.value         # create: null pointers
    assert create(C.byref(cfg), 2, 2, 60, None) == capi.ERR_INVALID
    # and the bank goes on: a null pcm is fine when nobody brings frames
    assert bank.process(0, 0, ch, fs, pos, frames=[0, 0]) == 0
    assert [(bank.fetch(s), bank.fetch_segments(s).tobytes()) for s in range(2)] == before

"""Programme bank peaks on the GPU (`-m gpu`): ProgramLoudnessBank.set_peaks / fetch_peaks (include/omx/program_peaks.h) against the
numpy restatement (tests/program_peaks_ref.py, pinned to the oracle's sample-by-sample meter by tests/test_cpu_program_peaks.py).

Bars: the linear peaks (f32 bit patterns) and the frame numbers are EXACT — the interpolator is a fixed-order f32 sum and a maximum
does not care about order; dB fields within 1e-4 dB (the project's loudness bar) of 20 log10(peak) computed in f64 and floored;
records of the same programme cut into calls in different ways are bitwise equal."""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import program_loudness_ref as lref
import program_peaks_ref as ref
from openmeters_amd import banks, capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import ProgramLoudnessBank
from parity import bar

pytestmark = pytest.mark.gpu
BAR = 1e-4
FLOOR = -99.9
F32_FLOOR = np.float32(FLOOR)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def coeffs(oracle):
    return ref.coefficients(oracle)


def feed(torch, bank, xs, fs, ch, schedule, resets=None):
    """schedule: per call an array of per-stream frame counts; every stream walks its own programme"""
    pos = capi.positions_fallback(ch)
    cursor = [0] * len(xs)
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


def new_bank(omx, fs, n_streams, ch, peaks=True, capacity_seconds=120):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n_streams, ch, capacity_seconds)
    if peaks:
        bank.set_peaks(True)
    return bank


def whole(xs):
    return [np.array([len(x) for x in xs], np.uint32)]


def check_peaks(rec, want, tag):
    """linear peaks and frames exact, dB within 1e-4 of the f64 value, the rest as defined"""
    assert rec.frames == want["frames"] and rec.channels == want["channels"] and rec.oversampling == want["oversampling"], (tag, rec, want)
    for f in ("true_peak", "sample_peak"):
        assert getattr(rec, f).view(np.uint32).tolist() == want[f].view(np.uint32).tolist(), (tag, f, getattr(rec, f), want[f])
    for f in ("true_peak_frame", "sample_peak_frame"):
        assert getattr(rec, f).tolist() == want[f].tolist(), (tag, f, getattr(rec, f), want[f])
    worst = 0.0
    for f, lin in (("true_peak_db", "true_peak"), ("sample_peak_db", "sample_peak")):
        for c in range(ref.MAX_CHANNELS):
            exact = ref.db_f64(want[lin][c], FLOOR)
            got = float(getattr(rec, f)[c])
            d = 0.0 if got == exact else abs(got - exact)     # (an infinite peak: inf on both sides)
            worst = max(worst, bar(f"program peaks: |d {f}| dB", d, BAR, (tag, c, got, exact)))
    used = want["channels"]
    assert np.float32(rec.max_true_peak_db) == max([F32_FLOOR] + list(rec.true_peak_db[:used])), tag
    assert np.float32(rec.max_sample_peak_db) == max([F32_FLOOR] + list(rec.sample_peak_db[:used])), tag
    assert rec.max_true_peak_channel == want["max_true_peak_channel"], (tag, rec.max_true_peak_channel, want["max_true_peak_channel"])
    return worst


@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0, 176400.0, 192000.0, 384000.0])
def test_peaks_are_bit_exact_against_the_restatement(torch_dev, omx, coeffs, fs, ch):
    """seeded programmes of 2 s and 1.37 s, channel levels spread over 40 dB, each whole in one call"""
    xs = [ref.programme(seed, fs, ch, seconds) for seed, seconds in ((0, 2.0), (1, 1.37))]
    bank = feed(torch_dev, new_bank(omx, fs, len(xs), ch), xs, fs, ch, whole(xs))
    worst = 0.0
    for s, x in enumerate(xs):
        want = ref.restate(x, fs, coeffs, FLOOR)
        assert want["oversampling"] == (4 if fs < 96000 else 2 if fs < 192000 else 1) and want["channels"] == ch
        rec = bank.fetch_peaks(s)
        worst = max(worst, check_peaks(rec, want, (fs, ch, s)))
        assert bank.fetch(s).max_true_peak_db == rec.max_true_peak_db and bank.fetch(s).frames == rec.frames
    print(f"{fs} Hz {ch} ch: peaks and frames exact; dB fields vs f64: {worst:.2e} dB")


@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0, 176400.0])
def test_ebu_true_peak_tones_through_the_product(torch_dev, omx, coeffs, fs):
    """fs/4 at 0 / 45 degrees (the EBU Tech 3341 tones, +0.2 / -0.4 dB) and fs/6, fs/8 (held to the restatement only: the reference's
    interpolator reads them 0.3 .. 0.7 dB high) as five streams of one bank"""
    tones = [(4, 0.0, 0.5, -6.0), (4, 45.0, 0.5, -6.0), (4, 45.0, 1.41, 3.0), (6, 60.0, 0.5, None), (8, 67.5, 0.5, None)]
    xs = [ref.tone(fs, div, phase, amp, channels=2) for div, phase, amp, _ in tones]
    bank = feed(torch_dev, new_bank(omx, fs, len(xs), 2), xs, fs, 2, whole(xs))
    for s, (div, phase, amp, target) in enumerate(tones):
        rec = bank.fetch_peaks(s)
        check_peaks(rec, ref.restate(xs[s], fs, coeffs, FLOOR), (fs, div, phase, amp))
        print(f"{fs} Hz fs/{div} at {phase} deg x {amp}: {rec.max_true_peak_db:.3f} dBTP, sample peak {rec.max_sample_peak_db:.3f} dBFS")
        if target is not None:
            assert target - 0.4 <= rec.max_true_peak_db <= target + 0.2, (fs, div, phase, amp, rec.max_true_peak_db)


def small_then_random(rng, lengths, same_for_all):
    """calls of 0, 1, 5, 11, 12, 23 and 24 frames first, then random counts up to 3000 (per stream, or the same for every stream)"""
    left, out = list(lengths), []
    for n in (0, 1, 5, 11, 12, 23, 24, 0, 24, 1):
        counts = [min(n, m) for m in left]
        left = [m - c for m, c in zip(left, counts)]
        out.append(np.array(counts, np.uint32))
    while any(left):
        if same_for_all:
            n = int(rng.integers(1, 3000))
            counts = [min(n, m) for m in left]
        else:
            counts = [0 if rng.random() < 0.2 else int(min(rng.integers(1, 3000), m)) for m in left]
        left = [m - c for m, c in zip(left, counts)]
        out.append(np.array(counts, np.uint32))
    return out


@pytest.mark.parametrize("fs,ch", [(48000.0, 2), (44100.0, 6), (96000.0, 3), (192000.0, 2)])
def test_the_cut_does_not_matter(torch_dev, omx, coeffs, fs, ch):
    """one call, 256-frame calls, a ragged schedule with calls of 0, 1, 5, 11, 12, 23 and 24 frames, and streams on different cursors:
    the peak records are bitwise equal (and equal the restatement)"""
    xs = [ref.programme(seed, fs, ch, seconds) for seed, seconds in ((2, 0.9), (3, 0.61), (4, 0.75))]
    lengths = [len(x) for x in xs]
    rng = np.random.default_rng(9)
    schedules = {
        "one call": whole(xs),
        "256-frame calls": [np.array([min(256, max(n - t, 0)) for n in lengths], np.uint32) for t in range(0, max(lengths), 256)],
        "ragged, small calls": small_then_random(rng, lengths, True),
        "different cursors": small_then_random(rng, lengths, False),
    }
    got = {}
    for name, schedule in schedules.items():
        bank = feed(torch_dev, new_bank(omx, fs, len(xs), ch), xs, fs, ch, schedule)
        got[name] = [bank.fetch_peaks(s) for s in range(len(xs))]
    for s, x in enumerate(xs):
        check_peaks(got["one call"][s], ref.restate(x, fs, coeffs, FLOOR), (fs, ch, s))
        for name in schedules:
            assert got[name][s].tobytes() == got["one call"][s].tobytes(), (name, s, got[name][s], got["one call"][s])


@pytest.mark.parametrize("fs", [48000.0, 96000.0])
def test_bursts_at_tile_and_call_boundaries(torch_dev, omx, coeffs, fs):
    """64 streams of silence with a burst of three equal samples at k 2^m +- 12 (m = 5 .. 11: every run, tile and halo boundary of the
    peak pass), at frame 0 and at the last frame; as one call, and as two calls cut inside the burst: values and frames as restated"""
    frames = 12000
    chosen = ref.burst_positions(frames, 64)
    assert len(set(chosen)) == 64 and 0 in chosen and frames - 1 in chosen and all(p in chosen for p in (1012, 1036, 2036, 2060, 10228, 10252))
    xs = [ref.burst_programme(frames, p) for p in chosen]
    want = [ref.restate(x, fs, coeffs, FLOOR) for x in xs]
    above = sum(1 for w in want if w["true_peak"][0] > w["sample_peak"][0] and w["true_peak_frame"][0] > w["sample_peak_frame"][0])
    assert above >= 60, above        # the interpolated peak exceeds the sample peak and lands after the burst's first frame
    cut = np.array([min(p + 1, frames) for p in chosen], np.uint32)
    for name, schedule in (("one call", whole(xs)), ("cut inside the burst", [cut, np.uint32(frames) - cut])):
        bank = feed(torch_dev, new_bank(omx, fs, 64, 1), xs, fs, 1, schedule)
        for s in range(64):
            check_peaks(bank.fetch_peaks(s), want[s], (fs, name, chosen[s]))


@pytest.mark.parametrize("fs", [48000.0, 96000.0])
def test_against_the_existing_route_through_a_loudness_bank(torch_dev, omx, fs):
    """the same PCM through LoudnessBank.process_device (256-frame blocks) + note_snapshots on a bank with peaks off: its record's
    max_true_peak_db equals, bit for bit, the peaks-on bank's record and its peak record"""
    ch, S, blocks, pos = 2, 3, 24, capi.positions_fallback(2)
    xs = np.stack([ref.programme(seed, fs, ch, 256 * blocks * 2 / fs + 0.01)[:256 * blocks * 2] for seed in (5, 6, 7)])
    meter = banks.LoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch)
    off, on = new_bank(omx, fs, S, ch, peaks=False), new_bank(omx, fs, S, ch)
    for half in range(2):
        d = torch_dev.from_numpy(np.ascontiguousarray(xs[:, half * 256 * blocks:(half + 1) * 256 * blocks])).cuda()
        snaps = meter.process_device(d.data_ptr(), 256, blocks, ch, fs, pos)
        off.process(d.data_ptr(), 256 * blocks, ch, fs, pos)
        off.note_snapshots(snaps, blocks)
        on.process(d.data_ptr(), 256 * blocks, ch, fs, pos)
        torch_dev.cuda.synchronize()
    for s in range(S):
        a, b, c = off.fetch(s).max_true_peak_db, on.fetch(s).max_true_peak_db, on.fetch_peaks(s).max_true_peak_db
        print(f"{fs} Hz stream {s}: loudness bank + note_snapshots {a!r}, peaks on {b!r}, peak record {c!r}")
        assert a > FLOOR and np.float32(a).tobytes() == np.float32(b).tobytes() == np.float32(c).tobytes(), (s, a, b, c)


def test_off_by_default_and_set_peaks_only_on_an_empty_bank(torch_dev, omx, coeffs):
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    x = ref.programme(8, fs, ch, 0.5)
    d = torch_dev.from_numpy(np.stack([x, x])).cuda()
    bank = new_bank(omx, fs, 2, ch, peaks=False)
    bank.process(d.data_ptr(), len(x), ch, fs, pos)
    assert bank.fetch(0).max_true_peak_db == F32_FLOOR      # nothing measures it
    for call in (lambda: bank.fetch_peaks(0), lambda: bank.peaks(), lambda: bank.set_peaks(True)):      # off; and a stream holds samples
        with pytest.raises(capi.OmxError) as e:
            call()
        assert e.value.status == capi.ERR_INVALID
    bank.reset([1, 0])
    with pytest.raises(capi.OmxError):
        bank.set_peaks(True)                                  # stream 1 still holds samples
    bank.reset()
    bank.set_peaks(True)
    empty = bank.fetch_peaks(0)
    assert empty.frames == 0 and empty.oversampling == 0 and empty.channels == 0 and empty.max_true_peak_db == F32_FLOOR
    assert not empty.true_peak.any() and (empty.true_peak_db == F32_FLOOR).all()
    bank.process(d.data_ptr(), len(x), ch, fs, pos, frames=[len(x), 100])
    check_peaks(bank.fetch_peaks(0), ref.restate(x, fs, coeffs, FLOOR), "after set_peaks")
    check_peaks(bank.fetch_peaks(1), ref.restate(x[:100], fs, coeffs, FLOOR), "after set_peaks, 100 frames")
    assert bank.peaks() != 0
    with pytest.raises(capi.OmxError):
        bank.set_peaks(False)                                 # refused again: nothing changes
    assert bank.fetch_peaks(0).frames == len(x)
    with pytest.raises(capi.OmxError) as e:
        bank.fetch_peaks(2)
    assert e.value.status == capi.ERR_INVALID
    bank.reset()
    bank.set_peaks(False)
    with pytest.raises(capi.OmxError):
        bank.fetch_peaks(0)


def test_reset_of_one_stream_and_reset_mask_inside_a_call(torch_dev, omx, coeffs):
    fs, ch = 48000.0, 2
    xs = [ref.programme(seed, fs, ch, 0.6) for seed in (9, 10)]
    half = len(xs[0]) // 2 + 7
    # stream 1 is reset by the mask of the second call, before its samples are taken: its programme is its second part alone
    schedule = [np.array([half, half], np.uint32), np.array([len(xs[0]) - half] * 2, np.uint32)]
    bank = feed(torch_dev, new_bank(omx, fs, 2, ch), xs, fs, ch, schedule, resets=[None, [0, 1]])
    check_peaks(bank.fetch_peaks(0), ref.restate(xs[0], fs, coeffs, FLOOR), "not reset")
    check_peaks(bank.fetch_peaks(1), ref.restate(xs[1][half:], fs, coeffs, FLOOR), "reset by the call's mask")
    before = bank.fetch_peaks(1)
    bank.reset([1, 0])
    empty = bank.fetch_peaks(0)
    assert bank.fetch_peaks(1).tobytes() == before.tobytes()
    assert empty.frames == 0 and not empty.true_peak.any() and not empty.sample_peak_frame.any() and empty.max_true_peak_db == F32_FLOOR
    assert bank.fetch(0).max_true_peak_db == F32_FLOOR and bank.fetch(1).max_true_peak_db == before.max_true_peak_db
    # and it starts over like a new bank: no history from before the reset
    d = torch_dev.from_numpy(np.stack(xs)).cuda()
    bank.process(d.data_ptr(), len(xs[0]), ch, fs, capi.positions_fallback(ch), frames=[len(xs[0]), 0])
    check_peaks(bank.fetch_peaks(0), ref.restate(xs[0], fs, coeffs, FLOOR), "after reset()")
    assert bank.fetch_peaks(1).tobytes() == before.tobytes()


def test_overflow_nan_and_ties(torch_dev, omx, coeffs):
    fs, ch = 48000.0, 2
    # capacity 1 s = 10 segments = 48 000 frames: the peaks cover the stored part only (a louder sample behind it is never taken)
    x = ref.programme(11, fs, ch, 1.5)
    x[50000, 0] = 3.0
    bank = feed(torch_dev, new_bank(omx, fs, 1, ch, capacity_seconds=1), [x], fs, ch, [np.array([20000], np.uint32)] * 3 + [np.array([12000], np.uint32)])
    rec, loud = bank.fetch_peaks(0), bank.fetch(0)
    assert loud.overflow and loud.frames == 48000 and rec.frames == loud.frames
    check_peaks(rec, ref.restate(x[:48000], fs, coeffs, FLOOR), "overflow")
    # a NaN sample adds nothing for its own frame and the next 11; the rest is as restated (in one call and cut behind the NaN)
    y = ref.programme(12, fs, ch, 0.5)
    y[np.argmax(np.abs(y[:, 1])), 1] = np.nan           # the loudest sample of channel 1 itself
    y[5000, 0] = np.nan
    want = ref.restate(y, fs, coeffs, FLOOR)
    assert np.isfinite(want["true_peak"][:ch]).all() and want["true_peak"][1] > 0
    for schedule in (whole([y]), [np.array([5001], np.uint32), np.array([len(y) - 5001], np.uint32)]):
        check_peaks(feed(torch_dev, new_bank(omx, fs, 1, ch), [y], fs, ch, schedule).fetch_peaks(0), want, "NaN")
    z = y.copy()
    z[7000, 1] = np.inf
    rec = feed(torch_dev, new_bank(omx, fs, 1, ch), [z], fs, ch, whole([z])).fetch_peaks(0)
    check_peaks(rec, ref.restate(z, fs, coeffs, FLOOR), "inf")
    assert np.isinf(rec.true_peak[1]) and np.isinf(rec.max_true_peak_db) and rec.max_true_peak_channel == 1
    # ties between channels name the lowest channel
    t = ref.programme(13, fs, 1, 0.3)
    tie = np.concatenate([0.5 * t, t, t], axis=1)
    rec = feed(torch_dev, new_bank(omx, fs, 1, 3), [tie], fs, 3, whole([tie])).fetch_peaks(0)
    check_peaks(rec, ref.restate(tie, fs, coeffs, FLOOR), "tie")
    assert rec.max_true_peak_channel == 1 and rec.true_peak[1] == rec.true_peak[2]


LOUDNESS_LEVELS = ("integrated_lufs", "relative_threshold_lufs", "loudness_range_lu", "momentary_lufs", "short_term_lufs",
                   "max_momentary_lufs", "max_short_term_lufs")


@pytest.mark.parametrize("fs,S,ch,frames", [(48000.0, 1024, 8, 16384), (48000.0, 64, 2, 60 * 48000), (96000.0, 64, 2, 60 * 96000)])
def test_full_size(torch_dev, omx, oracle, coeffs, fs, S, ch, frames):
    """the shapes the bank was built for, one call each: max_true_peak_db of EVERY stream and the full record of 16 streams against the
    restatement; the loudness record of the same call equals, field for field, that of a bank with peaks off (max_true_peak_db
    aside), and holds its own bar against the loudness restatement on two streams"""
    torch = torch_dev
    pos = capi.positions_fallback(ch)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    levels = 10.0 ** (torch.empty((S, 1, ch), device="cuda").uniform_(-40.0, 0.0, generator=gen) / 20.0)
    pcm = torch.randn((S, frames, ch), device="cuda", generator=gen) * (0.2 * levels)
    on, off = new_bank(omx, fs, S, ch, capacity_seconds=90), new_bank(omx, fs, S, ch, peaks=False, capacity_seconds=90)
    for bank in (on, off):
        bank.process(pcm.data_ptr(), frames, ch, fs, pos, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full = sorted(set(int(s) for s in np.linspace(0, S - 1, 16).round()))
    assert len(full) == 16
    worst = 0.0
    host = pcm.cpu().numpy()
    with ThreadPoolExecutor(8) as pool:      # (numpy releases the interpreter lock inside its array loops)
        wants = list(pool.map(lambda s: ref.restate(host[s], fs, coeffs, FLOOR), range(S)))
    for s in range(S):
        x, want = host[s], wants[s]
        rec, loud = on.fetch_peaks(s), on.fetch(s)
        assert np.float32(rec.max_true_peak_db).tobytes() == np.float32(loud.max_true_peak_db).tobytes(), s
        d = abs(float(rec.max_true_peak_db) - max(ref.db_f64(p, FLOOR) for p in want["true_peak"][:ch]))
        worst = max(worst, bar("program peaks: |d max_true_peak_db| dB", d, BAR, (fs, S, s)))
        assert rec.true_peak.view(np.uint32).tolist() == want["true_peak"].view(np.uint32).tolist(), (s, rec.true_peak, want["true_peak"])
        if s in full:
            check_peaks(rec, want, (fs, S, ch, s))
        plain = off.fetch(s)
        assert plain.max_true_peak_db == F32_FLOOR
        for f in type(plain).ENERGY_FIELDS + type(plain).COUNT_FIELDS + LOUDNESS_LEVELS + ("overflow",):
            assert getattr(loud, f) == getattr(plain, f), (s, f, getattr(loud, f), getattr(plain, f))
        if s in full[:2]:
            lw = lref.restate(x, fs, pos, oracle.k_weighting_coefficients(lref.sanitize_rate(fs)))
            for f in LOUDNESS_LEVELS:
                bar(f"program loudness: |d {f}| LU", abs(float(getattr(loud, f)) - float(lw[f])), BAR, (fs, S, s, f))
            assert loud.segments == lw["segments"] and loud.frames == frames
    print(f"{S} x {ch} x {frames} at {fs} Hz: linear true peaks of every stream exact, max_true_peak_db vs f64 {worst:.2e} dB")


def test_c99_host_reads_the_ebu_tone(tmp_path, omx):
    """tests/c_abi/program_peaks_demo.c: fs/4 at 45 degrees, amplitude 0.5, from a plain C host in calls of 0.37 s"""
    from test_cpu_program_peaks import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    v = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)}
    for s in "01":
        assert abs(v["sample_peak" + s] + 9.03) <= 0.01 and -6.4 <= v["true_peak" + s] <= -5.8, v
    assert v["record_true_peak0"] == v["true_peak0"] and v["frames"] == 48000 and v["oversampling"] == 4 and v["channels"] == 2

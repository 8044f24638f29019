"""numpy restatement of the programme bank's peaks (include/omx/program_peaks.h): the checker of
ProgramLoudnessBank.set_peaks / fetch_peaks.  tests/test_cpu_program_peaks.py pins it to the oracle's sample-by-sample TruePeakMeter.

For channel c with samples x[0 .. N) since the last reset (x[n] = 0 for n < 0) and the sanitised rate fs (compared in f64):
  fs <  96000          : o_p[n] = sum_{i < 12} x[n - i] * fir4[i][p], p = 0, 1, 2
  96000 <= fs < 192000 : o_0[n] = sum_{i < 24} x[n - i] * fir2[i]
  fs >= 192000         : no interpolated outputs
every sum f32 in the order i = 0, 1, ..., every product rounded before it is added (numpy's f32 multiply and add are two roundings);
v[n] = fmax(|x[n]|, |o_p[n]| ...) (NaN operands ignored), true_peak = max v (from 0), sample_peak = max |x|, *_frame = the first n
that reaches the peak (0 for a peak of 0), dB = power_to_db(p * p, floor)."""
import numpy as np

from program_loudness_ref import sanitize_rate

MAX_CHANNELS = 8
LN_TO_DB = np.float32(4.3429448)   # level.rs:5


def coefficients(oracle):
    """(fir4 [12][3], fir2 [24]) f32 from the oracle's true_peak_coefficient (loudness/processor.rs:79-97)"""
    import ctypes as C
    f = oracle.fn("kat_true_peak_coefficient", C.c_float, [C.c_uint64, C.c_uint64])
    fir4 = np.array([[f(4 * t + p + 1, 4) for p in range(3)] for t in range(12)], np.float32)
    fir2 = np.array([f(2 * t + 1, 2) for t in range(24)], np.float32)
    return fir4, fir2


def oversampling(fs):
    fs = float(sanitize_rate(fs))
    return 4 if fs < 96000.0 else (2 if fs < 192000.0 else 1)


def interpolated(x, taps):
    """o[n] = sum_i x[n - i] * taps[i] in f32, i ascending, x[n] = 0 for n < 0.  x: f32 [N]; taps: f32 [DL]"""
    n = len(x)
    pad = np.concatenate([np.zeros(len(taps) - 1, np.float32), x])
    at = len(taps) - 1
    with np.errstate(all="ignore"):
        acc = pad[at:at + n] * taps[0]
        for i in range(1, len(taps)):
            acc = acc + pad[at - i:at - i + n] * taps[i]
    assert acc.dtype == np.float32
    return acc


def power_to_db_f32(power, floor):
    """level.rs:28-34 in f32 (numpy's f32 log stands in for logf: 1 ulp of the dB value)"""
    power = np.float32(power)
    if not power > 0:
        return np.float32(floor)
    with np.errstate(all="ignore"):
        return max(np.float32(np.log(power) * LN_TO_DB), np.float32(floor))


def db_f64(peak, floor):
    """20 log10(peak) in f64, floored: what the record's dB fields are held against (1e-4 dB)"""
    peak = float(peak)
    if not peak > 0.0:
        return float(np.float32(floor))
    return max(20.0 * np.log10(peak), float(np.float32(floor))) if np.isfinite(peak) else np.inf


def _first_max(v):
    """(max ignoring NaN, starting from 0; the first index that reaches it, 0 for a maximum of 0)"""
    if len(v) == 0:
        return np.float32(0.0), 0
    with np.errstate(all="ignore"):
        v = np.fmax(v, np.float32(0.0))      # (a NaN — every operand was one — adds nothing)
    peak = v.max()
    return np.float32(peak), (int(np.argmax(v == peak)) if peak > 0 else 0)


def channel_peaks(x, fs, coeffs):
    """x: f32 [N] -> (true_peak, true_peak_frame, sample_peak, sample_peak_frame)"""
    x = np.ascontiguousarray(x, np.float32)
    fir4, fir2 = coeffs
    with np.errstate(all="ignore"):
        v = np.abs(x)
        sample_peak, sample_frame = _first_max(v)
        factor = oversampling(fs)
        outs = [interpolated(x, fir4[:, p]) for p in range(3)] if factor == 4 else ([interpolated(x, fir2)] if factor == 2 else [])
        for o in outs:
            v = np.fmax(v, np.abs(o))
    true_peak, true_frame = _first_max(v)
    return true_peak, true_frame, sample_peak, sample_frame


def restate(x, fs, coeffs, floor=-99.9):
    """x: f32 [frames][channels] (the frames the bank took since the reset) -> the fields of omx_program_peak_record"""
    x = np.asarray(x, np.float32)
    frames, channels = x.shape
    floor = np.float32(floor)
    r = {"frames": frames, "channels": channels if frames else 0, "oversampling": oversampling(fs) if frames else 0,
         "true_peak": np.zeros(MAX_CHANNELS, np.float32), "sample_peak": np.zeros(MAX_CHANNELS, np.float32),
         "true_peak_frame": np.zeros(MAX_CHANNELS, np.uint64), "sample_peak_frame": np.zeros(MAX_CHANNELS, np.uint64),
         "true_peak_db": np.full(MAX_CHANNELS, floor), "sample_peak_db": np.full(MAX_CHANNELS, floor)}
    for c in range(channels if frames else 0):
        tp, tf, sp, sf = channel_peaks(x[:, c], fs, coeffs)
        r["true_peak"][c], r["true_peak_frame"][c], r["sample_peak"][c], r["sample_peak_frame"][c] = tp, tf, sp, sf
        with np.errstate(all="ignore"):
            r["true_peak_db"][c] = power_to_db_f32(tp * tp, floor)
            r["sample_peak_db"][c] = power_to_db_f32(sp * sp, floor)
    used = r["channels"]
    r["max_true_peak_db"] = np.float32(max([floor] + list(r["true_peak_db"][:used])))
    r["max_sample_peak_db"] = np.float32(max([floor] + list(r["sample_peak_db"][:used])))
    r["max_true_peak_channel"] = int(np.argmax(r["true_peak"][:used])) if used and r["true_peak"][:used].max() > 0 else 0
    return r


# ---- inputs of the tests
def programme(seed, fs, ch, seconds):
    """seeded programme [frames][ch] f32: band-limited-ish noise plus two sines per channel, channel levels spread over 40 dB, finite"""
    rng = np.random.default_rng(1000 + seed)
    n = int(round(float(fs) * seconds))
    t = np.arange(n, dtype=np.float64) / float(fs)
    levels = 10.0 ** (-np.linspace(0.0, 40.0, ch)[rng.permutation(ch)] / 20.0) if ch > 1 else np.array([0.5])
    x = np.empty((n, ch), np.float64)
    for c in range(ch):
        f1, f2 = rng.uniform(50.0, 0.45 * float(fs), 2)
        noise = rng.standard_normal(n)
        noise = 0.5 * (noise + np.roll(noise, 1))
        x[:, c] = levels[c] * (0.3 * noise + 0.35 * np.sin(2 * np.pi * f1 * t + rng.uniform(0, 6.28)) + 0.25 * np.sin(2 * np.pi * f2 * t))
    return x.astype(np.float32)


def tone(fs, divisor, phase_deg, amplitude, seconds=0.5, channels=1):
    """sine at fs / divisor starting at phase_deg (EBU Tech 3341 true-peak tones: fs/4 at 0 and 45 degrees ...)"""
    n = int(round(float(fs) * seconds))
    x = amplitude * np.sin(2.0 * np.pi * np.arange(n) / divisor + np.deg2rad(phase_deg))
    return np.repeat(x.astype(np.float32)[:, None], channels, axis=1)


def burst_programme(frames, position, length=3, amplitude=0.4):
    """silence with `length` equal-sign samples from `position` (clipped to the programme): the interpolated peak exceeds the sample
    peak and lands a few frames after the burst starts"""
    x = np.zeros((frames, 1), np.float32)
    x[max(position, 0):min(position + length, frames), 0] = amplitude
    return x


def burst_positions(frames, count=64):
    """`count` burst positions: frame 0, the last frame, and k * 2^m + d for m = 11 .. 5 (every run, tile and history boundary of the
    peak pass lies on such a grid), d = -12, +12, 0, -1 in that order of preference"""
    out = [0, frames - 1]
    for d in (-12, 12, 0, -1, 1, -11, 11):
        for m in range(11, 4, -1):
            for k in (1, 5, 3):
                p = k * 2 ** m + d
                if 0 < p < frames - 1 and p not in out:
                    out.append(p)
    assert len(out) >= count
    return out[:count]

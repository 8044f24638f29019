"""numpy restatement of the programme bank's long-term spectrum (include/omx/program_spectrum.h, DEFINITION and HOST ONLY).

The device half is restated in f64: np.fft.rfft of the f32 window times the f32 samples (the product rounded to f32, as the kernel
forms it), |.|^2, summed in the header's grouping (runs of RUN transforms, then the runs).  The host-only half runs the same f64
operations in the same order as the library, scalar transcendentals through `math` (the C library's), so it agrees with the library
to the last bits except through numpy's vector cos.  Pinned by tests/test_cpu_program_spectrum.py."""
import math

import numpy as np

RUN = 16
MAX_BANDS = 48
MAX_PROBES = 8
MAX_TAPS = 4095
DB_FLOOR = -400.0
BANDLIMITED, TONE = 1, 2
SIZES = (2048, 4096, 8192)
RECORD_DTYPE = np.dtype([("frames", "<u8"), ("transforms", "<u8", (8,)), ("skipped", "<u8", (8,)), ("fft_size", "<u4"),
                         ("channels", "<u4"), ("finished", "<u4"), ("_pad", "<u4")])


class Invalid(ValueError):
    pass


def window(n):
    """the periodic Hann in f64, rounded once"""
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n, dtype=np.float64) / float(n))).astype(np.float32)


def window_power(w):
    """W2: the sum of (double)w^2 in ascending n"""
    w64 = w.astype(np.float64)
    return float(np.cumsum(w64 * w64)[-1])


def transforms(frames, finished, n):
    h = n // 2
    if finished:
        return (frames + h - 1) // h
    return (frames - n) // h + 1 if frames >= n else 0


def transforms_brute(frames, finished, n):
    """by the grid's own words: transform k is taken once frame k H + N - 1 is held; a finish completes every k with k H < frames"""
    h, k = n // 2, 0
    while (k * h < frames) if finished else (k * h + n - 1 < frames):
        k += 1
    return k


def powers(x, n, finished, w=None):
    """x: f32 [frames][channels] -> (p f64 [transforms][channels][bins], kept bool [transforms][channels])"""
    x = np.asarray(x, np.float32)
    frames, ch = x.shape
    w = window(n) if w is None else np.asarray(w, np.float32)
    h, count = n // 2, transforms(frames, finished, n)
    padded = np.zeros((max(count - 1, 0) * h + n, ch), np.float32)
    padded[:min(frames, len(padded))] = x[:len(padded)]
    p = np.zeros((count, ch, h + 1), np.float64)
    kept = np.ones((count, ch), bool)
    for k in range(count):
        seg = padded[k * h:k * h + n]
        kept[k] = np.isfinite(seg).all(axis=0)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (seg * w[:, None]).astype(np.float32)      # the product in f32
        y = np.where(kept[k][None, :], y, np.float32(0))
        spec = np.fft.rfft(y.astype(np.float64), axis=0)
        p[k] = (spec.real ** 2 + spec.imag ** 2).T
    return p, kept


def grouped_sum(p, kept):
    """S of the header: the chain over each run's transforms, then the chain over the runs"""
    count, ch, bins = p.shape
    total = np.zeros((ch, bins), np.float64)
    for j in range(0, count, RUN):
        run = np.zeros((ch, bins), np.float64)
        for k in range(j, min(j + RUN, count)):
            run = run + np.where(kept[k][:, None], p[k], 0.0)
        total = total + run
    return total


def record(x, n, finished=False, w=None):
    """-> (record, sums f64 [channels][bins], scale f64 [channels]): scale is the sum over the kept transforms of the largest bin,
    what the f32 bar of a sum is taken from"""
    x = np.asarray(x, np.float32)
    frames, ch = x.shape
    p, kept = powers(x, n, finished, w)
    rec = np.zeros((), RECORD_DTYPE)
    rec["frames"], rec["fft_size"], rec["channels"], rec["finished"] = frames, n, ch, 1 if finished else 0
    rec["transforms"][:ch] = kept.sum(axis=0)
    rec["skipped"][:ch] = (~kept).sum(axis=0)
    scale = np.where(kept, p.max(axis=2), 0.0).sum(axis=0) if len(p) else np.zeros((ch,))
    return rec, grouped_sum(p, kept), scale


def windowed_mean_square(x, n, finished=False, w=None):
    """per channel: the mean over the kept transforms of sum((w x)^2) / W2, what the sum of the density equals by Parseval"""
    x = np.asarray(x, np.float32)
    frames, ch = x.shape
    w = window(n) if w is None else np.asarray(w, np.float32)
    h, count = n // 2, transforms(frames, finished, n)
    padded = np.zeros((max(count - 1, 0) * h + n, ch), np.float32)
    padded[:min(frames, len(padded))] = x[:len(padded)]
    total = np.zeros((ch,))
    for k in range(count):
        y = (padded[k * h:k * h + n] * w[:, None]).astype(np.float32).astype(np.float64)
        total += (y * y).sum(axis=0)
    return total / (max(count, 1) * window_power(w))


def size_ok(n):
    return n in SIZES


def rate_ok(fs):
    return math.isfinite(fs) and fs > 200.0


def density(rec, sums, channel, w=None):
    n, ch = int(rec["fft_size"]), int(rec["channels"])
    if not size_ok(n) or not 1 <= ch <= 8 or not 0 <= channel < ch:
        raise Invalid("record or channel")
    s = np.asarray(sums, np.float64).reshape(ch, n // 2 + 1)[channel]
    t = int(rec["transforms"][channel])
    if t == 0:
        return np.zeros_like(s)
    g = np.full(s.shape, 2.0)
    g[0] = g[-1] = 1.0
    return (g * s) / ((float(t) * float(n)) * window_power(window(n) if w is None else w))


def check_density(d, n):
    d = np.asarray(d, np.float64)
    if d.shape != (n // 2 + 1,) or not np.isfinite(d).all() or (d < 0).any():
        raise Invalid("density")
    return d


def db(v):
    return max(10.0 * math.log10(v), DB_FLOOR) if v > 0.0 else DB_FLOOR


def level(power):
    return db(2.0 * power)


def band_edges(fraction, n, fs):
    """[(centre, lo, hi)] of the listed bands"""
    df, nyq = fs / float(n), fs / 2.0
    down, up = math.pow(10.0, -0.15 / float(fraction)), math.pow(10.0, 0.15 / float(fraction))
    out = []
    for x in range(-40 * fraction, 20 * fraction + 1):
        centre = 1000.0 * math.pow(10.0, 0.3 * float(x) / float(fraction))
        lo, hi = centre * down, centre * up
        if lo >= 4.0 * df and hi <= nyq:
            out.append((centre, lo, hi))
    return out


def band_power(d, n, fs, lo, hi):
    df, nyq = fs / float(n), fs / 2.0
    b = np.arange(n // 2 + 1, dtype=np.float64)
    b_lo, b_hi = np.maximum(0.0, (b - 0.5) * df), np.minimum(nyq, (b + 0.5) * df)
    inside = np.minimum(hi, b_hi) - np.maximum(lo, b_lo)
    share = np.where(inside > 0.0, inside / (b_hi - b_lo), 0.0)
    return float(np.cumsum(d * share)[-1])


def bands(d, n, fs, fraction):
    if not size_ok(n) or not rate_ok(fs) or fraction not in (1, 3):
        raise Invalid("size, rate or fraction")
    d = check_density(d, n)
    edges = band_edges(fraction, n, fs)
    return (np.array([c for c, _, _ in edges]), np.array([level(band_power(d, n, fs, lo, hi)) for _, lo, hi in edges]))


class Qc:
    def __init__(self, occupied_fraction=0.9999, bandwidth_min_ratio=0.8, tone_db=20.0, probe_hz=(50.0, 100.0, 150.0, 60.0, 120.0, 180.0),
                 flags=0, n_probes=None):
        self.occupied_fraction, self.bandwidth_min_ratio, self.tone_db = occupied_fraction, bandwidth_min_ratio, tone_db
        self.probe_hz, self.flags = list(probe_hz), flags
        self.n_probes = len(self.probe_hz) if n_probes is None else n_probes

    def valid(self):
        return (self.flags == 0 and self.n_probes <= MAX_PROBES and 0.0 < self.occupied_fraction <= 1.0
                and 0.0 <= self.bandwidth_min_ratio <= 1.0 and math.isfinite(self.tone_db) and self.tone_db >= 0.0
                and all(math.isfinite(f) and f > 0.0 for f in self.probe_hz[:self.n_probes]))


def summarize(qc, d, n, fs):
    if not qc.valid() or not size_ok(n) or not rate_ok(fs):
        raise Invalid("qc, size or rate")
    d = check_density(d, n)
    half, df, nyq = n // 2, fs / float(n), fs / 2.0
    running = np.cumsum(d)
    total, pk = float(running[-1]), int(np.argmax(d))
    out = {"verdict": 0, "n_probes": qc.n_probes, "total_db": level(total), "occupied_hz": 0.0, "prominence_db": [0.0] * MAX_PROBES}
    delta = skew = 0.0
    if 0 < pk < half and d[pk - 1] > 0.0 and d[pk + 1] > 0.0:
        a, m, c = (10.0 * math.log10(float(d[i])) for i in (pk - 1, pk, pk + 1))
        q = a - 2.0 * m + c
        delta = 0.5 * (a - c) / q if q < 0.0 else 0.0
        delta = min(max(delta, -0.5), 0.5)
        skew = a - c
    out["peak_hz"] = (float(pk) + delta) * df
    out["peak_db"] = max(10.0 * math.log10(2.0 * float(d[pk])) - 0.25 * skew * delta, DB_FLOOR) if d[pk] > 0.0 else DB_FLOOR
    if total > 0.0:
        reached = np.nonzero(running >= qc.occupied_fraction * total)[0]
        at = int(reached[0]) if len(reached) else half
        out["occupied_hz"] = min((float(at) + 0.5) * df, nyq)
    third_down, third_up = math.pow(10.0, -0.1), math.pow(10.0, 0.1)
    fb = np.arange(half + 1, dtype=np.float64) * df
    for i, f in enumerate(qc.probe_hz[:qc.n_probes]):
        if not f < nyq:
            continue
        bc = int(math.floor(f / df + 0.5))
        strongest = max([float(d[b]) for b in range(bc - 1, bc + 2) if 0 <= b <= half], default=0.0)
        off = np.abs(np.arange(half + 1) - bc)
        near = np.sort(d[(off > 2) & (np.arange(half + 1) >= 1) & (((fb >= f * third_down) & (fb <= f * third_up)) | (off <= 6))])
        if not len(near):
            continue
        m = len(near)
        med = float(near[m // 2]) if m % 2 else 0.5 * (float(near[m // 2 - 1]) + float(near[m // 2]))
        out["prominence_db"][i] = db(strongest) - db(med)
        if out["prominence_db"][i] > qc.tone_db:
            out["verdict"] |= TONE
    if total > 0.0 and out["occupied_hz"] < qc.bandwidth_min_ratio * nyq:
        out["verdict"] |= BANDLIMITED
    return out


class MatchSpec:
    def __init__(self, max_boost_db=12.0, max_cut_db=12.0, low_hz=40.0, high_hz=0.45 * 48000.0, flags=0):
        self.max_boost_db, self.max_cut_db, self.low_hz, self.high_hz, self.flags = max_boost_db, max_cut_db, low_hz, high_hz, flags

    def valid(self, fs):
        return (self.flags == 0 and all(math.isfinite(v) for v in (self.max_boost_db, self.max_cut_db, self.low_hz, self.high_hz))
                and self.max_boost_db >= 0.0 and self.max_cut_db >= 0.0 and self.low_hz >= 0.0 and self.low_hz < self.high_hz <= fs / 2.0)


def smooth(d, half):
    prefix = np.concatenate([[0.0], np.cumsum(d)])
    c_lo, c_hi = math.pow(10.0, -0.05), math.pow(10.0, 0.05)
    b = np.arange(1, half + 1, dtype=np.float64)
    lo = np.maximum(1, np.ceil(b * c_lo).astype(np.int64))
    hi = np.minimum(half, np.floor(b * c_hi).astype(np.int64))
    return np.concatenate([[d[0]], (prefix[hi + 1] - prefix[lo]) / (hi - lo + 1).astype(np.float64)])


def match_gain_db(d_source, d_target, n, fs, spec):
    """the wanted gain per bin in dB, clamped and held"""
    half, df = n // 2, fs / float(n)
    b_lo, b_hi = max(1, int(math.ceil(spec.low_hz / df))), min(half, int(math.floor(spec.high_hz / df)))
    if b_lo > b_hi:
        raise Invalid("no bin between low_hz and high_hz")
    src, tgt = smooth(d_source, half), smooth(d_target, half)
    g = np.array([db(float(t)) - db(float(s)) for s, t in zip(src, tgt)])
    g = np.minimum(np.maximum(g, -spec.max_cut_db), spec.max_boost_db)
    g[:b_lo] = g[b_lo]
    g[b_hi + 1:] = g[b_hi]
    return g


def match(d_source, d_target, n, fs, spec, n_taps, rounded=True):
    if not size_ok(n) or not rate_ok(fs) or not spec.valid(fs):
        raise Invalid("size, rate or spec")
    if n_taps <= 0 or n_taps % 2 == 0 or n_taps > MAX_TAPS or n_taps >= n:
        raise Invalid("n_taps")
    d_source, d_target = check_density(d_source, n), check_density(d_target, n)
    half = n // 2
    amp = np.array([math.pow(10.0, float(g) / 20.0) for g in match_gain_db(d_source, d_target, n, fs, spec)])
    cosine = np.cos(2.0 * math.pi * np.arange(n, dtype=np.float64) / float(n))
    mid = (n_taps - 1) // 2
    b = np.arange(1, half, dtype=np.int64)
    taps = np.zeros((n_taps,), np.float64)
    for m in range(mid + 1):
        total = float(np.cumsum(amp[1:half] * cosine[(b * m) % n])[-1])
        h = (amp[0] + 2.0 * total + amp[half] * cosine[(half * m) % n]) / float(n)
        taps[mid + m] = taps[mid - m] = h * (0.5 + 0.5 * math.cos(math.pi * float(m) / float(mid + 1)))
    return taps.astype(np.float32) if rounded else taps


# ---------------------------------------------------------------- inputs
def noise(seed, frames, ch, level_=0.5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((frames, ch)) * level_ / 3.0).astype(np.float32)


def tilted_noise(seed, frames, tilt_db_per_octave, level_=0.25):
    """one channel of noise whose spectrum falls (or rises) by tilt dB per octave from 1 kHz at 48 kHz: f32 [frames][1]"""
    rng = np.random.default_rng(seed)
    spec = np.fft.rfft(rng.standard_normal(frames))
    f = np.maximum(np.fft.rfftfreq(frames, 1.0 / 48000.0), 20.0)
    shaped = np.fft.irfft(spec * 10.0 ** (tilt_db_per_octave * np.log2(f / 1000.0) / 20.0), frames)
    return (shaped / np.abs(shaped).max() * level_).astype(np.float32).reshape(-1, 1)


def third_octave_residual(d_got, d_target, n, fs, lo_hz=63.0, hi_hz=16000.0):
    """the largest |third-octave level of got - of target| over the bands whose centre lies in [lo_hz, hi_hz]"""
    c, got = bands(d_got, n, fs, 3)
    _, want = bands(d_target, n, fs, 3)
    keep = (c >= lo_hz * 0.99) & (c <= hi_hz * 1.01)
    return float(np.abs(got - want)[keep].max())


# ---------------------------------------------------------------- the match FIR's closed loop, in numpy alone
MATCH_N, MATCH_FS, MATCH_TAPS, MATCH_FRAMES = 8192, 48000.0, 2047, 200000


def match_inputs():
    """(source, target): a pink-ish noise (-3 dB per octave) and a brighter one (-1 dB per octave), f32 [MATCH_FRAMES][1]"""
    return tilted_noise(11, MATCH_FRAMES, -3.0), tilted_noise(12, MATCH_FRAMES, -1.0)


def measured_density(x, n, finished=True):
    rec, sums, _ = record(x, n, finished)
    return density(rec, sums, 0)


def filtered(x, taps):
    """x [frames][1] through a symmetric FIR, the output in place (what convolve gives with delay (T - 1) / 2 and a flush)"""
    y = np.convolve(x[:, 0].astype(np.float64), np.asarray(taps, np.float64), mode="same")
    return y.astype(np.float32).reshape(-1, 1)


_closed_loop = []


def closed_loop():
    """-> (residual dB, taps, source density, target density): the source through the FIR that `match` designs from the two measured
    densities, measured again, against the target in third octaves from 63 Hz to 16 kHz.  Computed once."""
    if not _closed_loop:
        src, tgt = match_inputs()
        d_src, d_tgt = measured_density(src, MATCH_N), measured_density(tgt, MATCH_N)
        taps = match(d_src, d_tgt, MATCH_N, MATCH_FS, MatchSpec(), MATCH_TAPS)
        d_out = measured_density(filtered(src, taps), MATCH_N)
        _closed_loop.append((third_octave_residual(d_out, d_tgt, MATCH_N, MATCH_FS), taps, d_src, d_tgt))
    return _closed_loop[0]

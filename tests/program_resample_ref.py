"""Numpy restatement of include/omx/program_resample.h: the plan, the tap table (f64, every step its own numpy operation, the I0 power
series with its fixed number of terms), the output frames (f32 products rounded before they are added to one of four f32 accumulators,
k mod 4, each in order of increasing k) and the streaming rule with its carry of T - 1 frames.  numpy float32 / float64 operations are
IEEE and none is fused.  tests/test_cpu_program_resample.py pins it, tests/test_gpu_program_resample.py holds the kernels to it (on the
library's own table: the two tables differ only where libm and numpy round a sine differently)."""
from math import gcd

import numpy as np

IDLE, RUNNING, FLUSHED = 0, 1, 2
DEFAULT_HALF_WIDTH, DEFAULT_BETA, DEFAULT_CUTOFF = 32, 12.0, 0.94
I0_TERMS = 64
MAX_FACTOR, MAX_HALF_WIDTH, MIN_RATE, MAX_RATE = 1024, 512, 3364, 768000
THREADS, STAGE_FRAMES = 256, 2048      # kRsThreads, kRsStageFrames: what sizes a plan's tile
RECORD_FIELDS = ("frames_in", "frames_out", "frames_written", "samples_over", "out_sample_peak", "out_sample_peak_db", "state", "L", "M",
                 "taps", "latency_frames")
EXACT_FIELDS = tuple(f for f in RECORD_FIELDS if f != "out_sample_peak_db")


class Invalid(ValueError):
    pass


class Unsupported(ValueError):
    pass


def plan(rate_in, rate_out, half_width=DEFAULT_HALF_WIDTH, beta=DEFAULT_BETA, cutoff=DEFAULT_CUTOFF, flags=0):
    """-> dict(L, M, T, H, tile, cutoff, beta); Invalid / Unsupported as the header says"""
    beta32, cutoff32 = np.float32(beta), np.float32(cutoff)
    if rate_in == 0 or rate_out == 0 or rate_in == rate_out:
        raise Invalid("rates")
    if half_width < 8 or half_width > 64 or half_width % 2:
        raise Invalid("half_width")
    if not np.isfinite(beta32) or beta32 < 0 or beta32 > 20:
        raise Invalid("beta")
    if not (cutoff32 > np.float32(0.5) and cutoff32 <= np.float32(1.0)):
        raise Invalid("cutoff")
    if flags != 0:
        raise Invalid("flags")
    if not (MIN_RATE <= rate_in <= MAX_RATE and MIN_RATE <= rate_out <= MAX_RATE):
        raise Unsupported("rate")
    g = gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    if L > MAX_FACTOR or M > MAX_FACTOR:
        raise Unsupported("factor")
    H = half_width if L >= M else 2 * (-(-(half_width * M) // (2 * L)))
    if H > MAX_HALF_WIDTH:
        raise Unsupported("half width")
    T = 2 * H
    tile = THREADS
    while tile > 1 and ((tile - 1) * M) // L + 1 + T > STAGE_FRAMES:
        tile -= 1
    return dict(L=L, M=M, T=T, H=H, tile=tile, cutoff=float(cutoff32), beta=float(beta32))


def i0(v):
    v = np.asarray(v, np.float64)
    y = v * 0.5
    t, s = np.ones_like(y), np.ones_like(y)
    for i in range(1, I0_TERMS + 1):
        t = t * (y / float(i))
        s = s + t * t
    return s


def taps(pl):
    """the [L][T] f32 table of a plan, computed as the header says"""
    L, M, T, H = pl["L"], pl["M"], pl["T"], pl["H"]
    fc = pl["cutoff"] * (float(L) / float(M) if L < M else 1.0)
    k = np.arange(T, dtype=np.int64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    d = (k - H + 1).astype(np.float64) - p / float(L)
    r = d / float(H)
    u = fc * d
    a = np.pi * u
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(u == 0.0, 1.0, np.sin(a) / a)
        inside = np.abs(d) < float(H)
        w = i0(pl["beta"] * np.sqrt(np.where(inside, 1.0 - r * r, 0.0)))
    h = np.where(inside, fc * sinc * w / i0(pl["beta"]), 0.0)
    total = np.zeros(L, np.float64)
    for j in range(T):      # in order of increasing k (np.sum adds pairwise)
        total = total + h[:, j]
    return (h / total[:, None]).astype(np.float32)


def emitted(pl, n, e, flush):
    """E' of a stream that has taken n frames and emitted e so far"""
    L, M, H = pl["L"], pl["M"], pl["H"]
    if flush:
        return -(-(n * L) // M)
    return max(e, -(-((n - H) * L) // M) if n > H else 0)


def frames_of(pl, m_lo, m_hi, window, window_first):
    """output frames [m_lo, m_hi) of a stream.  window: f32 [frames][channels], the stream's frames window_first .. (zeros where the
    definition has zeros); it must cover i0(m_lo) - H + 1 .. i0(m_hi - 1) + H."""
    L, M, T, H, table = pl["L"], pl["M"], pl["T"], pl["H"], pl["table"]
    channels = window.shape[1]
    if m_hi <= m_lo:
        return np.zeros((0, channels), np.float32)
    pos = np.arange(m_lo, m_hi, dtype=np.int64) * M
    i0_, p = pos // L, pos % L
    start = i0_ - H + 1 - window_first
    assert start.min() >= 0 and start.max() + T <= len(window), (start.min(), start.max() + T, len(window))
    acc = [np.zeros((len(pos), channels), np.float32) for _ in range(4)]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(T):
            prod = table[p, k][:, None] * window[start + k]      # f32 * f32 -> f32: the product is rounded
            acc[k % 4] = acc[k % 4] + prod
        out = (acc[0] + acc[1]) + (acc[2] + acc[3])
    assert out.dtype == np.float32
    return out


def resample(pl, x):
    """the whole programme in one piece, flushed: f32 [N][channels] -> f32 [ceil(N * L / M)][channels]"""
    x = np.asarray(x, np.float32)
    T, n_out = pl["T"], emitted(pl, len(x), 0, True)
    pad = np.zeros((T, x.shape[1]), np.float32)
    return frames_of(pl, 0, n_out, np.concatenate([pad, x, pad]), -T)


def power_to_db(power, floor):
    power = np.float32(power)
    return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


class Resampler:
    """one stream: the host's mirror (N, E, flushed), the carry of T - 1 frames and the record"""

    def __init__(self, pl, channels, floor=-99.9):
        self.pl, self.channels, self.floor = pl, channels, floor
        self.reset()

    def reset(self):
        self.n = self.e = self.written = self.over = 0
        self.flushed = False
        self.peak = np.float32(0)
        self.carry = np.zeros((self.pl["T"] - 1, self.channels), np.float32)      # frames n - (T - 1) .. n - 1, zeros in front of the stream

    def feed(self, x, flush=False):
        x = np.asarray(x, np.float32).reshape(-1, self.channels)
        assert not (self.flushed and len(x)), "frames for a flushed stream"
        pl, T = self.pl, self.pl["T"]
        flush = flush or self.flushed
        n_new = self.n + len(x)
        e_new = emitted(pl, n_new, self.e, flush)
        tail = np.zeros((T if flush else 0, self.channels), np.float32)
        out = frames_of(pl, self.e, e_new, np.concatenate([self.carry, x, tail]), self.n - (T - 1))
        self.carry = np.concatenate([self.carry, x])[-(T - 1):]
        self.n, self.e, self.written, self.flushed = n_new, e_new, len(out), flush
        m = np.abs(out)
        self.over += int((m > np.float32(1.0)).sum())
        if m.size and not np.isnan(m).all():
            self.peak = max(self.peak, np.float32(np.nanmax(m)))
        return out

    def record(self):
        pl = self.pl
        state = FLUSHED if self.flushed else (RUNNING if self.n else IDLE)
        return {"frames_in": self.n, "frames_out": self.e, "frames_written": self.written, "samples_over": self.over,
                "out_sample_peak": self.peak, "out_sample_peak_db": power_to_db(self.peak * self.peak, self.floor), "state": state,
                "L": pl["L"], "M": pl["M"], "taps": pl["T"], "latency_frames": pl["H"]}


def check_record(got, want, tag, bar=1e-4):
    for f in EXACT_FIELDS:
        if f == "out_sample_peak":
            assert np.float32(got[f]).tobytes() == np.float32(want[f]).tobytes(), (tag, f, got[f], want[f])
        else:
            assert int(got[f]) == int(want[f]), (tag, f, got[f], want[f])
    g, w = float(got["out_sample_peak_db"]), float(want["out_sample_peak_db"])
    assert g == w or abs(g - w) <= bar, (tag, g, w)      # (an infinite peak has an infinite level on both sides)


# ---------------------------------------------------------------- inputs of the tests
def noise(seed, frames, channels, amplitude=1.0):
    return (np.random.default_rng(seed).uniform(-amplitude, amplitude, (frames, channels))).astype(np.float32)


def hard(seed, frames, channels):
    """noise at +-1 with a NaN and an infinity of each sign a while apart, where the stream is long enough to hold them"""
    x = noise(seed, frames, channels)
    for at, v in ((frames // 3, np.nan), (frames // 2, np.inf), (frames // 2 + 300, -np.inf)):
        if 0 < at < frames:
            x[at, at % channels] = v
    return x


def tone(frames, fs, freq, amplitude=0.5, channels=1):
    t = np.arange(frames, dtype=np.float64)
    return np.repeat((amplitude * np.sin(2.0 * np.pi * freq * t / fs)).astype(np.float32)[:, None], channels, axis=1)


def fit_tone(y, fs, freq):
    """least-squares fit of a sine of `freq` to y (one channel, f64) -> (amplitude, rms of what is left)"""
    t = np.arange(len(y), dtype=np.float64)
    basis = np.stack([np.sin(2.0 * np.pi * freq * t / fs), np.cos(2.0 * np.pi * freq * t / fs)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, y, rcond=None)
    rest = y - basis @ coef
    return float(np.hypot(coef[0], coef[1])), float(np.sqrt(np.mean(rest * rest)))


def lengths_beside_a_tile(pl, tile, k=1, flush=True):
    """input lengths whose emission ends at k * tile - 1, k * tile and k * tile + 1 output frames"""
    out = []
    for want in (k * tile - 1, k * tile, k * tile + 1):
        n = next(n for n in range(0, (want + 2) * pl["M"] // pl["L"] + 2 * pl["T"] + 4) if emitted(pl, n, 0, flush) >= want)
        if emitted(pl, n, 0, flush) == want:
            out.append(n)
    return out

"""Numpy restatement of include/omx/program_convolve.h: the output frames (an f64 accumulator array that starts as h[0] * x[n] and
takes h[k] * x[n - k] for k = 1 .. T-1 in that order: each step one exact f64 product and one rounded f64 sum, then one rounding to
f32), the bypass copy, the streaming rule with its carry of max_taps - 1 frames, the record, and the design formulas (f64, every step
its own numpy operation, the resampler's I0 series).  numpy float64 operations are IEEE and none is fused.
tests/test_cpu_program_convolve.py pins it, tests/test_gpu_program_convolve.py holds the kernels to it (on the library's own taps:
the two designs differ only where libm and numpy round a sine differently)."""
import numpy as np

IDLE, RUNNING, FLUSHED = 0, 1, 2
LOWPASS, HIGHPASS, BANDPASS, BANDSTOP = range(4)
MAX_TAPS, MAX_FIRS, BYPASS = 4096, 64, 0xFFFFFFFF
I0_TERMS = 64
RECORD_FIELDS = ("frames_in", "frames_out", "frames_written", "samples_over", "samples_nonfinite", "out_sample_peak",
                 "out_sample_peak_db", "state", "delay_frames", "max_taps")
EXACT_FIELDS = tuple(f for f in RECORD_FIELDS if f != "out_sample_peak_db")


class Invalid(ValueError):
    pass


# ---------------------------------------------------------------- design
def i0(v):
    v = np.asarray(v, np.float64)
    y = v * 0.5
    t, s = np.ones_like(y), np.ones_like(y)
    for i in range(1, I0_TERMS + 1):
        t = t * (y / float(i))
        s = s + t * t
    return s


def lowpass64(fc, fs, beta, T):
    """lp(fc): f64 [T], unit DC gain, the half k <= M computed and mirrored"""
    M = (T - 1) // 2
    c = 2.0 * np.float64(fc) / np.float64(fs)
    k = np.arange(M + 1, dtype=np.float64)
    d = k - float(M)
    r = d / float(M)
    u = c * d
    a = np.pi * u
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(u == 0.0, 1.0, np.sin(a) / a)
    half = c * sinc * i0(np.float64(beta) * np.sqrt(1.0 - r * r)) / i0(np.float64(beta))
    w = np.concatenate([half, half[:M][::-1]])
    total = np.float64(0.0)
    for j in range(T):      # in order of increasing k (np.sum adds pairwise)
        total = total + w[j]
    return w / total


def design(kind, n_taps, fs, f_lo=0.0, f_hi=0.0, beta=9.0):
    """the f32 taps of a spec, as the header's DESIGN FORMULAS say; Invalid where the header refuses"""
    T = int(n_taps)
    if kind not in (LOWPASS, HIGHPASS, BANDPASS, BANDSTOP):
        raise Invalid("kind")
    if T < 3 or T > MAX_TAPS - 1 or T % 2 == 0:
        raise Invalid("n_taps")
    if not np.isfinite(fs) or not fs > 0:
        raise Invalid("rate")
    uses_lo, uses_hi = kind != LOWPASS, kind != HIGHPASS
    for used, f in ((uses_lo, f_lo), (uses_hi, f_hi)):
        if used and (not np.isfinite(f) or not f > 0 or not f < fs / 2.0):
            raise Invalid("frequency")
    if uses_lo and uses_hi and not f_lo < f_hi:
        raise Invalid("band")
    if not np.isfinite(beta) or beta < 0 or beta > 20:
        raise Invalid("beta")
    M = (T - 1) // 2
    delta = np.zeros(T, np.float64)
    delta[M] = 1.0
    hi = lowpass64(f_hi, fs, beta, T) if uses_hi else None
    lo = lowpass64(f_lo, fs, beta, T) if uses_lo else None
    h = {LOWPASS: lambda: hi, HIGHPASS: lambda: delta - lo, BANDPASS: lambda: hi - lo, BANDSTOP: lambda: delta - (hi - lo)}[kind]()
    half = h[:M + 1].astype(np.float32)
    return np.concatenate([half, half[:M][::-1]])


def response(taps, fs, hz):
    """(dB, radians) of sum h[k] e^{-jwk}, added in f64 in order of increasing k"""
    w = 2.0 * np.pi * hz / fs
    re = im = np.float64(0.0)
    for k, h in enumerate(np.asarray(taps, np.float32).astype(np.float64)):
        ph = w * float(k)
        re = re + h * np.cos(ph)
        im = im - h * np.sin(ph)
    with np.errstate(divide="ignore"):
        return float(20.0 * np.log10(np.sqrt(re * re + im * im))), float(np.arctan2(im, re))


# ---------------------------------------------------------------- the output frames
def emitted(delay, n, e, flush):
    """E' of a stream that has taken n frames and emitted e so far"""
    if flush:
        return n
    return max(e, n - delay if n > delay else 0)


def frames_of(taps, delay, m_lo, m_hi, window, window_first):
    """output frames [m_lo, m_hi) of ONE channel.  taps: f32 [T], or None for a bypassed channel.  window: f32 [frames], the channel's
    frames window_first .. (zeros where the definition has zeros); it must cover m_lo + delay - (T - 1) .. m_hi - 1 + delay (a bypass:
    m_lo .. m_hi - 1)."""
    count = m_hi - m_lo
    if count <= 0:
        return np.zeros((0,), np.float32)
    if taps is None:
        return window[m_lo - window_first:m_hi - window_first].copy()      # on bits
    h64 = np.asarray(taps, np.float32).astype(np.float64)
    x64 = window.astype(np.float64)
    at = m_lo + delay - window_first      # the window's index of x[n] for the first frame
    assert at - (len(h64) - 1) >= 0 and at + count <= len(window), (at, len(h64), count, len(window))
    with np.errstate(invalid="ignore", over="ignore"):
        acc = h64[0] * x64[at:at + count]
        for k in range(1, len(h64)):
            acc = acc + h64[k] * x64[at - k:at - k + count]      # one exact product, one rounded sum
        out = acc.astype(np.float32)      # round to nearest even, denormals produced
    return out


def convolve(firs, delay, x):
    """the whole programme in one piece, flushed: f32 [N][channels] -> f32 [N][channels].  firs: per channel f32 taps or None."""
    x = np.asarray(x, np.float32)
    st = Stream(firs, delay)
    return st.feed(x, flush=True)


def power_to_db(power, floor):
    power = np.float32(power)
    return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


class Stream:
    """one stream: the host's mirror (N, E, flushed), the carry of max_taps - 1 frames and the record.  firs: per channel f32 taps, or
    None for a bypassed channel; max_taps: the bank's (the longest FIR any stream references), this stream's longest by default."""

    def __init__(self, firs, delay, max_taps=None, floor=-99.9):
        self.firs = [None if t is None else np.asarray(t, np.float32).reshape(-1) for t in firs]
        self.channels, self.delay, self.floor = len(firs), int(delay), floor
        self.max_taps = int(max_taps) if max_taps is not None else max([len(t) for t in self.firs if t is not None] + [1])
        assert 0 <= self.delay <= self.max_taps - 1
        self.reset()

    def reset(self):
        self.n = self.e = self.written = self.over = self.nonfinite = 0
        self.flushed = False
        self.peak = np.float32(0)
        self.hist = self.max_taps - 1
        self.carry = np.zeros((self.hist, self.channels), np.float32)      # frames n - hist .. n - 1, zeros in front of the stream

    def feed(self, x, flush=False):
        x = np.asarray(x, np.float32).reshape(-1, self.channels)
        assert not (self.flushed and len(x)), "frames for a flushed stream"
        flush = flush or self.flushed
        n_new = self.n + len(x)
        e_new = emitted(self.delay, n_new, self.e, flush)
        tail = np.zeros((self.delay if flush else 0, self.channels), np.float32)
        window = np.concatenate([self.carry, x, tail])
        out = np.stack([frames_of(t, self.delay, self.e, e_new, window[:, c], self.n - self.hist) for c, t in enumerate(self.firs)], axis=1)
        self.carry = np.concatenate([self.carry, x])[len(x):]
        self.n, self.e, self.written, self.flushed = n_new, e_new, len(out), flush
        m = np.abs(out)
        self.over += int((m > np.float32(1.0)).sum())
        self.nonfinite += int((~np.isfinite(out)).sum())
        if m.size and not np.isnan(m).all():
            self.peak = max(self.peak, np.float32(np.nanmax(m)))
        return out

    def record(self):
        state = FLUSHED if self.flushed else (RUNNING if self.n else IDLE)
        with np.errstate(over="ignore"):
            power = self.peak * self.peak      # (f32: the square of a large peak is infinite, and so is its level)
        return {"frames_in": self.n, "frames_out": self.e, "frames_written": self.written, "samples_over": self.over,
                "samples_nonfinite": self.nonfinite, "out_sample_peak": self.peak,
                "out_sample_peak_db": power_to_db(power, self.floor), "state": state, "delay_frames": self.delay,
                "max_taps": self.max_taps}


def check_record(got, want, tag, bar=1e-4):
    for f in EXACT_FIELDS:
        if f == "out_sample_peak":
            assert np.float32(got[f]).tobytes() == np.float32(want[f]).tobytes(), (tag, f, got[f], want[f])
        else:
            assert int(got[f]) == int(want[f]), (tag, f, got[f], want[f])
    g, w = float(got["out_sample_peak_db"]), float(want["out_sample_peak_db"])
    assert g == w or abs(g - w) <= bar, (tag, g, w)      # (an infinite peak has an infinite level on both sides)


def same_floats(got, want, tag):
    """equal on bytes, with a NaN where the restatement has a NaN (the bits of a NaN the arithmetic produces are not defined)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (tag, "NaN positions", np.argwhere(np.isnan(got) != nan)[:4])
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (tag, bad.size, bad[:4], got[~nan][bad[:4]], want[~nan][bad[:4]])


# ---------------------------------------------------------------- inputs of the tests
def noise(seed, frames, channels, amplitude=1.0):
    return (np.random.default_rng(seed).uniform(-amplitude, amplitude, (frames, channels))).astype(np.float32)


def random_taps(seed, n, zeros=True):
    """finite taps of mixed sizes, a few of them zero"""
    rng = np.random.default_rng(seed)
    h = (rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-12, 2, n))).astype(np.float32)
    if zeros and n > 2:
        h[rng.integers(0, n, max(1, n // 16))] = 0.0
    return h


def cuts_of(n, pieces):
    """`pieces` cut lengths that sum to n"""
    return [len(p) for p in np.array_split(np.arange(n), pieces)]

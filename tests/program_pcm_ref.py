"""Numpy restatement of include/omx/program_pcm.h: integer PCM to f32 (import) and f32 to integer PCM with TPDF dither (export), sample
by sample as the header defines them.  Every step of the export is f64 (numpy float64 operations are IEEE, none is fused); the hash is
uint64 arithmetic that wraps.  tests/test_cpu_program_pcm.py pins it, tests/test_gpu_program_pcm.py holds the kernels to it."""
import numpy as np

S16, S24, S32 = 1, 2, 3
NONE, TPDF = 0, 1
BYTES = {S16: 2, S24: 3, S32: 4}
BITS = {S16: 16, S24: 24, S32: 32}
RECORD_FIELDS = ("frames_out", "frames_written", "samples_clipped", "samples_nan", "out_peak", "out_peak_db", "format", "dither")
EXACT_FIELDS = tuple(f for f in RECORD_FIELDS if f != "out_peak_db")
TILE_SAMPLES = 4096      # kPcTileSamples: both passes move a row in tiles of this many samples

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def rule_valid(rule):
    fmt, dither, _seed, *flags = rule
    return fmt in BYTES and dither in (NONE, TPDF) and (not flags or flags[0] == 0)


def mix(z):
    z = np.asarray(z, np.uint64).copy().reshape(-1)
    z ^= z >> np.uint64(30)
    z *= M1
    z ^= z >> np.uint64(27)
    z *= M2
    z ^= z >> np.uint64(31)
    return z


def u64(v):
    return np.array([int(v) % 2 ** 64], np.uint64)


def stream_key(seed, stream):
    return mix(u64(seed) + GOLDEN * u64(stream + 1))


def dither(seed, stream, frames, channel):
    """d, in LSB, for the absolute frames `frames` (array of ints) of (seed, stream, channel)"""
    n = np.array([int(f) % 2 ** 64 for f in np.asarray(frames, object).reshape(-1)], np.uint64)
    h = mix(stream_key(seed, stream) + GOLDEN * (n * np.uint64(8) + np.uint64(channel)))
    a = (h & np.uint64(0xFFFFFF)).astype(np.int64)
    b = ((h >> np.uint64(24)) & np.uint64(0xFFFFFF)).astype(np.int64)
    return (a - b).astype(np.float64) * 2.0 ** -24


# ---------------------------------------------------------------- import
def unpack(raw, fmt):
    """bytes -> the integer samples as int64"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    if fmt == S16:
        return raw.view("<i2").astype(np.int64)
    if fmt == S32:
        return raw.view("<i4").astype(np.int64)
    b = raw.reshape(-1, 3).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v >= 2 ** 23, v - 2 ** 24, v)


def pack(y, fmt):
    """integer samples -> bytes"""
    y = np.asarray(y, np.int64).reshape(-1)
    if fmt == S16:
        return y.astype("<i2").tobytes()
    if fmt == S32:
        return y.astype("<i4").tobytes()
    u = (y & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def import_pcm(raw, fmt, channels):
    """bytes of one row -> f32 [frames][channels]"""
    v = unpack(raw, fmt)
    x = v.astype(np.float32) * np.float32(2.0 ** -(BITS[fmt] - 1))      # int -> f32 rounds to nearest even, the scale is exact
    return x.reshape(-1, channels)


# ---------------------------------------------------------------- export
def power_to_db(power, floor):
    power = np.float32(power)
    return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


def peak_db(out_peak, fmt, floor):
    p = np.float32(float(out_peak) / 2.0 ** (BITS[fmt] - 1))
    return power_to_db(p * p, floor)


def quantise(x, d, fmt):
    """x f32, d f64 (same shape) -> (y int64, clipped bool, nan bool, sv f64)"""
    x = np.asarray(x, np.float32)
    full = 2.0 ** (BITS[fmt] - 1)
    nan = np.isnan(x)
    sv = np.where(nan, np.float32(0), x).astype(np.float64) * full
    with np.errstate(invalid="ignore"):
        t = sv + d
        r = np.floor(t + 0.5)
        clipped = ((r < -full) | (r > full - 1.0)) & ~nan
        y = np.clip(r, -full, full - 1.0)
    y = np.where(nan, 0.0, y).astype(np.int64)
    return y, clipped, nan, sv


def dither_block(rule, stream, first_frame, frames, channels):
    """d [frames][channels] for the absolute frames first_frame .. first_frame + frames - 1"""
    fmt, dith, seed = rule[:3]
    if dith == NONE or frames == 0:
        return np.zeros((frames, channels), np.float64)
    n = np.arange(frames, dtype=np.uint64) + np.uint64(first_frame)
    return np.stack([dither(seed, stream, n, c) for c in range(channels)], axis=1)


def export_pcm(x, rule, stream, first_frame):
    """x f32 [frames][channels], the stream's frames first_frame .. -> (bytes, {samples_clipped, samples_nan, out_peak})"""
    x = np.asarray(x, np.float32)
    frames, channels = x.shape
    y, clipped, nan, _ = quantise(x, dither_block(rule, stream, first_frame, frames, channels), rule[0])
    counts = {"samples_clipped": int(clipped.sum()), "samples_nan": int(nan.sum()), "out_peak": int(np.abs(y).max()) if y.size else 0}
    return pack(y, rule[0]), counts


class Exporter:
    """one stream of the export with its carried position and record"""

    def __init__(self, rule, stream, floor=-99.9):
        self.rule, self.stream, self.floor = rule, stream, floor
        self.reset()

    def reset(self):
        self.pos, self.written, self.clipped, self.nans, self.peak = 0, 0, 0, 0, 0

    def feed(self, x):
        raw, c = export_pcm(x, self.rule, self.stream, self.pos)
        self.pos += len(x)
        self.written = len(x)
        self.clipped += c["samples_clipped"]
        self.nans += c["samples_nan"]
        self.peak = max(self.peak, c["out_peak"])
        return raw

    def record(self):
        return {"frames_out": self.pos, "frames_written": self.written, "samples_clipped": self.clipped, "samples_nan": self.nans,
                "out_peak": self.peak, "out_peak_db": peak_db(self.peak, self.rule[0], self.floor), "format": self.rule[0],
                "dither": self.rule[1]}


def check_record(got, want, tag, bar=1e-4):
    for f in EXACT_FIELDS:
        assert int(got[f]) == int(want[f]), (tag, f, got[f], want[f])
    assert abs(float(got["out_peak_db"]) - float(want["out_peak_db"])) <= bar, (tag, got["out_peak_db"], want["out_peak_db"])


# ---------------------------------------------------------------- inputs of the GPU tests
def noise(seed, frames, channels, amplitude=1.2):
    return (np.random.default_rng(seed).uniform(-amplitude, amplitude, (frames, channels))).astype(np.float32)


def low_sine(frames, channels, fmt, amplitude_lsb=0.4, fs=48000.0):
    t = np.arange(frames, dtype=np.float64)
    x = amplitude_lsb * np.sin(2.0 * np.pi * 997.0 * t / fs) / 2.0 ** (BITS[fmt] - 1)
    return np.repeat(x.astype(np.float32)[:, None], channels, axis=1)


def hard(seed, frames, channels, fmt):
    """NaN (both signs, a payload), infinities, denormals, +-1.0, exact halves k + 0.5 and the last values in range, in noise"""
    x = noise(seed, frames, channels, 0.5)
    flat = x.reshape(-1)
    if flat.size == 0:
        return x
    full = 2.0 ** (BITS[fmt] - 1)
    halves = [(k + 0.5) / full for k in (-3, -2, -1, 0, 1, 2, 100, -101)] if fmt != S32 else [0.5, -0.5]      # (k + 0.5 is no f32 at 32 bits)
    specials = [np.nan, -np.nan, np.inf, -np.inf, 1e-40, -3e-42, -0.0, 1.0, -1.0, (full - 1) / full, (full - 0.5) / full,
                -(full + 0.5) / full] + halves
    special = np.array(specials, np.float32)
    special = np.concatenate([special, np.array([0x7FC12345, 0xFF800001], np.uint32).view(np.float32)])
    at = np.random.default_rng(seed + 1).choice(flat.size, size=min(len(special) * 3, flat.size), replace=False)
    flat[at] = np.resize(special, at.size)
    return x


def export_case_streams(seed, lengths, channels, fmt, first_kind=0):
    """per stream one of: noise at +-1.2 full scale, the hard values, a low-level sine, zeros -- in that order from `first_kind` on,
    repeated"""
    makers = [lambda s, f: noise(s, f, channels), lambda s, f: hard(s, f, channels, fmt), lambda s, f: low_sine(f, channels, fmt),
              lambda s, f: np.zeros((f, channels), np.float32)]
    return [makers[(k + first_kind) % 4](seed + k, f) for k, f in enumerate(lengths)]


def random_pcm(seed, frames, channels, fmt):
    """random bytes plus the extremes; S32: values that round on their way to f32"""
    rng = np.random.default_rng(seed)
    raw = bytearray(rng.integers(0, 256, frames * channels * BYTES[fmt], dtype=np.uint8).tobytes())
    lo, hi = -2 ** (BITS[fmt] - 1), 2 ** (BITS[fmt] - 1) - 1
    specials = [lo, hi, 0, -1, 1, lo + 1, hi - 1]
    if fmt == S32:
        specials += [2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 25 + 2, 2 ** 25 + 6, hi - 63, hi - 64, hi - 65]
    n = frames * channels
    for k, v in enumerate(specials):
        if k < n:
            at = int(rng.integers(0, n)) if n > len(specials) else k
            raw[at * BYTES[fmt]:(at + 1) * BYTES[fmt]] = pack([v], fmt)
    return bytes(raw)


def tile_frames(channels):
    """frame counts one frame either side of a tile of a row that starts 16-byte aligned, and either side of the longest head"""
    t = TILE_SAMPLES // channels
    return sorted({max(t - 1, 0), t, t + 1, t + 2})

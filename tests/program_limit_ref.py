"""numpy restatement of the programme bank's limiter (include/omx/program_limit.h, DESIGN.md section 10 "Limiter"): the checker of
ProgramLoudnessBank.apply_limited.  It reads nothing from the library.  Also the rules, inputs and shapes shared by
tests/test_cpu_program_limit.py and tests/test_gpu_program_limit.py.

For one stream with samples x[n][c], n = 0 .. N-1, gain factor g and ceiling c = f32(10 ** (f64(ceiling_db) / 20)):
  v[n]  = fmax over the channels of program_peaks_ref's v[n] (|x[n]| and the interpolated outputs of the rate's band)
  u[n]  = v[n] * |g|                                  one f32 multiply
  q[n]  = u[n] > c ? floor(f64(c) / f64(u[n]) * 2^24) : 2^24;  2^24 for n < 0 and, once flushed, for n >= N
  w[n]  = min q[n-W+1 .. n],  W = A + 24 + R
  S[n]  = sum w[n-A+1 .. n]                           integers
  Gf[j] = f32(f64(S[j + LA]) / f64(A << 24)),  LA = A + 23
  out[j][c] = x[j][c] * (g * Gf[j])                   two f32 multiplies
`Limiter` is the streaming form with carried state (the interpolator history, the newest W + A - 2 values of q, the frames taken but
not yet emitted); `direct` evaluates the definition frame by frame in O(N W)."""
import numpy as np

import program_peaks_ref as pk

UNITY_Q = 1 << 24
UNITY_GAIN = 2 ** 32 - 1
HISTORY = 23
IDLE, RUNNING, FLUSHED = 0, 1, 2
RECORD_FIELDS = ("frames_in", "frames_out", "frames_written", "frames_limited", "samples_over", "gain", "ceiling", "min_envelope",
                 "out_sample_peak", "out_sample_peak_db", "max_reduction_db", "gain_index", "state", "latency_frames", "_pad")
EXACT_FIELDS = ("frames_in", "frames_out", "frames_written", "frames_limited", "samples_over", "gain", "ceiling", "min_envelope",
                "out_sample_peak", "gain_index", "state", "latency_frames")


def latency(rule):
    return int(rule[1]) + HISTORY


def window(rule):
    return int(rule[1]) + 24 + int(rule[2])


def ceiling(rule):
    """rule: (ceiling_db, attack_frames, release_hold_frames)"""
    return np.float32(np.power(np.float64(10.0), np.float64(np.float32(rule[0])) / np.float64(20.0)))


def rule_valid(rule):
    db, A, R = rule[:3]
    flags = rule[3] if len(rule) > 3 else 0
    return bool(np.isfinite(np.float32(db)) and -120.0 <= np.float32(db) <= 20.0 and 1 <= A <= 4096 and 0 <= R <= 16384 and flags == 0)


def level(x, history, fs, coeffs):
    """v[n] of the frames x [F][C] that follow `history` [<= 23][C] (zeros before it)"""
    x = np.asarray(x, np.float32)
    both = np.concatenate([np.asarray(history, np.float32).reshape(-1, x.shape[1]), x])
    fir4, fir2 = coeffs
    factor = pk.oversampling(fs)
    v = np.full(len(both), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for c in range(x.shape[1]):
            col = np.ascontiguousarray(both[:, c])
            vc = np.abs(col)
            outs = [pk.interpolated(col, fir4[:, p]) for p in range(3)] if factor == 4 else ([pk.interpolated(col, fir2)] if factor == 2 else [])
            for o in outs:
                vc = np.fmax(vc, np.abs(o))
            v = np.fmax(v, vc)
    assert v.dtype == np.float32
    return v[len(both) - len(x):]


def required(v, g, c):
    """q[n] as uint32"""
    with np.errstate(all="ignore"):
        u = (np.asarray(v, np.float32) * np.abs(np.float32(g))).astype(np.float32)
        over = u > np.float32(c)
        ratio = np.float64(np.float32(c)) / u.astype(np.float64) * np.float64(16777216.0)
        q = np.where(over, np.floor(np.where(over, ratio, 0.0)), float(UNITY_Q))
    return q.astype(np.uint32)


def sliding_min(q, W):
    """min q[i-W+1 .. i] for i >= W - 1 (len(q) - W + 1 values), by doubling"""
    q = np.asarray(q, np.uint32)
    if len(q) < W:
        return np.zeros(0, np.uint32)
    m, win = q.copy(), 1                       # m[i] = min of the `win` values that end at i
    while 2 * win <= W:
        m[win:] = np.minimum(m[win:], m[:-win])
        win *= 2
    out = m[W - 1:].copy()
    if W > win:
        out = np.minimum(out, m[win - 1:len(m) - (W - win)])
    return out


def boxcar(w, A):
    """sum w[i-A+1 .. i] for i >= A - 1, exact in u64"""
    w = np.asarray(w, np.uint64)
    if len(w) < A:
        return np.zeros(0, np.uint64)
    p = np.concatenate([[np.uint64(0)], np.cumsum(w, dtype=np.uint64)])
    return p[A:] - p[:-A]


def envelope(S, A):
    return (np.asarray(S, np.uint64).astype(np.float64) / np.float64(A << 24)).astype(np.float32)


def power_to_db(p, floor):
    with np.errstate(all="ignore"):
        return float(pk.power_to_db_f32(np.float32(p) * np.float32(p), floor))


class Limiter:
    """one stream of the limiter, fed in pieces"""

    def __init__(self, rule, fs, coeffs, channels, floor=-99.9):
        assert rule_valid(rule)
        self.rule, self.fs, self.coeffs, self.channels, self.floor = rule, fs, coeffs, channels, np.float32(floor)
        self.A, self.R, self.W, self.LA = int(rule[1]), int(rule[2]), window(rule), latency(rule)
        self.c = ceiling(rule)
        self.reset()

    def reset(self):
        self.N = self.E = 0
        self.flushed = False
        self.g, self.gain_index = np.float32(1.0), UNITY_GAIN
        self.history = np.zeros((0, self.channels), np.float32)
        self.pending = np.zeros((0, self.channels), np.float32)          # frames E .. N-1
        self.q = np.full(self.W + self.A - 2, UNITY_Q, np.uint32)          # q[N - (W + A - 2) .. N)
        self.frames_limited = self.samples_over = self.frames_written = 0
        self.min_envelope, self.out_sample_peak = np.float32(1.0), np.float32(0.0)

    def feed(self, x, flush=False, gain=1.0, gain_index=UNITY_GAIN):
        """-> (out [frames emitted][C], Gf of those frames).  gain / gain_index are read only when the first frame arrives"""
        x = np.asarray(x, np.float32).reshape(-1, self.channels)
        assert not (self.flushed and len(x)), "frames for a flushed stream"
        if self.N == 0 and len(x):
            self.g, self.gain_index = np.float32(gain), gain_index
        flush = flush or self.flushed
        q_all = np.concatenate([self.q, required(level(x, self.history, self.fs, self.coeffs), self.g, self.c)])   # q[N_old - Hq .. N_new)
        n_old, n_new = self.N, self.N + len(x)
        if flush:
            q_all = np.concatenate([q_all, np.full(self.LA, UNITY_Q, np.uint32)])
        S = boxcar(sliding_min(q_all, self.W), self.A)                      # S[n_old ..]: one per value of q behind the history
        e_new = n_new if flush else max(self.E, n_new - self.LA)
        gf = envelope(S[self.E + self.LA - n_old:e_new + self.LA - n_old], self.A)
        have = np.concatenate([self.pending, x])
        with np.errstate(all="ignore"):
            k = (self.g * gf).astype(np.float32)
            out = (have[:e_new - self.E] * k[:, None]).astype(np.float32)
            mag = np.abs(out)
            self.samples_over += int(np.count_nonzero(mag > np.float32(1.0)))
            seen = mag[~np.isnan(mag)]
        if seen.size:
            self.out_sample_peak = max(self.out_sample_peak, np.float32(seen.max()))
        if gf.size:
            self.frames_limited += int(np.count_nonzero(gf < np.float32(1.0)))
            self.min_envelope = min(self.min_envelope, np.float32(gf.min()))
        self.frames_written = e_new - self.E
        self.pending = have[e_new - self.E:]
        self.history = np.concatenate([self.history, x])[-HISTORY:]
        self.q = q_all[:len(self.q) + len(x)][-len(self.q):]
        self.N, self.E, self.flushed = n_new, e_new, flush
        return out, gf

    def record(self):
        return {"frames_in": self.N, "frames_out": self.E, "frames_written": self.frames_written, "frames_limited": self.frames_limited,
                "samples_over": self.samples_over, "gain": self.g, "ceiling": self.c, "min_envelope": self.min_envelope,
                "out_sample_peak": self.out_sample_peak, "out_sample_peak_db": power_to_db(self.out_sample_peak, self.floor),
                "max_reduction_db": -power_to_db(self.min_envelope, self.floor), "gain_index": self.gain_index,
                "state": FLUSHED if self.flushed else (RUNNING if self.N else IDLE), "latency_frames": self.LA}


def restate(x, fs, coeffs, g, rule, floor=-99.9):
    """the whole programme in one flushed call -> (out, Gf, record)"""
    x = np.asarray(x, np.float32)
    lim = Limiter(rule, fs, coeffs, x.shape[1], floor)
    out, gf = lim.feed(x, flush=True, gain=g, gain_index=0)
    return out, gf, lim.record()


def direct(x, fs, coeffs, g, rule):
    """the definition frame by frame, O(N W): (out, Gf) of the flushed programme"""
    x = np.asarray(x, np.float32)
    N, A, W, LA = len(x), int(rule[1]), window(rule), latency(rule)
    q = [int(v) for v in required(level(x, np.zeros((0, x.shape[1]), np.float32), fs, coeffs), g, ceiling(rule))]
    at = lambda n: q[n] if 0 <= n < N else UNITY_Q
    w = {n: min(at(t) for t in range(n - W + 1, n + 1)) for n in range(LA - A + 1, N + LA)}
    gf = np.zeros(N, np.float32)
    for j in range(N):
        S = sum(w[n] for n in range(j + LA - A + 1, j + LA + 1))
        gf[j] = np.float32(np.float64(S) / np.float64(A << 24))
    with np.errstate(all="ignore"):
        k = (np.float32(g) * gf).astype(np.float32)
        return (x * k[:, None]).astype(np.float32), gf


def check_record(got, want, tag):
    """got: a LIMIT_RECORD_DTYPE scalar, want: Limiter.record().  Integers and linear floats equal bits; the dB fields within 1e-4 dB"""
    for f in EXACT_FIELDS:
        w = np.float32(want[f]) if got[f].dtype == np.float32 else got[f].dtype.type(want[f])
        assert got[f].tobytes() == w.tobytes(), (tag, f, got[f], want[f])
    for f in ("out_sample_peak_db", "max_reduction_db"):
        if np.isinf(want[f]):
            assert got[f] == want[f], (tag, f, got[f], want[f])
        else:
            assert abs(float(got[f]) - float(want[f])) <= 1e-4, (tag, f, got[f], want[f])


# ---------------------------------------------------------------- rules, inputs and shapes shared by the CPU and the GPU file
CEILING_DB = -1.0
ATTACKS, HOLDS = (1, 16, 240), (0, 100)
RATES = (48000.0, 96000.0, 192000.0)           # 4x, 2x, no interpolation
CHANNELS = (1, 2, 3, 8)
# the tile lengths of the four passes, in frames (program_limit.hpp: kLmLevelTile, kLmHoldTile, kLmSmoothTile) and in floats
# (kLmApplyTileFloats); stream lengths straddle each by one
LEVEL_TILE, HOLD_TILE, SMOOTH_TILE, APPLY_TILE_FLOATS = 1024, 2048, 2048, 4096
LONGEST = 6000
GAIN = 2.0                                       # +6 dB on inputs that reach 0.9: 6 dB over a ceiling of -1 dBTP


def noise(seed, frames, channels, scale=0.9):
    return np.random.default_rng([seed, 11]).uniform(-scale, scale, (frames, channels)).astype(np.float32)


def gated_tone(seed, frames, channels, fs, amplitude=0.9):
    """a sine near fs / 4.37 at `amplitude`, switched on and off every few hundred frames (the same gate on every channel, another
    phase per channel): attacks and releases of the envelope in the open, silence between them"""
    rng = np.random.default_rng([seed, 12])
    n = np.arange(frames, dtype=np.float64)
    gate = ((n // 300) % 2 == 0).astype(np.float64)
    phases = rng.uniform(0.0, 2 * np.pi, channels)
    return (amplitude * gate[:, None] * np.sin(2 * np.pi * n[:, None] / 4.37 + phases[None, :])).astype(np.float32)


def planted(x, seed):
    """a copy with one NaN, one +inf and one -inf at seeded places"""
    x = np.array(x, np.float32)
    flat = x.reshape(-1)
    at = np.random.default_rng([seed, 13]).choice(flat.size, 3, replace=False)
    flat[at] = np.array([np.nan, np.inf, -np.inf], np.float32)
    return x


def case_lengths(channels):
    """five lengths of at most LONGEST frames: one beside a tile end of every pass"""
    apply_frames = APPLY_TILE_FLOATS // channels
    return [LONGEST, HOLD_TILE + 1, apply_frames - 1 if apply_frames - 1 not in (HOLD_TILE + 1, SMOOTH_TILE - 1) else apply_frames + 1,
            SMOOTH_TILE - 1, LEVEL_TILE + 1]


def case_streams(seed, channels, fs):
    """(name, x, factor) of the five streams of a bit-equality case: noise driven over the ceiling, a gated tone, one that is never
    limited, one with a NaN and infinities planted, all zeros.  The gated tone's factor is negative: the level takes |g|"""
    n = case_lengths(channels)
    return [("noise", noise(seed, n[0], channels), GAIN),
            ("gated tone", gated_tone(seed + 1, n[1], channels, fs), -GAIN),
            ("never limited", noise(seed + 2, n[2], channels, 0.05), GAIN),
            ("planted", planted(noise(seed + 3, n[3], channels), seed + 3), GAIN),
            ("zeros", np.zeros((n[4], channels), np.float32), GAIN)]


def ragged_cuts(seed, frames, longest=700):
    """call lengths that add up to `frames`: seeded, with calls of 0 and 1 frames among them"""
    rng = np.random.default_rng([seed, 14])
    cuts, left = [], frames
    while left:
        f = int(rng.choice([0, 1, int(rng.integers(2, longest))]))
        f = min(f, left)
        cuts.append(f)
        left -= f
    return cuts


# ---- the round trip: programmes whose loudness asks for a gain that lifts their peaks over the ceiling
ROUND_TRIP_RATE, ROUND_TRIP_FRAMES = 8000.0, 9600      # 1.2 s: nine gating blocks
ROUND_TRIP_TARGET = -14.0
ROUND_TRIP_RULE = (CEILING_DB, 16, 100)


def round_trip_programmes():
    """stereo: a quiet 997 Hz tone (-30 dBFS) with a 5 ms burst at -4 dBFS every 0.2 s; the tone sets the loudness, the bursts the
    peak.  Three programmes with other burst levels and phases"""
    n = np.arange(ROUND_TRIP_FRAMES, dtype=np.float64)
    out = []
    for s, burst_db in enumerate((-4.0, -6.0, -9.0)):
        tone = 10.0 ** (-30.0 / 20.0) * np.sin(2 * np.pi * 997.0 * n / ROUND_TRIP_RATE + 0.3 * s)
        gate = ((n % 1600) >= 700 + 100 * s) & ((n % 1600) < 740 + 100 * s)
        burst = 10.0 ** (burst_db / 20.0) * np.sin(2 * np.pi * 1733.0 * n / ROUND_TRIP_RATE + 0.7 * s) * gate
        x = tone + burst
        out.append(np.stack([x, 0.8 * x], axis=1).astype(np.float32))
    return out

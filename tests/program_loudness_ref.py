"""f64 numpy restatement of the programme loudness definitions (include/omx/program_loudness.h): the checker of
openmeters_amd.program_loudness.  K-weighting through the oracle's k_weighting_coefficients and scipy.signal.lfilter (the same
transposed direct form II, f64), cast to f32, squared in f64; 100 ms segment means; gating and short-term blocks on the segment grid;
gates on energies; nearest-rank percentiles.  Also returns the GATE MARGIN: the smallest distance in LU between any block and a gate
it is compared with — a block within the parity bar of a gate may legitimately fall on either side, so tests require a margin."""
import numpy as np
from scipy.signal import lfilter

ABSOLUTE_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
WEIGHTS = {3: 0.0, 4: 1.41, 5: 1.41, 6: 1.41, 7: 1.41}   # ChannelPosition: LFE; rear / side left / right; everything else 1.0


def channel_weights(positions, channels):
    return np.array([WEIGHTS.get(int(p), 1.0) for p in positions[:channels]], np.float64)


def sanitize_rate(fs):
    fs = np.float32(fs)
    if not np.isfinite(fs) or fs <= 0:
        fs = np.float32(48000.0)
    return float(min(max(fs, np.float32(1.0)), np.float32(768000.0)))


def segment_frames(fs):
    return (int(sanitize_rate(fs)) + 5) // 10


def level(z):
    return -0.691 + 10.0 * np.log10(z)


def lufs(z, floor):
    """mean_square_to_lufs: floored, f32"""
    return np.float32(max(level(z), float(floor))) if z > 0.0 else np.float32(floor)


def segment_energies(x, fs, positions, coefficients):
    """x: f32 [frames][channels] -> e[j] for the complete segments"""
    b, a = coefficients
    x = np.asarray(x, np.float32)
    frames, channels = x.shape
    seg = segment_frames(fs)
    with np.errstate(all="ignore"):
        y = lfilter(b, a, x.astype(np.float64), axis=0).astype(np.float32).astype(np.float64)
        v = y * y
    v[~np.isfinite(v)] = 0.0
    n = frames // seg
    sums = v[:n * seg].reshape(n, seg, channels).sum(axis=1)
    return (sums * channel_weights(positions, channels)[None, :]).sum(axis=1) / seg


def sliding_mean(e, width):
    """block j = mean of e[j - width + 1 .. j], summed oldest first; index 0 of the result is block j = width - 1"""
    if len(e) < width:
        return np.zeros((0,), np.float64)
    acc = e[0:len(e) - width + 1].copy()
    for k in range(1, width):
        acc = acc + e[k:len(e) - width + 1 + k]
    return acc / float(width)


def _margin(blocks, gate):
    if len(blocks) == 0 or not gate > 0.0:
        return np.inf
    pos = blocks[blocks > 0.0]
    return float(np.abs(level(pos) - level(gate)).min()) if len(pos) else np.inf


def results(e, floor=-99.9):
    """the record of a stream whose stored segment energies are e (dict with the field names of omx_program_loudness_record)"""
    e = np.asarray(e, np.float64)
    g, st = sliding_mean(e, 4), sliding_mean(e, 30)
    r = {"segments": len(e), "gating_blocks": len(g), "short_term_blocks": len(st)}
    margin = min(_margin(g, ABSOLUTE_GATE), _margin(st, ABSOLUTE_GATE))
    ga = g[g > ABSOLUTE_GATE]
    rel = 0.1 * ga.mean() if len(ga) else 0.0
    gr = ga[ga > rel]
    margin = min(margin, _margin(ga, rel))
    r["gating_above_absolute"], r["gating_above_relative"] = len(ga), len(gr)
    r["relative_threshold_energy"] = rel
    r["integrated_energy"] = gr.mean() if len(gr) else 0.0
    sa = st[st > ABSOLUTE_GATE]
    srel = 0.01 * sa.mean() if len(sa) else 0.0
    sr = np.sort(sa[sa > srel])
    margin = min(margin, _margin(sa, srel))
    r["short_term_above_absolute"], r["short_term_above_relative"] = len(sa), len(sr)
    if len(sr):
        lo = sr[int(np.floor((len(sr) - 1) * 0.10 + 0.5))]
        hi = sr[int(np.floor((len(sr) - 1) * 0.95 + 0.5))]
        r["lra_low_energy"], r["lra_high_energy"] = lo, hi
        r["loudness_range_lu"] = np.float32(level(hi) - level(lo))
    else:
        r["lra_low_energy"] = r["lra_high_energy"] = 0.0
        r["loudness_range_lu"] = np.float32(0.0)
    r["momentary_energy"] = g[-1] if len(g) else 0.0
    r["short_term_energy"] = st[-1] if len(st) else 0.0
    r["max_momentary_energy"] = g.max() if len(g) else 0.0
    r["max_short_term_energy"] = st.max() if len(st) else 0.0
    for name in ("integrated", "relative_threshold", "momentary", "short_term", "max_momentary", "max_short_term"):
        r[name + "_lufs"] = lufs(r[name + "_energy"], floor)
    r["gate_margin"] = margin
    r["gating_levels"], r["gating"] = (level(ga) if len(ga) else np.zeros(0)), g
    return r


def restate(x, fs, positions, coefficients, floor=-99.9, capacity_segments=None):
    e = segment_energies(x, fs, positions, coefficients)
    if capacity_segments is not None:
        e = e[:capacity_segments]
    r = results(e, floor)
    r["frames"] = len(x) if capacity_segments is None else min(len(x), capacity_segments * segment_frames(fs))
    r["e"] = e
    return r


# ---- inputs shared by the CPU and the GPU tests
def tone_programme(fs, spans, channels=2, freq=1000.0):
    """EBU Tech 3341 / 3342 synthetic cases: a sine of `freq` Hz in every channel, spans = [(dBFS, seconds), ...]"""
    parts, t0 = [], 0
    for db, seconds in spans:
        n = int(round(fs * seconds))
        t = (t0 + np.arange(n)) / fs
        parts.append(10.0 ** (db / 20.0) * np.sin(2 * np.pi * freq * t))
        t0 += n
    mono = np.concatenate(parts)
    return np.repeat(mono[:, None], channels, axis=1).astype(np.float32)


EBU_3341 = [("3341-1", [(-23, 20)], -23.0), ("3341-2", [(-33, 20)], -33.0), ("3341-3", [(-36, 10), (-23, 60), (-36, 10)], -23.0),
            ("3341-4", [(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0),
            ("3341-5", [(-26, 20), (-20, 20.1), (-26, 20)], -23.0)]
EBU_3342 = [("3342-1", [(-20, 20), (-30, 20)], 10.0), ("3342-2", [(-20, 20), (-15, 20)], 5.0), ("3342-3", [(-40, 20), (-20, 20)], 20.0),
            ("3342-4", [(-50, 20), (-35, 20), (-20, 20), (-35, 20), (-50, 20)], 15.0)]


def programme(seed, fs, ch, seconds):
    """the seeded programme generator of the feature's issue (levels on both sides of both gates)"""
    rng = np.random.default_rng(seed); T = int(fs * seconds); x = np.zeros((T, ch)); t = 0
    while t < T:
        n = int(rng.uniform(0.3, 4.0) * fs); kind = rng.integers(0, 4); lvl = 10 ** (rng.uniform(-75, -6) / 20)
        n = min(n, T - t); tt = np.arange(t, t + n) / fs
        if kind == 0: seg = np.zeros((n, ch))
        elif kind == 1: seg = lvl * np.sin(2 * np.pi * rng.uniform(40, 8000) * tt)[:, None] * rng.uniform(0.3, 1, (1, ch))
        else: seg = lvl * rng.standard_normal((n, ch))
        x[t:t + n] = seg; t += n
    return x.astype(np.float32)


SURROUND_71 = [0, 1, 2, 3, 4, 5, 6, 7]   # FL FR FC LFE RL RR SL SR


def positions_for(ch):
    """fallback positions (reference src/dsp.rs:36-47) as openmeters_amd.capi.positions_fallback"""
    from openmeters_amd import capi
    return capi.positions_fallback(ch)


# (rate, channels, seeds): 40 s programmes.  (48 kHz, 2 ch, seed 2) is left out: its gate margin is 0.0010 LU, below the 2e-3 LU the
# comparison needs (20 x the 1e-4 LU bar); every other case holds it and tests/test_cpu_program_loudness.py asserts that.
SEEDED_CASES = [(48000.0, 2, (0, 1, 3, 4, 5)), (44100.0, 6, (0, 1, 2, 3, 4, 5)), (96000.0, 8, (0, 1, 2, 3, 4, 5))]
SEEDED_SECONDS = 40
GATE_MARGIN_MIN = 2e-3

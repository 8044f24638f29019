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


# ---- the wider matrix (tests/test_gpu_program_loudness_matrix.py; conditions asserted by tests/test_cpu_program_loudness_inputs.py)
# Lowest rate the bank accepts: the K-weighting shelf sits at 1681.97 Hz, and below twice that the bilinear transform puts poles outside
# the unit circle (tests/test_cpu_program_loudness_inputs.py finds the limit from the oracle's coefficients)
MIN_RATE = 3364.0
TIME_PARALLEL_MAX_RATE = 384000.0   # above it the bank runs the reference order whatever form is asked for (last_form() says so)
MAX_RATE = 768000.0

# (rate, channels, seconds, seeds) of `programme`: every channel count, every lane map, segments shorter than a work item (8 and 9 kHz),
# a work item that is no whole number of tiles (9 kHz: 900 frames), an odd segment (11 025 Hz: 1103 frames), rates up to the highest
MATRIX_CASES = [(MIN_RATE, 1, 40, (1, 3, 6)), (8000.0, 1, 40, (1, 2, 3)), (9000.0, 3, 40, (0, 1, 2)), (11025.0, 5, 40, (0, 1, 2)), (22050.0, 4, 40, (0, 1, 2)),
                (32000.0, 7, 40, (0, 1, 2)), (48000.0, 1, 40, (0, 1, 3)), (48000.0, 3, 40, (0, 1, 2)), (48000.0, 4, 40, (0, 3, 4)),
                (48000.0, 5, 40, (0, 1, 2)), (48000.0, 7, 40, (0, 1, 2)), (88200.0, 1, 20, (1, 3, 5)), (176400.0, 1, 20, (1, 2, 6)),
                (192000.0, 1, 20, (0, 1, 2)), (384000.0, 1, 10, (0, 2, 3)), (MAX_RATE, 1, 10, (2, 3, 4))]


def expected_form(pinned, fs):
    """what last_form() reports after a call with the time-parallel form pinned (or picked by shape)"""
    return 1 if pinned == 1 or sanitize_rate(fs) > TIME_PARALLEL_MAX_RATE else 2


HARD_KINDS = ("dc", "5 Hz", "15 Hz", "drop")
HARD_RATES = (48000.0, 96000.0, 192000.0, TIME_PARALLEL_MAX_RATE, MAX_RATE)
HARD_SECONDS = 10


def hard_input(kind, fs, ch, seconds=HARD_SECONDS, seed=0):
    """inputs that leave the K-weighting state large while the output is small (a DC offset, rumble below the 38 Hz high-pass) or that
    follow a loud passage by a quiet one: where a scan over the filter state loses its accuracy first.
      dc / 5 Hz / 15 Hz : an offset / a sine of 0.5 plus noise at -60 dBFS
      drop              : noise at full scale (uniform, +-0.9) for 40 %, the same noise 100 dB lower for 30 %, noise at -60 dBFS
                          (above the absolute gate, below the relative one) for the rest"""
    rng = np.random.default_rng([seed, HARD_KINDS.index(kind), ch])
    n = int(fs * seconds)
    quiet = np.float32(1e-3) * rng.standard_normal((n, ch), dtype=np.float32)
    if kind == "dc":
        return quiet + np.float32(0.5)
    if kind in ("5 Hz", "15 Hz"):
        f = 5.0 if kind == "5 Hz" else 15.0
        return quiet + (0.5 * np.sin(2 * np.pi * f * np.arange(n) / fs)).astype(np.float32)[:, None]
    assert kind == "drop"
    a, b = int(0.4 * n), int(0.7 * n)
    loud = (rng.random((b, ch), dtype=np.float32) * np.float32(1.8) - np.float32(0.9))
    loud[a:] *= np.float32(1e-5)
    quiet[:b] = loud
    return quiet


def long_loud_then_quiet(fs, ch, seed=0):
    """90 s of noise at full scale (uniform, +-0.9), then 8 s of noise at -60 dBFS"""
    rng = np.random.default_rng([seed, 90, ch])
    loud = rng.random((int(fs * 90), ch), dtype=np.float32) * np.float32(1.8) - np.float32(0.9)
    return np.concatenate([loud, np.float32(1e-3) * rng.standard_normal((int(fs * 8), ch), dtype=np.float32)])


def segment_energies_per_call(x, fs, calls, coefficients):
    """as segment_energies, for a programme whose positions change between calls: calls = [(frames, positions), ...]; a sample takes
    the weights of the call it arrived in (include/omx/program_loudness.h)"""
    b, a = coefficients
    x = np.asarray(x, np.float32)
    frames, channels = x.shape
    assert sum(n for n, _ in calls) == frames
    seg = segment_frames(fs)
    with np.errstate(all="ignore"):
        y = lfilter(b, a, x.astype(np.float64), axis=0).astype(np.float32).astype(np.float64)
        v = y * y
    v[~np.isfinite(v)] = 0.0
    at = 0
    for n, positions in calls:
        v[at:at + n] *= channel_weights(positions, channels)[None, :]
        at += n
    n = frames // seg
    return v[:n * seg].reshape(n, seg, channels).sum(axis=1).sum(axis=1) / seg


# ---- the result pass on its own: ref.results(bank.fetch_segments(s)) against bank.fetch(s)
def energy_bound(n):
    """Relative bound on an energy field that is the mean of n blocks (n = 0: a single block), between the result pass and `results`
    fed the same e[].  u = 2^-53.  A block is a sum of 4 or 30 non-negative f64 terms and a division: within (29 + 1) u of its exact
    value on either side (both sides add oldest first, so the blocks are in fact the same bits).  A sum of n non-negative terms in
    ANY order is within (n - 1) u of exact, relatively, because no partial sum exceeds the total; the division by the count and the
    gate's factor 0.1 add one u each, which the 30 u of the blocks' own slack covers when the blocks are identical.  The two sides
    order the sum differently (lane-strided partials and a binary tree; numpy's pairwise sum), and each depth is far below n / 2 for
    n > 64 (n / 256 + 8 and about 19 + log2 n additions), so their distance stays below (n + 30) u: first order in u, all terms
    non-negative, nothing measured."""
    return (n + 30) * 2.0 ** -53


def result_pass_order_mean(values):
    """the mean of `values` in the order of the result pass: 256 lane-strided partial sums, then a binary tree (pl_result_kernel)"""
    lanes = np.zeros(256, np.float64)
    for k in range(0, len(values), 256):
        part = values[k:k + 256]
        lanes[:len(part)] += part
    d = 128
    while d:
        lanes[:d] += lanes[d:2 * d]
        d //= 2
    return lanes[0] / float(len(values))


HOUR_RATE, HOUR_SECONDS = 8000.0, 3600


def hour_programme(kind, fs=HOUR_RATE, seconds=HOUR_SECONDS, seed=0):
    """long mono programmes made cheap by a low rate, for the result pass (ranks and gates over tens of thousands of blocks).
      tone  : of every 30 min, a 1 kHz sine at -26 dBFS for 11 min, then at -20 dBFS for 14 min (a whole number of periods per
              segment: runs of thousands of EQUAL short-term blocks at two levels, so each loudness-range rank falls inside a run of
              equal keys), stepped noise for the rest
      steps : noise whose level steps every 2 ... 20 s between -80 and -10 dBFS, with silences: blocks on both sides of both gates"""
    rng = np.random.default_rng([seed, 3600, 0 if kind == "tone" else 1])
    n = int(fs * seconds)
    x = rng.standard_normal(n, dtype=np.float32)
    gain = np.empty(n, np.float32)
    t = 0
    while t < n:
        m = min(int(rng.uniform(2.0, 20.0) * fs), n - t)
        gain[t:t + m] = 0.0 if rng.random() < 0.1 else 10.0 ** (rng.uniform(-80.0, -10.0) / 20.0)
        t += m
    x *= gain
    if kind == "tone":
        period = int(fs * 1800)
        tone = (0.1 * np.sin(2 * np.pi * 1000.0 * np.arange(int(fs * 1500)) / fs)).astype(np.float32)
        tone[:int(fs * 660)] *= np.float32(0.5)
        for t0 in range(0, n, period):
            m = min(len(tone), n - t0)
            x[t0:t0 + m] = tone[:m]
    return x[:, None]


RESULT_PASS_MARGIN_MIN = 1e-6   # LU: both sides of that comparison read the same e[], so the margin only has to exceed energy_bound

# ---- bank shapes and ragged calls: a pool of short programmes of different lengths (seed, seconds), streams take them in turn
SHAPE_RATE = 48000.0
SHAPE_POOL = {2: [(0, 4.0), (1, 4.37), (3, 5.11), (4, 5.83), (5, 6.29)], 3: [(0, 4.0), (1, 4.37), (3, 5.11), (4, 5.83), (5, 6.29)]}
SHAPE_CASES = [(SHAPE_RATE, ch, seconds, (seed,)) for ch, pool in SHAPE_POOL.items() for seed, seconds in pool]
REAR_POSITIONS = [4, 5, 6, 7, 4, 5, 6, 7]    # rear / side: weight 1.41 in every channel
FRONT_POSITIONS = [0, 1, 2, 0, 1, 2, 0, 1]   # weight 1.0 in every channel
WEIGHT_CHANGE_CASE = (SHAPE_RATE, 2, 12, 1)  # (rate, channels, seconds, seed)


def shape_programmes(ch, n_streams):
    pool = [programme(seed, SHAPE_RATE, ch, seconds) for seed, seconds in SHAPE_POOL[ch]]
    return [pool[s % len(pool)] for s in range(n_streams)]


# the calls of the one-hour test, (frames of stream 0, frames of stream 1): `tone` ends 1.5 segments short of the capacity, `steps` fills
# it exactly with its last segment
HOUR_CALLS = [(4_800_000, 4_800_000), (2960, 2960), (1_440_000, 1_440_001), (1, 1), (12_000_000, 12_000_000), (10_555_839, 10_557_038)]


def segment_energies_long(x, fs, positions, coefficients, chunk_segments=36000):
    """segment_energies for programmes too long to filter in one piece: the same sequential recurrence, carried from chunk to chunk
    through lfilter's state (chunks of whole segments)"""
    b, a = np.asarray(coefficients[0], np.float64), np.asarray(coefficients[1], np.float64)
    frames, channels = x.shape
    seg = segment_frames(fs)
    zi, out = np.zeros((4, channels)), []
    for t in range(0, frames // seg * seg, chunk_segments * seg):
        part = x[t:min(t + chunk_segments * seg, frames // seg * seg)]
        with np.errstate(all="ignore"):
            y, zi = lfilter(b, a, part.astype(np.float64), axis=0, zi=zi)
            y = y.astype(np.float32).astype(np.float64)
            v = y * y
        v[~np.isfinite(v)] = 0.0
        sums = v.reshape(len(part) // seg, seg, channels).sum(axis=1)
        out.append((sums * channel_weights(positions, channels)[None, :]).sum(axis=1) / seg)
    return np.concatenate(out)


FOUR_HOURS_SECONDS, FOUR_HOURS_SEED = 4 * 3600, 0   # 144 000 segments at 8 kHz mono: hour_programme("steps", seconds=FOUR_HOURS_SECONDS)

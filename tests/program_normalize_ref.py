"""numpy restatement of the programme bank's normalisation (include/omx/program_normalize.h, DESIGN.md section 10 "Normalisation"):
the gain of steps 1 - 7, in f64 on np.float32 inputs and rounded where the definition rounds, and the pass out = x * f32(gain) with its
count of samples over full scale and its peak.  It reads nothing from the library.  Also the rules and shapes shared by
tests/test_cpu_program_normalize.py and tests/test_gpu_program_normalize.py."""
import numpy as np

LIMIT_PEAK = 1
BY_TARGET, BY_PEAK, BY_MAX_GAIN, BY_MIN_GAIN, BY_NO_MEASUREMENT = 0, 1, 2, 3, 4
UNITY = 2 ** 32 - 1
RECORD_FIELDS = ("gain_db", "gain", "source_lufs", "source_peak_db", "predicted_lufs", "predicted_peak_db", "limited_by", "peak_known")
EXACT_FIELDS = ("gain_db", "source_lufs", "source_peak_db", "predicted_lufs", "predicted_peak_db", "limited_by", "peak_known")


def gain(rule, integrated_lufs, gating_above_relative, max_true_peak_db, floor_db):
    """rule: (target_lufs, true_peak_ceiling_db, min_gain_db, max_gain_db, flags).  Returns the record as a dict of np.float32 / int."""
    target, ceiling, lo, hi = (np.float32(v) for v in rule[:4])
    flags = int(rule[4])
    I, P, F = np.float32(integrated_lufs), np.float32(max_true_peak_db), np.float32(floor_db)
    peak_known = bool(P > F)
    r = {"source_lufs": I, "source_peak_db": P, "peak_known": int(peak_known)}
    if int(gating_above_relative) == 0:
        r.update(gain_db=np.float32(0.0), gain=np.float32(1.0), predicted_lufs=I, predicted_peak_db=P, limited_by=BY_NO_MEASUREMENT)
        return r
    g, by = np.float64(target) - np.float64(I), BY_TARGET
    if (flags & LIMIT_PEAK) and peak_known:
        pg = np.float64(ceiling) - np.float64(P)
        if pg < g:
            g, by = pg, BY_PEAK
    if g > np.float64(hi):
        g, by = np.float64(hi), BY_MAX_GAIN
    if g < np.float64(lo):
        g, by = np.float64(lo), BY_MIN_GAIN
    with np.errstate(all="ignore"):
        gain_db = np.float32(g)
        r["gain_db"] = gain_db
        r["gain"] = np.float32(np.power(np.float64(10.0), np.float64(gain_db) / np.float64(20.0)))
        r["predicted_lufs"] = np.float32(np.float64(I) + np.float64(gain_db))
        r["predicted_peak_db"] = np.float32(np.float64(P) + np.float64(gain_db)) if peak_known else F
    r["limited_by"] = by
    return r


def ulps(a, b):
    """distance of two finite f32 of the same sign in units of the last place"""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def check_record(got, want, tag):
    """got: a GAIN_RECORD_DTYPE scalar.  gain_db, predicted_*, source_*, limited_by and peak_known equal bits; gain within 1 f32 ulp
    (pow is the only step whose f64 result may differ between libraries, and one f64 ulp moves the f32 rounding by at most one)"""
    for f in EXACT_FIELDS:
        w = np.float32(want[f]) if f not in ("limited_by", "peak_known") else np.uint32(want[f])
        assert got[f].tobytes() == w.tobytes(), (tag, f, got[f], want[f])
    assert ulps(got["gain"], want["gain"]) <= 1, (tag, "gain", got["gain"], want["gain"])


def apply(x, g):
    """(out, samples_over, out_sample_peak): out = x * f32(g), one f32 multiply; |out| > 1 counted (NaN not, infinity yes); the peak
    with fmaxf semantics (NaN ignored), 0 for no sample"""
    with np.errstate(all="ignore"):
        out = (np.asarray(x, np.float32) * np.float32(g)).astype(np.float32)
        mag = np.abs(out)
        over = int(np.count_nonzero(mag > np.float32(1.0)))
        finite_or_inf = mag[~np.isnan(mag)]
    peak = np.float32(finite_or_inf.max()) if finite_or_inf.size else np.float32(0.0)
    return out, over, peak


def peak_db(peak, floor_db):
    """power_to_db(p * p, floor_db) of include/omx/program_peaks.h, in f64 (compared within 1e-4 dB)"""
    with np.errstate(all="ignore"):
        p2 = np.float32(peak) * np.float32(peak)
    if not p2 > 0:
        return float(floor_db)
    return float("inf") if np.isinf(p2) else max(10.0 * np.log10(np.float64(p2)), float(floor_db))


# ---------------------------------------------------------------- rules shared by the CPU and the GPU file
# (target, ceiling, min, max, flags) over the five known programmes of program_groups_ref (-23, -29, -50, -20, -30 dBFS tones, true
# peak = the tone's level within 0.01 dB)
RULE_TARGET = (-23.0, -1.0, -60.0, 60.0, 0)
RULE_CEILING = (-23.0, -25.0, -60.0, 60.0, LIMIT_PEAK)      # a tone's peak sits at its loudness: the ceiling 2 dB below the target holds every stream
RULE_CLAMPS = (-23.0, -25.0, -1.5, 4.5, LIMIT_PEAK)         # peak-limited gains of -2, +4, +25, -5, +5 dB: min, peak, max, min, max
KNOWN_TRACK_GAINS_DB = (0.0, 6.0, 27.0, -3.0, 7.0)

# ---------------------------------------------------------------- shapes of the pass
APPLY_CAPACITY = 1001
APPLY_CHANNELS = (1, 2, 3, 5, 8)
APPLY_FRAMES = (0, 1, 3, 4, 5, 255, 256, 257, 1001)
LONG_FRAMES, LONG_CHANNELS = 70001, 2


def planted(x, seed):
    """a copy of x (f32, any shape) with NaN, both infinities, denormals and -0.0 at seeded places (when it has room for them)"""
    x = np.array(x, np.float32)
    flat = x.reshape(-1)
    specials = np.array([np.nan, np.inf, -np.inf, 1e-40, -3e-42, -0.0, 0.0, 1.0, -1.0], np.float32)
    if flat.size >= 4 * len(specials):
        at = np.random.default_rng([seed, 128]).choice(flat.size, len(specials), replace=False)
        flat[at] = specials
    return x


def noise(seed, frames, channels, scale=0.9):
    return (np.random.default_rng([seed, 7]).uniform(-scale, scale, (frames, channels))).astype(np.float32)

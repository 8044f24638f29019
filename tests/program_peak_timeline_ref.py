"""numpy restatement of the programme bank's peak timeline (include/omx/program_peak_timeline.h), frame by
frame, on top of tests/program_peaks_ref.py: the checker of ProgramLoudnessBank.peak_rows / *_interval_peaks / *_group_peaks.

With v[n] and |x[n]| of program_peaks_ref (the interpolator runs over the WHOLE programme since the reset, so its history is the
programme's) and L = (uint(fs) + 5) // 10:
  peak segment j = frames [j L, min((j + 1) L, N)), ceil(N / L) of them, the last one possibly open;
  per channel true_peak[j] = max v, sample_peak[j] = max |x| over them (from 0, NaN ignored), each with the offset of the first frame
  that reaches it (0 for a peak of 0);
  row i of (first, stride, count) = the maximum over the segments [first + i stride, first + (i + 1) stride) that exist, the earlier
  frame on a tie, offsets from the row's first frame; an interval peak = the same over COMPLETE segments with frames counted from the
  reset; a group peak = the maximum over its members, the first member and then the earliest frame on a tie."""
import numpy as np

import program_peaks_ref as pref
from program_loudness_ref import sanitize_rate

MAX_CHANNELS = pref.MAX_CHANNELS
TO_END = 2 ** 64 - 1
PEAK_ROW_DTYPE = np.dtype([("true_peak", "<f4", (8,)), ("sample_peak", "<f4", (8,)), ("true_peak_offset", "<u4", (8,)),
                           ("sample_peak_offset", "<u4", (8,)), ("frames", "<u4"), ("valid", "<u4")])
PART_PEAK_DTYPE = np.dtype([("frames", "<u8"), ("true_peak_frame", "<u8", (8,)), ("sample_peak_frame", "<u8", (8,)),
                            ("true_peak_member", "<u4", (8,)), ("sample_peak_member", "<u4", (8,)), ("true_peak", "<f4", (8,)),
                            ("sample_peak", "<f4", (8,)), ("true_peak_db", "<f4", (8,)), ("sample_peak_db", "<f4", (8,)),
                            ("max_true_peak_db", "<f4"), ("max_sample_peak_db", "<f4"), ("max_true_peak_channel", "<u4"),
                            ("channels", "<u4")])
DB_FIELDS = ("true_peak_db", "sample_peak_db", "max_true_peak_db", "max_sample_peak_db")


def segment_frames(fs):
    return (int(sanitize_rate(fs)) + 5) // 10


def coefficients():
    """(fir4 [12][3], fir2 [24]) from the header's formula, f64 rounded to f32 (tests/test_cpu_program_peak_timeline.py holds them to
    the oracle's)"""
    def c(j, factor):
        x = (j - 24.0) * np.pi / factor
        return np.float32(0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0)) * np.sin(x) / x)
    fir4 = np.array([[c(4 * t + p + 1, 4) for p in range(3)] for t in range(12)], np.float32)
    fir2 = np.array([c(2 * t + 1, 2) for t in range(24)], np.float32)
    return fir4, fir2


def frame_values(x, fs, coeffs):
    """x: f32 [N][channels] -> (v, m): f32 [N][channels], v[n] = the true-peak value of frame n, m[n] = |x[n]|; a NaN stays a NaN
    only where every operand was one"""
    x = np.asarray(x, np.float32)
    fir4, fir2 = coeffs
    factor = pref.oversampling(fs)
    with np.errstate(all="ignore"):
        m = np.abs(x)
        v = m.copy()
        for c in range(x.shape[1]):
            col = np.ascontiguousarray(x[:, c])
            outs = [pref.interpolated(col, fir4[:, p]) for p in range(3)] if factor == 4 else ([pref.interpolated(col, fir2)] if factor == 2 else [])
            for o in outs:
                v[:, c] = np.fmax(v[:, c], np.abs(o))
    return v, m


def _first_max(a):
    """(max from 0 ignoring NaN, index of the first frame that reaches it or 0 for a maximum of 0) of a 1-d f32 array"""
    if len(a) == 0:
        return np.float32(0.0), 0
    with np.errstate(all="ignore"):
        a = np.fmax(a, np.float32(0.0))
    peak = a.max()
    return np.float32(peak), (int(np.argmax(a == peak)) if peak > 0 else 0)


def segment_peaks(x, fs, coeffs):
    """x: f32 [N][channels], the frames taken since the reset -> dict: L, frames, channels, and per kind arrays [segments][channels]
    `true_peak` / `true_offset` / `sample_peak` / `sample_offset`, frame by frame"""
    x = np.asarray(x, np.float32)
    n, ch = x.shape
    L = segment_frames(fs)
    v, m = frame_values(x, fs, coeffs)
    segs = (n + L - 1) // L
    out = {"L": L, "frames": n, "channels": ch, "true_peak": np.zeros((segs, ch), np.float32), "true_offset": np.zeros((segs, ch), np.int64),
           "sample_peak": np.zeros((segs, ch), np.float32), "sample_offset": np.zeros((segs, ch), np.int64)}
    for j in range(segs):
        for c in range(ch):
            out["true_peak"][j, c], out["true_offset"][j, c] = _first_max(v[j * L:(j + 1) * L, c])
            out["sample_peak"][j, c], out["sample_offset"][j, c] = _first_max(m[j * L:(j + 1) * L, c])
    return out


def _over(sp, kind, c, j0, j1):
    """maximum of one kind and channel over the segments [j0, j1): (value, frames from segment j0's first frame); earliest on a tie"""
    best, at = np.float32(0.0), 0
    for j in range(j0, j1):
        p = sp[kind + "_peak"][j, c]
        if p > best:
            best, at = p, (j - j0) * sp["L"] + int(sp[kind + "_offset"][j, c])
    return best, at


def rows(sp, first, stride, count):
    """omx_program_peak_row [count] of one stream from its segment_peaks"""
    out = np.zeros(count, PEAK_ROW_DTYPE)
    segs, L = len(sp["true_peak"]), sp["L"]
    for i in range(count):
        j0 = first + i * stride
        if j0 >= segs:
            continue
        j1 = min(j0 + stride, segs)
        for c in range(sp["channels"]):
            out[i]["true_peak"][c], out[i]["true_peak_offset"][c] = _over(sp, "true", c, j0, j1)
            out[i]["sample_peak"][c], out[i]["sample_peak_offset"][c] = _over(sp, "sample", c, j0, j1)
        out[i]["frames"] = min(sp["frames"], j1 * L) - j0 * L
        out[i]["valid"] = 1
    return out


def part_peaks(sps, members, groups=None, floor=-99.9):
    """sps: the segment_peaks of every stream; members: (stream, first_segment, segment_count) with TO_END allowed; groups:
    (first_member, member_count) or None = every member a part of its own -> omx_program_part_peak [parts]"""
    floor = np.float32(floor)
    if groups is None:
        groups = [(i, 1) for i in range(len(members))]
    out = np.zeros(len(groups), PART_PEAK_DTYPE)
    for k, (g0, gn) in enumerate(groups):
        r = out[k]
        r["true_peak_db"][:] = floor
        r["sample_peak_db"][:] = floor
        ch = 0
        for mi in range(gn):
            s, first, n = members[g0 + mi]
            sp = sps[s]
            stored = sp["frames"] // sp["L"]                     # complete segments
            n = stored - first if n == TO_END else n
            assert first + n <= stored
            r["frames"] += n * sp["L"]
            ch = sp["channels"]
            for c in range(ch):
                for kind in ("true", "sample"):
                    p, at = _over(sp, kind, c, first, first + n)
                    if p > r[kind + "_peak"][c]:                 # strictly greater: the first member wins a tie
                        r[kind + "_peak"][c] = p
                        r[kind + "_peak_member"][c] = mi
                        r[kind + "_peak_frame"][c] = first * sp["L"] + at
        r["channels"] = ch if r["frames"] else 0
        with np.errstate(all="ignore"):
            for c in range(MAX_CHANNELS):
                r["true_peak_db"][c] = pref.power_to_db_f32(r["true_peak"][c] * r["true_peak"][c], floor)
                r["sample_peak_db"][c] = pref.power_to_db_f32(r["sample_peak"][c] * r["sample_peak"][c], floor)
        used = int(r["channels"])
        r["max_true_peak_db"] = max([floor] + list(r["true_peak_db"][:used]))
        r["max_sample_peak_db"] = max([floor] + list(r["sample_peak_db"][:used]))
        r["max_true_peak_channel"] = int(np.argmax(r["true_peak"][:used])) if used and r["true_peak"][:used].max() > 0 else 0
    return out


def split_db(records):
    """(the records with the dB fields zeroed, for a comparison on bytes; the dB fields as one f64 array, for the 1e-4 dB bar)"""
    rest = records.copy()
    db = np.concatenate([np.asarray(records[f], np.float64).reshape(len(records), -1) for f in DB_FIELDS], axis=1)
    for f in DB_FIELDS:
        rest[f] = 0
    return rest, db


def hard_programme(seed, frames, ch):
    """seeded noise with NaN, +-inf, -0.0 and denormals sprinkled in (at most one infinity per channel, away from the ends)"""
    rng = np.random.default_rng(7000 + seed)
    x = (0.3 * rng.standard_normal((frames, ch))).astype(np.float32)
    if frames >= 8:
        for c in range(ch):
            at = rng.choice(frames, size=min(6, frames), replace=False)
            x[at[0], c] = np.nan
            x[at[1], c] = -0.0
            x[at[2], c] = np.float32(1e-41)
            x[at[3], c] = np.float32(-3e-39)
            if frames >= 64 and c % 2 == 0:
                x[at[4], c] = np.inf if c % 4 == 0 else -np.inf
            x[at[5], c] = np.nan
    return x

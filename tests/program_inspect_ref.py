"""numpy restatement of the programme bank's signal QC, written from the DEFINITION and the SUMMARY in include/omx/program_inspect.h and
from nothing else: the record of a stream from all the PCM it took since its reset (no tiles, no calls: run lengths are one running
count over the whole programme), and the summary of a record.  Every float operation is one f32 operation of numpy; the sums are
Python integers (exact) stored as 64-bit."""
import math

import numpy as np

MAX_PAIRS = 4
DB_FLOOR = -400.0
NAN, CLIPPED, DROPOUT, ALL_SILENT, DC, ANTIPHASE = 1, 2, 4, 8, 16, 32
CHANNEL_FIELDS = ("dc_sum", "nan_samples", "clipped_samples", "clip_runs", "longest_clip_run", "longest_clip_start", "open_clip_run", "_pad")
PAIR_FIELDS = ("sum_ab", "sum_aa", "sum_bb", "a", "b")
STREAM_FIELDS = ("frames", "silent_frames", "silent_runs", "longest_silent_run", "longest_silent_start", "leading_silence", "trailing_silence")
CHANNEL_DTYPE = np.dtype([("dc_sum", "<i8")] + [(f, "<u8") for f in CHANNEL_FIELDS[1:]])
PAIR_DTYPE = np.dtype([("sum_ab", "<i8"), ("sum_aa", "<u8"), ("sum_bb", "<u8"), ("a", "<u4"), ("b", "<u4")])
RECORD_DTYPE = np.dtype([(f, "<u8") for f in STREAM_FIELDS] + [("channels", "<u4"), ("n_pairs", "<u4"), ("channel", CHANNEL_DTYPE, (8,)),
                                                               ("pair", PAIR_DTYPE, (MAX_PAIRS,))])
assert CHANNEL_DTYPE.itemsize == 64 and PAIR_DTYPE.itemsize == 32 and RECORD_DTYPE.itemsize == 704


class Invalid(ValueError):
    """OMX_ERR_INVALID"""


class Rule:
    """omx_program_inspect_rule with the header's defaults"""

    def __init__(self, clip_level=0.99996948, clip_min_run=3, silence_level=0.0, silence_min_run=480, dc_limit=1e-3, correlation_min=-0.2,
                 flags=0):
        self.clip_level, self.silence_level = np.float32(clip_level), np.float32(silence_level)
        self.dc_limit, self.correlation_min = np.float32(dc_limit), np.float32(correlation_min)
        self.clip_min_run, self.silence_min_run, self.flags = clip_min_run, silence_min_run, flags

    def valid(self):
        return bool(np.isfinite(self.clip_level) and self.clip_level > 0 and 1 <= self.clip_min_run <= 65535
                    and np.isfinite(self.silence_level) and self.silence_level >= 0 and 1 <= self.silence_min_run <= 2 ** 24
                    and np.isfinite(self.dc_limit) and self.dc_limit >= 0 and -1 <= self.correlation_min <= 1 and self.flags == 0)


def run_lengths(mask):
    """R[n] = mask[n] ? R[n-1] + 1 : 0"""
    mask = np.asarray(mask, bool)
    n = np.arange(len(mask), dtype=np.int64)
    last_clear = np.maximum.accumulate(np.where(mask, np.int64(-1), n)) if len(mask) else n
    return n - last_clear


def run_figures(mask, min_run):
    """-> (set frames, frames at which a run reaches min_run, longest run, its earliest start, the run open at the end)"""
    r = run_lengths(mask)
    if not len(r):
        return 0, 0, 0, 0, 0
    longest = int(r.max())
    start = int(np.flatnonzero(r == longest)[0]) - longest + 1 if longest else 0
    return int(np.count_nonzero(mask)), int(np.count_nonzero(r == min_run)), longest, start, int(r[-1])


def fixed(values, limit, scale):
    """NaN gives 0; otherwise rint(clamp(v, -limit, limit) * scale), ties to even, as exact integers (int64)"""
    v = np.asarray(values, np.float32)
    nan = np.isnan(v)
    with np.errstate(all="ignore"):
        vc = np.minimum(np.maximum(np.where(nan, np.float32(0), v), np.float32(-limit)), np.float32(limit))
        q = np.rint(vc * np.float32(scale))       # f32 * f32 -> f32, an exact scaling by a power of two
    return np.where(nan, 0, q.astype(np.int64))


def record(x, channels, rule, pairs=()):
    """the record of a stream that took x (f32 [frames][channels]) since its reset, as a RECORD_DTYPE scalar"""
    x = np.asarray(x, np.float32).reshape(-1, channels)
    n = len(x)
    out = np.zeros((), RECORD_DTYPE)
    out["channels"], out["n_pairs"] = channels, len(pairs)
    with np.errstate(all="ignore"):
        mag = np.abs(x)
        hot = mag >= rule.clip_level          # false for NaN, true for infinity
        quiet = (mag <= rule.silence_level).all(axis=1)       # one NaN in the frame makes it false
    out["frames"] = n
    silent, runs, longest, start, open_run = run_figures(quiet, rule.silence_min_run)
    out["silent_frames"], out["silent_runs"], out["longest_silent_run"], out["longest_silent_start"] = silent, runs, longest, start
    out["trailing_silence"] = open_run
    loud = np.flatnonzero(~quiet)
    out["leading_silence"] = int(loud[0]) if len(loud) else n
    for c in range(channels):
        ch = out["channel"][c]
        clipped, runs, longest, start, open_run = run_figures(hot[:, c], rule.clip_min_run)
        ch["dc_sum"] = int(fixed(x[:, c], 4.0, 268435456.0).sum(dtype=np.int64))
        ch["nan_samples"] = int(np.isnan(x[:, c]).sum())
        ch["clipped_samples"], ch["clip_runs"], ch["longest_clip_run"], ch["longest_clip_start"], ch["open_clip_run"] = (
            clipped, runs, longest, start, open_run)
    for p, (a, b) in enumerate(pairs):
        pr = out["pair"][p]
        with np.errstate(all="ignore"):
            ab, aa, bb = x[:, a] * x[:, b], x[:, a] * x[:, a], x[:, b] * x[:, b]      # each rounded to f32
        pr["sum_ab"] = int(fixed(ab, 1.0, 1073741824.0).sum(dtype=np.int64))
        pr["sum_aa"] = int(fixed(aa, 1.0, 1073741824.0).sum(dtype=np.int64))
        pr["sum_bb"] = int(fixed(bb, 1.0, 1073741824.0).sum(dtype=np.int64))
        pr["a"], pr["b"] = a, b
    return out


def summarize(rule, rec):
    """omx_program_inspect_summarize -> dict"""
    channels, n_pairs, frames = int(rec["channels"]), int(rec["n_pairs"]), int(rec["frames"])
    if not rule.valid() or not 1 <= channels <= 8 or n_pairs > MAX_PAIRS:
        raise Invalid()
    verdict = 0
    dc_offset, dc_db = [0.0] * 8, [0.0] * 8
    for c in range(channels):
        ch = rec["channel"][c]
        dc = np.float32(float(int(ch["dc_sum"])) / 268435456.0 / float(frames)) if frames else np.float32(0)
        dc_offset[c] = float(dc)
        dc_db[c] = max(20.0 * math.log10(abs(float(dc))), DB_FLOOR) if dc != 0 else DB_FLOOR
        if int(ch["nan_samples"]):
            verdict |= NAN
        if int(ch["clip_runs"]):
            verdict |= CLIPPED
        if abs(dc) > rule.dc_limit:
            verdict |= DC
    correlation, valid = [0.0] * MAX_PAIRS, [0] * MAX_PAIRS
    for p in range(n_pairs):
        pr = rec["pair"][p]
        ab, aa, bb = int(pr["sum_ab"]), int(pr["sum_aa"]), int(pr["sum_bb"])
        if aa > 0 and bb > 0:
            v = np.float32(min(max(float(ab) / math.sqrt(float(aa) * float(bb)), -1.0), 1.0))
            correlation[p], valid[p] = float(v), 1
            if v < rule.correlation_min:
                verdict |= ANTIPHASE
    lead, trail = int(rec["leading_silence"]), int(rec["trailing_silence"])
    interior = int(rec["silent_runs"]) - (1 if lead >= rule.silence_min_run else 0) - (
        1 if trail >= rule.silence_min_run and lead < frames else 0)
    if interior > 0:
        verdict |= DROPOUT
    if frames > 0 and lead == frames:
        verdict |= ALL_SILENT
    return {"verdict": verdict, "channels": channels, "n_pairs": n_pairs, "interior_silent_runs": interior, "dc_offset": dc_offset,
            "dc_offset_db": dc_db, "correlation": correlation, "correlation_valid": valid}


def noise(seed, frames, channels, scale=1.2, quiet_every=7):
    """uniform noise in [-scale, scale) (some samples hot at the default clip level) with every quiet_every-th frame, and short
    stretches behind some of them, set to zero"""
    rng = np.random.default_rng(seed)
    x = (rng.random((frames, channels), dtype=np.float32) * np.float32(2) - np.float32(1)) * np.float32(scale)
    if frames:
        z = np.zeros(frames, bool)
        z[::quiet_every] = True
        z[1::3 * quiet_every] = True
        z[2::9 * quiet_every] = True
        x[z] = 0
        x[rng.random((frames, channels)) < 0.05] = np.float32(1.0)     # hot samples that repeat: runs of hot samples
    return x

"""numpy restatement of the programme bank's edit pass (include/omx/program_edit.h, DEFINITION): the phase in uint64, the curve by
three rounded f32 operations, the weight of a clip at a frame, the copy rule, the order of the sum of two clips, the zero fill, windows,
the record, trim and extent.  Frame by frame in numpy arrays: no spans, no tiles, nothing of how the library walks a table.

The curve TABLES are data here: the functions take `tabs`, a mapping curve -> f32 [4097] (openmeters_amd.edit_curve gives the library's
for bit comparisons, `analytic_tables()` numpy's own); tests/test_cpu_program_edit.py checks the library's tables separately."""
from dataclasses import dataclass

import numpy as np

CURVE_LINEAR, CURVE_EQUAL_POWER, CURVE_RAISED_COSINE = 0, 1, 2
CURVES = (CURVE_LINEAR, CURVE_EQUAL_POWER, CURVE_RAISED_COSINE)
POINTS = 4097
MAX_FADE = 1 << 24
MAX_POSITION = 1 << 40
RECORD_DTYPE = np.dtype([("out_first", "<u8"), ("frames", "<u8"), ("silent_frames", "<u8"), ("faded_frames", "<u8"), ("mixed_frames", "<u8"),
                         ("samples_over", "<u8"), ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("clips", "<u4"), ("_pad", "<u4")])
EXACT_FIELDS = tuple(f for f in RECORD_DTYPE.names if f != "out_sample_peak_db")
COUNT_FIELDS = ("frames", "silent_frames", "faded_frames", "mixed_frames", "samples_over")


class Invalid(ValueError):
    pass


@dataclass
class Clip:
    src_stream: int = 0
    dst_stream: int = 0
    src_first: int = 0
    dst_first: int = 0
    frames: int = 0
    fade_in_frames: int = 0
    fade_out_frames: int = 0
    fade_in_curve: int = CURVE_LINEAR
    fade_out_curve: int = CURVE_LINEAR
    flags: int = 0
    gain: float = 1.0


@dataclass
class Trim:
    keep_head: int = 0
    keep_tail: int = 0
    pad_head: int = 0
    pad_tail: int = 0
    fade_in_frames: int = 0
    fade_out_frames: int = 0
    fade_in_curve: int = CURVE_LINEAR
    fade_out_curve: int = CURVE_LINEAR
    flags: int = 0


# ---------------------------------------------------------------- phase and curve
def analytic_curve(curve):
    """the curve in double at k / 4096, k = 0 .. 4096"""
    x = np.arange(POINTS, dtype=np.float64) / 4096.0
    if curve == CURVE_LINEAR:
        return x
    if curve == CURVE_EQUAL_POWER:
        return np.sin(np.pi / 2.0 * x)
    if curve == CURVE_RAISED_COSINE:
        return 0.5 - 0.5 * np.cos(np.pi * x)
    raise Invalid("curve")


def analytic_tables():
    out = {}
    for c in CURVES:
        t = analytic_curve(c).astype(np.float32)
        t[0], t[-1] = 0.0, 1.0
        out[c] = t
    return out


def phase(fade_frames, index):
    """p of the DEFINITION for an array of indices, in uint64 throughout"""
    if not 1 <= fade_frames <= MAX_FADE:
        raise Invalid("fade_frames")
    i = np.asarray(index, np.uint64)
    if i.size and int(i.max()) >= fade_frames:
        raise Invalid("index")
    m = np.uint64((1 << 63) // fade_frames)
    return ((np.uint64(2) * i + np.uint64(1)) * m) >> np.uint64(40)


def gain(tab, fade_frames, index):
    """g of the DEFINITION: three f32 operations, each rounded"""
    p = phase(fade_frames, index)
    k = (p >> np.uint64(12)).astype(np.int64)
    tab = np.asarray(tab, np.float32)
    a, b = tab[k], tab[k + 1]
    fr = (p & np.uint64(4095)).astype(np.float32) * np.float32(2.0 ** -12)
    d = (b - a).astype(np.float32)
    t = (d * fr).astype(np.float32)
    return (a + t).astype(np.float32)


# ---------------------------------------------------------------- tables
def clip_refusal(c, frames_of_source):
    g = np.float32(c.gain)
    if c.flags != 0 or not np.isfinite(g):
        return "flags or gain"
    if c.fade_in_curve not in CURVES or c.fade_out_curve not in CURVES:
        return "curve"
    if c.fade_in_frames > MAX_FADE or c.fade_out_frames > MAX_FADE or c.fade_in_frames > c.frames or c.fade_out_frames > c.frames:
        return "fade"
    if c.src_first + c.frames > frames_of_source:
        return "source range"
    if c.dst_first + c.frames > MAX_POSITION:
        return "position"
    return None


def extent(clips, frames_in, n_out):
    """validates the table -> one past the last covered frame of every output stream"""
    out = [0] * n_out
    for k, c in enumerate(clips):
        if c.src_stream >= len(frames_in) or c.dst_stream >= n_out:
            raise Invalid("stream index")
        why = clip_refusal(c, frames_in[c.src_stream])
        if why:
            raise Invalid(why)
        if k and (clips[k - 1].dst_stream, clips[k - 1].dst_first) > (c.dst_stream, c.dst_first):
            raise Invalid("order")
    # depth: brute force over the clips of an output that start at or before this one
    for k, c in enumerate(clips):
        if c.frames == 0:
            continue
        over = [p for p in clips[:k] if p.dst_stream == c.dst_stream and p.frames and p.dst_first + p.frames > c.dst_first]
        if len(over) >= 2:
            raise Invalid("depth")
        out[c.dst_stream] = max(out[c.dst_stream], c.dst_first + c.frames)
    return out


def trim(record, rule, src_stream=0, dst_stream=0):
    """-> (Clip, frames of the output) from a record with frames, leading_silence, trailing_silence"""
    n, lead, trail = int(record["frames"]), int(record["leading_silence"]), int(record["trailing_silence"])
    if rule.flags != 0 or rule.fade_in_curve not in CURVES or rule.fade_out_curve not in CURVES:
        raise Invalid("rule")
    if rule.fade_in_frames > MAX_FADE or rule.fade_out_frames > MAX_FADE:
        raise Invalid("fade")
    if n > 2 ** 32 - 1 or lead > n or trail > n or (lead < n and lead + trail > n):
        raise Invalid("record")
    c = Clip(src_stream=src_stream, dst_stream=dst_stream, dst_first=rule.pad_head, fade_in_curve=rule.fade_in_curve,
             fade_out_curve=rule.fade_out_curve, gain=1.0)
    if lead < n:
        c.src_first = lead - min(rule.keep_head, lead)
        c.frames = n - c.src_first - (trail - min(rule.keep_tail, trail))
        c.fade_in_frames = min(rule.fade_in_frames, c.frames)
        c.fade_out_frames = min(rule.fade_out_frames, c.frames)
    total = rule.pad_head + c.frames + rule.pad_tail
    if total > MAX_POSITION:
        raise Invalid("position")
    return c, total


# ---------------------------------------------------------------- rendering
def power_to_db(power, floor):
    power = np.float32(power)
    with np.errstate(all="ignore"):
        return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


def weights(c, j, tabs):
    """-> (w f32, faded bool) of clip c at its local frames j (uint64 array)"""
    j = np.asarray(j, np.uint64)
    w = np.full(j.shape, np.float32(c.gain), np.float32)
    faded = np.zeros(j.shape, bool)
    m = j < np.uint64(c.fade_in_frames)
    if m.any():
        w[m] = (w[m] * gain(tabs[c.fade_in_curve], c.fade_in_frames, j[m])).astype(np.float32)
        faded |= m
    back = np.uint64(c.frames - 1) - j
    m = back < np.uint64(c.fade_out_frames)
    if m.any():
        w[m] = (w[m] * gain(tabs[c.fade_out_curve], c.fade_out_frames, back[m])).astype(np.float32)
        faded |= m
    return w, faded


def render_window(inputs, clips, dst_stream, out_first, out_frames, channels, tabs, floor=-99.9):
    """inputs[s]: f32 [frames][channels] of input stream s.  -> (f32 [out_frames][channels], the record as a RECORD_DTYPE scalar) of
    output frames [out_first, out_first + out_frames) of one output stream"""
    y = np.zeros((out_frames, channels), np.float32)
    cover = np.zeros(out_frames, np.int64)
    any_fade = np.zeros(out_frames, bool)
    touching = 0
    last = out_first + out_frames
    for c in clips:
        if c.dst_stream != dst_stream or c.frames == 0:
            continue
        lo, hi = max(out_first, c.dst_first), min(last, c.dst_first + c.frames)
        if lo >= hi:
            continue
        touching += 1
        j = np.arange(lo - c.dst_first, hi - c.dst_first, dtype=np.uint64)
        w, faded = weights(c, j, tabs)
        x = np.asarray(inputs[c.src_stream], np.float32)[c.src_first + (lo - c.dst_first):c.src_first + (hi - c.dst_first)]
        with np.errstate(all="ignore"):
            part = (w[:, None] * x).astype(np.float32)
        if np.float32(c.gain) == np.float32(1.0):      # the copy rule: the bits of the source where no fade applies
            part.view(np.uint32)[~faded] = x.view(np.uint32)[~faded]
        at = slice(lo - out_first, hi - out_first)
        first = cover[at] == 0
        assert (cover[at] <= 1).all(), "a third clip over an output frame"
        seg = y[at]
        with np.errstate(all="ignore"):
            summed = (seg + part).astype(np.float32)
        seg.view(np.uint32)[first] = part.view(np.uint32)[first]
        seg.view(np.uint32)[~first] = summed.view(np.uint32)[~first]
        cover[at] += 1
        any_fade[at] |= faded
    rec = np.zeros((), RECORD_DTYPE)
    rec["out_first"], rec["frames"], rec["clips"] = out_first, out_frames, touching
    rec["silent_frames"], rec["faded_frames"], rec["mixed_frames"] = (cover == 0).sum(), any_fade.sum(), (cover == 2).sum()
    mag = np.abs(y)
    finite_or_inf = mag[~np.isnan(mag)]      # (taken out by hand: a maximum that ignores NaN is not trusted with signalling ones)
    peak = np.float32(finite_or_inf.max()) if finite_or_inf.size else np.float32(0)
    with np.errstate(all="ignore"):
        rec["samples_over"] = int((mag > np.float32(1.0)).sum())
        rec["out_sample_peak"] = peak
        rec["out_sample_peak_db"] = power_to_db(peak * peak, floor)
    return y, rec


def render(inputs, clips, out_frames, channels, tabs, out_first=None, floor=-99.9):
    """every output stream of a call -> (list of f32 [out_frames[o]][channels], list of records)"""
    extent(clips, [len(x) for x in inputs], len(out_frames))
    ys, recs = [], []
    for o, n in enumerate(out_frames):
        y, r = render_window(inputs, clips, o, out_first[o] if out_first is not None else 0, n, channels, tabs, floor)
        ys.append(y)
        recs.append(r)
    return ys, recs


def check_record(got, want, tag, bar=1e-4):
    """every field equal, out_sample_peak_db within the family's 1e-4 dB"""
    for f in EXACT_FIELDS:
        if f == "out_sample_peak":
            assert np.float32(got[f]).tobytes() == np.float32(want[f]).tobytes(), (tag, f, got[f], want[f])
        else:
            assert int(got[f]) == int(want[f]), (tag, f, got[f], want[f])
    g, w = float(got["out_sample_peak_db"]), float(want["out_sample_peak_db"])
    assert g == w or abs(g - w) <= bar, (tag, "out_sample_peak_db", g, w)      # (an infinite peak has an infinite level on both sides)


def noise(seed, frames, channels, scale=0.9):
    rng = np.random.default_rng(seed)
    return ((rng.random((frames, channels), dtype=np.float32) * np.float32(2) - np.float32(1)) * np.float32(scale)).astype(np.float32)

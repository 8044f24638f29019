"""numpy restatement of the programme bank's mix pass (include/omx/program_mix.h, DEFINITION): the f64 accumulator that takes the
exact product of every covering send in table order, the single rounding to f32, the zero fill, windows, the record, extent, plan-free
depth and the null-test table.  Frame by frame in numpy arrays: no spans, no tiles, no batches, nothing of how the library walks a
table.

numpy's float64 product of two float32 values is exact (24 x 24 bits in 53), its float64 sum rounds once to nearest even, and its
float64 -> float32 cast rounds to nearest even and produces denormals: the three operations of the DEFINITION."""
from dataclasses import dataclass

import numpy as np

MAX_LAYERS = 64
MAX_SENDS = 1 << 20
MAX_POSITION = 1 << 40
RECORD_DTYPE = np.dtype([("out_first", "<u8"), ("frames", "<u8"), ("silent_frames", "<u8"), ("mixed_frames", "<u8"), ("samples_over", "<u8"),
                         ("samples_nonfinite", "<u8"), ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("sends", "<u4"),
                         ("max_layers", "<u4")])
EXACT_FIELDS = tuple(f for f in RECORD_DTYPE.names if f != "out_sample_peak_db")
COUNT_FIELDS = ("frames", "silent_frames", "mixed_frames", "samples_over", "samples_nonfinite")


class Invalid(ValueError):
    pass


@dataclass
class Send:
    src_stream: int = 0
    dst_bus: int = 0
    src_first: int = 0
    dst_first: int = 0
    frames: int = 0
    gain: float = 1.0
    flags: int = 0


# ---------------------------------------------------------------- tables
def send_refusal(s, frames_of_source):
    if s.flags != 0 or not np.isfinite(np.float32(s.gain)):
        return "flags or gain"
    if s.src_first + s.frames > frames_of_source:
        return "source range"
    if s.dst_first + s.frames > MAX_POSITION:
        return "position"
    return None


def extent(sends, frames_in, n_out):
    """validates the table -> one past the last covered frame of every bus"""
    if len(sends) > MAX_SENDS:
        raise Invalid("sends")
    out = [0] * n_out
    for k, s in enumerate(sends):
        if s.src_stream >= len(frames_in) or s.dst_bus >= n_out:
            raise Invalid("stream index")
        why = send_refusal(s, frames_in[s.src_stream])
        if why:
            raise Invalid(why)
        if k and (sends[k - 1].dst_bus, sends[k - 1].dst_first) > (s.dst_bus, s.dst_first):
            raise Invalid("order")
    # depth: brute force over the earlier sends of the bus that still cover this one's first frame
    for k, s in enumerate(sends):
        if s.frames == 0:
            continue
        over = [p for p in sends[:k] if p.dst_bus == s.dst_bus and p.frames and p.dst_first + p.frames > s.dst_first]
        if len(over) >= MAX_LAYERS:
            raise Invalid("depth")
        out[s.dst_bus] = max(out[s.dst_bus], s.dst_first + s.frames)
    return out


def null_table(stems, reference_stream, frames, bus=0):
    if not 1 <= len(stems) <= MAX_LAYERS - 1 or frames > MAX_POSITION:
        raise Invalid("null")
    return [Send(s, bus, 0, 0, frames, 1.0) for s in stems] + [Send(reference_stream, bus, 0, 0, frames, -1.0)]


# ---------------------------------------------------------------- rendering
def power_to_db(power, floor):
    power = np.float32(power)
    with np.errstate(all="ignore"):
        return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


def render_window(inputs, sends, bus, out_first, out_frames, channels, floor=-99.9):
    """inputs[s]: f32 [frames][channels] of input stream s.  -> (f32 [out_frames][channels], the record as a RECORD_DTYPE scalar) of
    bus frames [out_first, out_first + out_frames) of one bus"""
    acc = np.zeros((out_frames, channels), np.float64)
    cover = np.zeros(out_frames, np.int64)
    touching = 0
    last = out_first + out_frames
    for s in sends:      # in table order
        if s.dst_bus != bus or s.frames == 0:
            continue
        lo, hi = max(out_first, s.dst_first), min(last, s.dst_first + s.frames)
        if lo >= hi:
            continue
        touching += 1
        x = np.asarray(inputs[s.src_stream], np.float32)[s.src_first + (lo - s.dst_first):s.src_first + (hi - s.dst_first)]
        at = slice(lo - out_first, hi - out_first)
        with np.errstate(all="ignore"):
            prod = np.float64(np.float32(s.gain)) * x.astype(np.float64)      # exact
            summed = acc[at] + prod                                            # one rounding to f64
        first = cover[at] == 0
        seg = acc[at]
        seg[first] = prod[first]
        seg[~first] = summed[~first]
        cover[at] += 1
    assert (cover <= MAX_LAYERS).all(), "a 65th send over a bus frame"
    with np.errstate(all="ignore"):
        y = acc.astype(np.float32)                                             # one rounding to f32, nearest even, denormals kept
    y[cover == 0] = np.float32(0.0)
    rec = np.zeros((), RECORD_DTYPE)
    rec["out_first"], rec["frames"], rec["sends"] = out_first, out_frames, touching
    rec["silent_frames"], rec["mixed_frames"] = (cover == 0).sum(), (cover >= 2).sum()
    rec["max_layers"] = int(cover.max()) if out_frames else 0
    mag = np.abs(y)
    finite_or_inf = mag[~np.isnan(mag)]      # (taken out by hand: a maximum that ignores NaN is not trusted with signalling ones)
    peak = np.float32(finite_or_inf.max()) if finite_or_inf.size else np.float32(0)
    with np.errstate(all="ignore"):
        rec["samples_over"] = int((mag > np.float32(1.0)).sum())
        rec["samples_nonfinite"] = int((~np.isfinite(y)).sum())
        rec["out_sample_peak"] = peak
        rec["out_sample_peak_db"] = power_to_db(peak * peak, floor)
    return y, rec


def render(inputs, sends, out_frames, channels, out_first=None, floor=-99.9):
    """every bus of a call -> (list of f32 [out_frames[o]][channels], list of records)"""
    extent(sends, [len(x) for x in inputs], len(out_frames))
    ys, recs = [], []
    for o, n in enumerate(out_frames):
        y, r = render_window(inputs, sends, o, out_first[o] if out_first is not None else 0, n, channels, floor)
        ys.append(y)
        recs.append(r)
    return ys, recs


def same_bytes_nan_as_nan(got, want):
    """equal on bytes, except that a NaN of one may sit where a NaN of the other does (the bits of a NaN are not defined)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all() and (got.view(np.uint32)[~gn] == want.view(np.uint32)[~wn]).all())


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


def lattice(seed, frames, channels, n_stems):
    """n_stems stems on a 2^-16 lattice inside +-0.25, and their sum (the printmaster): every partial sum is exact in f32 and f64"""
    rng = np.random.default_rng(seed)
    stems = [(rng.integers(-16384, 16385, (frames, channels)).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
             for _ in range(n_stems)]
    total = np.sum(np.stack(stems).astype(np.float64), axis=0).astype(np.float32)
    return stems, total

"""numpy restatement of the programme bank's channel remix, written from the DEFINITION in include/omx/program_remix.h and from nothing
else: the mix, the two preset builders (the BS.775-style fold-down and the select matrix) and the record.  Every operation is one f32
operation of numpy, in the header's order: a product is rounded before it is added, a zero coefficient is skipped (its input never
enters the arithmetic), the first term of a row is a product and not a sum with zero."""
import numpy as np

POS_FL, POS_FR, POS_FC, POS_LFE, POS_RL, POS_RR, POS_SL, POS_SR, POS_MONO, POS_UNKNOWN, POS_AUX0 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16
KIND_STEREO, KIND_MONO = 0, 1
NORMALIZE = 1
DEFAULT_CENTER = DEFAULT_SURROUND = np.float32(0.70710678)
DEFAULT_LFE = np.float32(0.0)
MAX_MATRICES = 65536
RECORD_FIELDS = ("frames", "samples_over", "out_sample_peak", "out_sample_peak_db", "matrix_index", "terms")
EXACT_FIELDS = tuple(f for f in RECORD_FIELDS if f != "out_sample_peak_db")


class Invalid(ValueError):
    """OMX_ERR_INVALID"""


def _channels_ok(c):
    return 1 <= c <= 8


# ---------------------------------------------------------------- the mix
def remix(matrix, x):
    """f32 [frames][channels_in] under f32 [channels_out][channels_in] -> f32 [frames][channels_out]"""
    m = np.asarray(matrix, np.float32)
    x = np.asarray(x, np.float32).reshape(-1, m.shape[1])
    out = np.zeros((len(x), m.shape[0]), np.float32)      # a row without a non-zero coefficient: +0.0f
    with np.errstate(all="ignore"):
        for o in range(m.shape[0]):
            acc = None
            for i in range(m.shape[1]):
                if m[o, i] == 0:      # either sign: skipped
                    continue
                prod = m[o, i] * x[:, i]      # f32 * f32 -> f32
                acc = prod if acc is None else acc + prod
            if acc is not None:
                out[:, o] = acc
    return out


def terms(matrix):
    return int((np.asarray(matrix, np.float32) != 0).sum())


def power_to_db(power, floor):
    power = np.float32(power)
    return max(float(np.float32(np.log(power)) * np.float32(4.3429448)), floor) if power > 0 else floor


def record(out, matrix, matrix_index=0, floor=-99.9):
    """the record of one call that wrote `out` for a stream"""
    mag = np.abs(np.asarray(out, np.float32))
    peak = np.float32(0)
    if mag.size and not np.isnan(mag).all():
        peak = max(peak, np.float32(np.nanmax(mag)))
    with np.errstate(all="ignore"):
        return {"frames": len(out), "samples_over": int((mag > np.float32(1.0)).sum()), "out_sample_peak": peak,
                "out_sample_peak_db": power_to_db(peak * peak, floor), "matrix_index": matrix_index, "terms": terms(matrix)}


def check_record(got, want, tag, bar=1e-4):
    for f in EXACT_FIELDS:
        if f == "out_sample_peak":
            assert np.float32(got[f]).tobytes() == np.float32(want[f]).tobytes(), (tag, f, got[f], want[f])
        else:
            assert int(got[f]) == int(want[f]), (tag, f, got[f], want[f])
    g, w = float(got["out_sample_peak_db"]), float(want["out_sample_peak_db"])
    assert g == w or abs(g - w) <= bar, (tag, g, w)      # (an infinite peak has an infinite level on both sides)


# ---------------------------------------------------------------- the presets
def _level_ok(v):
    v = np.float32(v)
    return bool(np.isfinite(v)) and 0.0 <= float(v) <= 2.0


def downmix(channels_in, positions_in, kind=KIND_STEREO, center=DEFAULT_CENTER, surround=DEFAULT_SURROUND, lfe=DEFAULT_LFE, flags=0):
    """-> (matrix f32 [channels_out][channels_in], positions_out: 8 entries)"""
    if not _channels_ok(channels_in) or kind not in (KIND_STEREO, KIND_MONO) or flags & ~NORMALIZE:
        raise Invalid("channels_in, kind or flags")
    if not (_level_ok(center) and _level_ok(surround) and _level_ok(lfe)):
        raise Invalid("a level")
    c, s, l, one, zero = np.float32(center), np.float32(surround), np.float32(lfe), np.float32(1), np.float32(0)
    pairs = {POS_FL: (one, zero), POS_FR: (zero, one), POS_FC: (c, c), POS_MONO: (c, c), POS_LFE: (l, l), POS_RL: (s, zero), POS_SL: (s, zero),
             POS_RR: (zero, s), POS_SR: (zero, s)}
    wl = np.array([pairs.get(int(p), (zero, zero))[0] for p in positions_in[:channels_in]], np.float32)
    wr = np.array([pairs.get(int(p), (zero, zero))[1] for p in positions_in[:channels_in]], np.float32)
    if flags & NORMALIZE:
        sl = sr = np.float32(0)
        for i in range(channels_in):
            sl = np.float32(sl + np.abs(wl[i]))
        for i in range(channels_in):
            sr = np.float32(sr + np.abs(wr[i]))
        n = max(sl, sr)
        if n > np.float32(1):
            wl, wr = (wl / n).astype(np.float32), (wr / n).astype(np.float32)
    if kind == KIND_STEREO:
        return np.stack([wl, wr]), [POS_FL, POS_FR] + [POS_UNKNOWN] * 6
    return (np.float32(0.5) * (wl + wr).astype(np.float32)).astype(np.float32)[None], [POS_MONO] + [POS_UNKNOWN] * 7


def select(channels_in, positions_in, channels_out, positions_out):
    """-> (matrix f32 [channels_out][channels_in], the mask of the outputs without a source)"""
    if not _channels_ok(channels_in) or not _channels_ok(channels_out):
        raise Invalid("a channel count")
    m, missing = np.zeros((channels_out, channels_in), np.float32), 0
    for o in range(channels_out):
        for i in range(channels_in):
            if int(positions_in[i]) == int(positions_out[o]):
                m[o, i] = 1.0
                break
        else:
            missing |= 1 << o
    return m, missing


# ---------------------------------------------------------------- inputs of the tests
def noise(seed, frames, channels, amplitude=1.0):
    return (np.random.default_rng(seed).uniform(-amplitude, amplitude, (frames, channels))).astype(np.float32)


def dense(seed, channels_in, channels_out):
    """a matrix of the pair with a few exact zeros of either sign in it"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (channels_out, channels_in)).astype(np.float32)
    zero = rng.random((channels_out, channels_in)) < 0.25
    m[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return m

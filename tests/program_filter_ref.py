"""numpy restatement of include/omx/program_filter.h: the DEFINITION block line by line (a loop over time, vectorised over the
(stream, channel) lanes: elementwise f64 numpy operations round like the scalar code, so the bits match), the design formulas, the
record, and a model of the time-parallel schedule (work items, f64 dot products for the zero-state end states, a double-double scan
of the zero-input transition, the items again from their start states) that says what that form may differ by."""
import math

import numpy as np

MAX_SECTIONS = 2
MAX_FILTERS = 256
BYPASS = 0xFFFFFFFF
HIGHPASS, LOWPASS, LOW_SHELF, HIGH_SHELF, PEAKING, NOTCH, DC_BLOCK, DEEMPHASIS, PREEMPHASIS = range(9)
CHUNK_FRAMES = 1024
TILE_FRAMES = 32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)

RECORD_DTYPE = np.dtype([("frames", "<u8"), ("frames_total", "<u8"), ("samples_over", "<u8"), ("samples_nonfinite", "<u8"),
                         ("out_sample_peak", "<f4"), ("out_sample_peak_db", "<f4"), ("form", "<u4"), ("_pad", "<u4")])


# ---- design formulas (sections are tuples (b0, b1, b2, a1, a2), a0 = 1)
def _rbj(b0, b1, b2, a0, a1, a2):
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def _pass2(high, w0, q):
    cs, al = math.cos(w0), math.sin(w0) / (2.0 * q)
    if high:
        return _rbj((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0, 1.0 + al, -2.0 * cs, 1.0 - al)
    return _rbj((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0, 1.0 + al, -2.0 * cs, 1.0 - al)


def design(kind, fs, frequency_hz=0.0, order=0, q=0.0, gain_db=0.0, time_constant_us=0.0, time_constant_zero_us=0.0):
    """The sections of a spec at the sample rate fs: a list of one or two (b0, b1, b2, a1, a2)."""
    f = frequency_hz
    qq = 1.0 / math.sqrt(2.0) if q == 0.0 else q
    w0 = 2.0 * math.pi * f / fs
    cs, al = math.cos(w0), math.sin(w0) / (2.0 * qq)
    if kind in (HIGHPASS, LOWPASS):
        high = kind == HIGHPASS
        if order == 1:
            K = math.tan(math.pi * f / fs)
            if high:
                return [(1.0 / (1.0 + K), -(1.0 / (1.0 + K)), 0.0, (K - 1.0) / (K + 1.0), 0.0)]
            return [(K / (1.0 + K), K / (1.0 + K), 0.0, (K - 1.0) / (K + 1.0), 0.0)]
        if order == 2:
            return [_pass2(high, w0, qq)]
        assert order == 4
        return [_pass2(high, w0, 1.0 / math.sqrt(2.0 + math.sqrt(2.0))), _pass2(high, w0, 1.0 / math.sqrt(2.0 - math.sqrt(2.0)))]
    if kind in (LOW_SHELF, HIGH_SHELF):
        A = math.pow(10.0, gain_db / 40.0)
        r = 2.0 * math.sqrt(A) * al
        if kind == LOW_SHELF:
            return [_rbj(A * ((A + 1.0) - (A - 1.0) * cs + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - r),
                         (A + 1.0) + (A - 1.0) * cs + r, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - r)]
        return [_rbj(A * ((A + 1.0) + (A - 1.0) * cs + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - r),
                     (A + 1.0) - (A - 1.0) * cs + r, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - r)]
    if kind == PEAKING:
        A = math.pow(10.0, gain_db / 40.0)
        return [_rbj(1.0 + al * A, -2.0 * cs, 1.0 - al * A, 1.0 + al / A, -2.0 * cs, 1.0 - al / A)]
    if kind == NOTCH:
        return [_rbj(1.0, -2.0 * cs, 1.0, 1.0 + al, -2.0 * cs, 1.0 - al)]
    if kind == DC_BLOCK:
        return [(1.0, -1.0, 0.0, -(1.0 - w0), 0.0)]
    k1, k2 = 2.0 * fs * (time_constant_us * 1.0e-6), 2.0 * fs * (time_constant_zero_us * 1.0e-6)
    if kind == DEEMPHASIS:
        return [((1.0 + k2) / (1.0 + k1), (1.0 - k2) / (1.0 + k1), 0.0, (1.0 - k1) / (1.0 + k1), 0.0)]
    assert kind == PREEMPHASIS
    return [((1.0 + k1) / (1.0 + k2), (1.0 - k1) / (1.0 + k2), 0.0, (1.0 - k2) / (1.0 + k2), 0.0)]


def stable(section):
    _, _, _, a1, a2 = section
    return abs(a2) < 1.0 and abs(a1) < 1.0 + a2


def response(sections, fs, hz):
    """H(e^{jw}) of a cascade as a complex number."""
    z = np.exp(-2j * np.pi * hz / fs)
    h = 1.0 + 0.0j
    for b0, b1, b2, a1, a2 in sections:
        h *= (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return h


# ---- the definition
def lane_table(filters, filter_of_channel, n_streams, channels):
    """Per (stream, channel) lane: coefficient array [2][5][lanes] f64, section counts [lanes], bypass mask [lanes].
    filters: list of section lists; filter_of_channel: [n_streams][channels] of indices or BYPASS, None: filter 0 everywhere."""
    idx = np.zeros((n_streams, channels), np.int64) if filter_of_channel is None else np.asarray(filter_of_channel, np.int64).reshape(n_streams, channels)
    lanes = n_streams * channels
    coef = np.zeros((2, 5, lanes))
    coef[:, 0, :] = 1.0
    count = np.ones(lanes, np.int64)
    bypass = idx.reshape(-1) == BYPASS
    for lane, i in enumerate(idx.reshape(-1)):
        if i == BYPASS:
            continue
        secs = filters[i]
        count[lane] = len(secs)
        for k, sec in enumerate(secs):
            coef[k, :, lane] = sec
    return coef, count, bypass


def run(x, coef, count, bypass, state=None, unrounded=None):
    """x: f32 [frames][lanes].  Returns (out f32 [frames][lanes], state f64 [4][lanes]); `state` carries on from an earlier call.
    unrounded: an f64 [frames][lanes] array that takes v before it is rounded to f32 (for the model's comparison)."""
    x = np.asarray(x, np.float32)
    n, lanes = x.shape
    st = np.zeros((4, lanes)) if state is None else np.array(state, np.float64)
    out = np.empty_like(x)
    two = count == 2
    with np.errstate(all="ignore"):
        for i in range(n):
            v = x[i].astype(np.float64)
            for k in range(2):
                b0, b1, b2, a1, a2 = coef[k]
                s1, s2 = st[2 * k], st[2 * k + 1]
                y = b0 * v + s1
                n1 = (b1 * v - a1 * y) + s2
                n2 = b2 * v - a2 * y
                if k == 0:
                    st[0], st[1] = n1, n2
                    v = y
                else:  # a lane of one section has no second one: neither its output nor its state moves
                    st[2], st[3] = np.where(two, n1, s1), np.where(two, n2, s2)
                    v = np.where(two, y, v)
            out[i] = v.astype(np.float32)
            if unrounded is not None:
                unrounded[i] = v
    bits = out.view(np.uint32)
    bits[:, bypass] = x.view(np.uint32)[:, bypass]
    st[:, bypass] = 0.0 if state is None else np.asarray(state)[:, bypass]
    return out, st


def power_to_db(power, floor):  # level.rs:28-34 in f32, as the kernels' power_to_db
    power = np.float32(power)
    if not power > 0:
        return np.float32(floor)
    return max(np.float32(np.log(power, dtype=np.float32) * np.float32(4.3429448)), np.float32(floor))


def record(out, frames_total, form, floor_db):
    """The record of one stream's call from its output out: f32 [frames][channels]."""
    out = np.asarray(out, np.float32)
    r = np.zeros((), RECORD_DTYPE)
    mag = np.abs(out)
    r["frames"] = out.shape[0]
    r["frames_total"] = frames_total
    r["samples_over"] = int(np.count_nonzero(mag > np.float32(1.0)))
    r["samples_nonfinite"] = int(np.count_nonzero(~np.isfinite(out)))
    finite = mag[~np.isnan(mag)]
    peak = np.float32(finite.max()) if finite.size else np.float32(0.0)
    r["out_sample_peak"] = peak
    with np.errstate(all="ignore"):
        r["out_sample_peak_db"] = power_to_db(peak * peak, floor_db)
    r["form"] = form if out.shape[0] else 0
    return r


# ---- double-double scalars for the tables of the time-parallel form (Dekker / Knuth, no fma needed)
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a
    h = t - (t - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(a, b):
    sh, sl = _two_sum(a[0], b[0])
    th, tl = _two_sum(a[1], b[1])
    sl += th
    sh, sl = sh + sl, sl - ((sh + sl) - sh)
    sl += tl
    return sh + sl, sl - ((sh + sl) - sh)


def _dd_mul_d(a, b):
    p, e = _two_prod(a[0], b)
    e += a[1] * b
    return p + e, e - ((p + e) - p)


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    e += a[0] * b[1] + a[1] * b[0]
    return p + e, e - ((p + e) - p)


def _dd_step(f, x, secs):
    v = x
    for k in range(2):
        b0, b1, b2, a1, a2 = secs[k]
        y = _dd_add(_dd_mul_d(v, b0), f[2 * k])
        f[2 * k] = _dd_add(_dd_add(_dd_mul_d(v, b1), _dd_mul_d(y, -a1)), f[2 * k + 1])
        f[2 * k + 1] = _dd_add(_dd_mul_d(v, b2), _dd_mul_d(y, -a2))
        v = y
    return f


def tables(sections, L=CHUNK_FRAMES):
    """W [L][4] (f64: the weight of sample k of a work item on its zero-state end state), T [4][4] as (high, low) arrays, and the two
    figures of the rule: the largest |T| entry and the largest column sum of |W|."""
    secs = [tuple(sections[0]), tuple(sections[1]) if len(sections) == 2 else IDENTITY]
    W = np.zeros((L, 4))
    g = _dd_step([(0.0, 0.0)] * 4, (1.0, 0.0), secs)
    for n in range(L):
        W[L - 1 - n] = [g[i][0] for i in range(4)]
        g = _dd_step(g, (0.0, 0.0), secs)
    Th, Tl = np.zeros((4, 4)), np.zeros((4, 4))
    for m in range(4):
        f = [(1.0 if k == m else 0.0, 0.0) for k in range(4)]
        for n in range(L):
            f = _dd_step(f, (0.0, 0.0), secs)
        for k in range(4):
            Th[k, m], Tl[k, m] = f[k]
    return W, Th, Tl, float(np.abs(Th).max()), float(np.abs(W).sum(0).max())


def predicted_start_error(sections, L=CHUNK_FRAMES):
    """The rule's figure, per unit of input peak: every one of the L steps of an item rounds the state by 2^-53 of its size (at most
    the largest zero-state state of a full-scale item), and A^n (at most the largest |A^L| entry) carries it to the item's end."""
    _, _, _, largest, gain = tables(sections, L)
    return L * largest * gain * 2.0 ** -53


def time_parallel_ok(sections, L=CHUNK_FRAMES):
    return predicted_start_error(sections, L) <= 2.0 ** -25


def run_time_parallel(x, sections, state=None, L=CHUNK_FRAMES, unrounded=None):
    """The model of the time-parallel schedule for lanes that all run `sections`: x f32 [frames][lanes] ->
    (out f32 [frames][lanes], state f64 [4][lanes]); unrounded as in run()."""
    x = np.asarray(x, np.float32)
    n, lanes = x.shape
    W, Th, Tl, _, _ = tables(sections, L)
    items = (n + L - 1) // L
    start = np.zeros((max(items, 1), 4, lanes))
    if state is not None:
        start[0] = state
    full = max(items - 1, 0)  # (A) the full items that somebody starts behind
    z = np.zeros((full, 4, lanes))
    if full:
        xs = x[:full * L].astype(np.float64).reshape(full, L, lanes)
        for k in range(L):
            z += W[k][None, :, None] * xs[:, k][:, None, :]
    with np.errstate(all="ignore"):
        for lane in range(lanes):  # (B) the scan, a double-double pair per state
            st = [(float(start[0, i, lane]), 0.0) for i in range(4)]
            for j in range(full):
                nx = []
                for i in range(4):
                    acc = (float(z[j, i, lane]), 0.0)
                    for k in range(4):
                        acc = _dd_add(acc, _dd_mul((float(Th[i, k]), float(Tl[i, k])), st[k]))
                    nx.append(acc)
                st = nx
                start[j + 1, :, lane] = [v[0] for v in st]
    coef, count, bypass = lane_table([sections], None, 1, lanes)
    out = np.empty_like(x)
    last = np.zeros((4, lanes)) if state is None else np.array(state, np.float64)
    for j in range(items):  # (C) the items again from their start states
        out[j * L:(j + 1) * L], last = run(x[j * L:(j + 1) * L], coef, count, bypass, start[j],
                                           None if unrounded is None else unrounded[j * L:(j + 1) * L])
    return out, last

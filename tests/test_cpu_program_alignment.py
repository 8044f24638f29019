"""The cases of tests/test_gpu_program_alignment.py (the programme bank's stages fed buffers at every 4-byte alignment) without a
device: case_of() builds a stage's inputs, capacities, call schedule and the restatement's expected outputs in numpy alone, and the GPU
file imports it.  Four things are tested here.

a. Every case is accepted by its restatement and in range: every call's emitted frame count is at most out_capacity - 1, and the calls
   of a carrying stage add up to the restatement's one-call output.
b. The coverage conditions hold, computed from (offset, capacity, channels, stream): over the 16 offset pairs and the five streams the
   input and the output row bases each reach all four residues {0, 4, 8, 12} mod 16 at every channel count (4 and 8 included, where
   only the base offset moves a row); at up to 3 channels the one-frame stream is shorter than a peel; the edit case has clips whose
   sources sit on the output's 16-byte phase and clips whose sources do not.
c. The comparison helper rejects what it is there for: a row's first float left at the sentinel, a row's last float written one place
   further, a guard float in front of d_out overwritten, a whole row shifted by one float; and it accepts the faultless image.
d. placed() puts the host array at the right index and leaves every pad float at the fill, whatever an earlier allocation of the same
   size held: a stale store cannot make (c) pass for the wrong reason."""
import os

import numpy as np
import pytest

import program_convolve_ref as cr
import program_dynamics_ref as dr
import program_edit_ref as er
import program_inspect_ref as ir
import program_limit_ref as lr
import program_loudness_ref as lref
import program_mix_ref as xr
import program_pcm_ref as pr
import program_peaks_ref as pk
import program_remix_ref as mr
import program_resample_ref as rr
from openmeters_amd import capi
from openmeters_amd.program_loudness import (DYNAMICS_FLUSHED, ResampleRule, convolve_frames, convolve_plan, dynamics_frames, edit_plan, filter_plan, inspect_plan,
                                             mix_plan, remix_plan, resample_frames, resample_plan)
from test_cpu_program_resample import lib_plan
from test_gpu_program_dynamics import bursts, compressor, step_over, tiles
from test_gpu_program_edit import tabs_of
from test_gpu_program_filter import filter_table_for, per_channel, restate as filter_restate
from test_gpu_program_filter import noise as filter_noise
from test_gpu_program_inspect import pairs_of
from test_gpu_program_loudness import FLOOR

FS = 48000.0
SENTINEL = np.float32(777.25)
SENTINEL_BYTE = 0xA5
PAD_BYTES = 32                      # 8 floats of slack per store
OFFSETS = (0, 1, 2, 3)              # floats; a uint8 store moves by 4 * offset bytes
PAIRS = [(a_in, a_out) for a_in in OFFSETS for a_out in OFFSETS]
N = 5
CHANNELS = {"resample": (1, 2, 3, 4, 8), "convolve": (1, 2, 3, 4, 6, 8), "dynamics": (1, 2, 3, 4, 6, 8), "limiter": (1, 2, 3, 4, 8),
            "remix": (6, 1, 4), "inspect": (1, 2, 3, 4, 6, 8), "filter": (1, 2, 3, 4, 6, 8), "edit": (1, 2, 3, 4, 6, 8),
            "mix": (1, 2, 3, 4, 6, 8), "import_pcm": (1, 2, 3, 4, 8), "export_pcm": (1, 2, 3, 4, 8), "apply_gains": (1, 2, 3, 4, 8),
            "process": (3,)}
REMIX_OUT = {6: 2, 1: 2, 4: 4}      # one matrix down, one up, one square
RESAMPLE_RATES = ((44100, 48000), (48000, 44100))
APPLY_TILE_FLOATS = 4096            # kPnTileFloats (program_normalize.hpp): apply_gains has no plan call to ask
LIMIT_RULE = (lr.CEILING_DB, 16, 100)
LIMIT_FACTORS = [2.0, 1.5, -2.0, 2.0, 1.75]
PROCESS_RATE = 8000.0
PROCESS_SEEDS = (0, 1, 3, 4, 5)


# ================================================================ shapes and placement
def lengths_of(t):
    """the five streams of a case: none, one frame (fewer floats than a peel at up to 3 channels), one frame either side of a tile, and
    two tiles and a ragged rest"""
    return [0, 1, t - 1, t + 1, 2 * t + 3]


def odd_above(frames):
    """a capacity of at least frames + 1, odd: rows of 3 channels then start at every residue on their own"""
    return (frames + 1) | 1


def pair_of_call(k, a_in, a_out):
    """the offsets of call k of a carrying stage: the carried state must not remember an alignment"""
    return [(a_in, a_out), ((a_in + 1) % 4, (a_out + 3) % 4), ((a_in + 2) % 4, (a_out + 2) % 4)][k]


def hard_edges(x):
    """NaN, both infinities, denormals and -0.0 into the first four and the last four floats: the floats a head peel and a tail move
    apart from the body.  The NaN with a payload is a QUIET one: the restatements' maxima (np.fmax in program_dynamics_ref.level) hand a
    signalling NaN on where the definition and the device's fmaxf ignore it, so a signalling one beside an infinity would test numpy"""
    x = np.array(x, np.float32)
    flat = x.reshape(-1)
    assert flat.size >= 8
    head = np.array([np.nan, np.inf, 1e-40, -0.0], np.float32)
    tail = np.array([-np.inf, -0.0, -3e-42, np.nan], np.float32)
    tail.view(np.uint32)[3] = 0x7FC12345
    flat[:4], flat[-4:] = head, tail
    return x


def rows_of(xs, cap, ch, seed):
    """[n][cap][ch]: stream s's frames at the head of row s, other seeded samples behind them"""
    host = np.random.default_rng([seed, 77]).uniform(-0.9, 0.9, (len(xs), cap, ch)).astype(np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    return host


def pad_of(dtype):
    return PAD_BYTES // np.dtype(dtype).itemsize


def input_fill(host, seed=5):
    """what an input store holds around the rows: seeded noise (bytes for an integer store)"""
    host = np.asarray(host)
    rng = np.random.default_rng([seed, host.size])
    if host.dtype == np.uint8:
        return rng.integers(0, 256, host.size + pad_of(np.uint8), dtype=np.uint8)
    return rng.uniform(-0.9, 0.9, host.size + pad_of(np.float32)).astype(np.float32)


def store_image(host, offset, fill):
    """host (flattened) at index `offset` of a store of host.size + 8 floats (32 bytes) that holds `fill` (a value, or an array of the
    store's size) everywhere else"""
    host = np.ascontiguousarray(host).reshape(-1)
    store = np.empty(host.size + pad_of(host.dtype), host.dtype)
    store[:] = fill
    store[offset:offset + host.size] = host
    return store


def placed(torch, host, offset, fill, device="cuda"):
    """-> (the store, the pointer to host's first element inside it).  offset: elements of host's type, so 0 .. 3 floats, or 0, 4, 8, 12
    bytes of a uint8 store"""
    image = store_image(host, offset, fill)
    store = torch.from_numpy(image).to(device)
    assert store.data_ptr() % 16 == 0
    assert 0 <= offset and offset + np.asarray(host).size <= image.size
    return store, store.data_ptr() + offset * image.itemsize


# ================================================================ the comparison
def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def expected_image(before, wants, offset, row_units):
    """what a faultless device leaves of the store `before`: stream s's output at the head of row s, everything else untouched"""
    image = before.copy()
    for s, w in enumerate(wants):
        w = np.ascontiguousarray(w).reshape(-1)
        assert w.size <= row_units and w.dtype == before.dtype, (s, w.size, row_units, w.dtype)
        image[offset + s * row_units:offset + s * row_units + w.size] = w
    return image


def rows_of_image(got, offset, row_units, counts):
    """the first counts[s] elements of every row as the device left them"""
    return [got[offset + s * row_units:offset + s * row_units + c].copy() for s, c in enumerate(counts)]


def check_image(got, before, wants, offset, row_units, tag, nan_as_nan=True):
    """got: the whole output store as the device left it.  Equal on bits to expected_image (with nan_as_nan, a NaN where the
    restatement has a NaN: the bits of a NaN the arithmetic produces are not defined).  So: every stream's output is the restatement's,
    the guard floats in front of d_out and behind the last row keep their fill, and so does every float of a row at or beyond the
    stream's frames"""
    want = expected_image(before, wants, offset, row_units)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    same = bits_of(got) == bits_of(want)
    if nan_as_nan and got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if same.all():
        return
    at = int(np.flatnonzero(~same)[0])
    near = (got[max(at - 2, 0):at + 4], want[max(at - 2, 0):at + 4])
    if at < offset:
        raise AssertionError((tag, "a guard element in front of d_out was written", at, near))
    if at >= offset + len(wants) * row_units:
        raise AssertionError((tag, "a guard element behind the last row was written", at - offset - len(wants) * row_units, near))
    s, i = divmod(at - offset, row_units)
    size = np.asarray(wants[s]).size
    what = "written at or beyond the stream's frames" if i >= size else "output differs from the restatement"
    raise AssertionError((tag, what, "stream", s, "element", i, "of", size, int((~same).sum()), "in all", near))


# ================================================================ the cases (numpy only)
_CASES = {}


def oracle_api():
    return capi.Api(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libomx_oracle.so"), "omxo_")


def case_of(stage, ch, omx):
    """-> the variants of a stage's case at one channel count (one, or one per rate pair / PCM format / key routing): dicts with
    ci, co         channels of d_in and d_out
    t              the stage's tile in frames, from its own plan
    xs             the five streams' inputs, f32 [frames][ci] (raw bytes per stream for import_pcm)
    cap, out_cap   frames_capacity and out_capacity, odd
    calls          the schedule: dicts with rows (each stream's frames of the call), emits (frames each stream writes), wants (the slice
                   of the one-call output the call writes), flush
    wants, records the restatement's one-call outputs and what its records hold at the end"""
    key = (stage, ch)
    if key not in _CASES:
        _CASES[key] = BUILDERS[stage](ch, omx)
    return _CASES[key]


def make_case(stage, ci, co, t, xs, wants, records, calls=None, **extra):
    cap = odd_above(max(len(x) for x in xs))
    out_cap = odd_above(max(len(w) for w in wants)) if wants is not None else 0
    if calls is None:      # one call that brings everything
        calls = [dict(rows=xs, emits=[len(w) for w in wants] if wants is not None else None, wants=wants, flush=False)]
    return dict(stage=stage, ci=ci, co=co, t=t, xs=xs, wants=wants, records=records, cap=cap, out_cap=out_cap, calls=calls,
                in_unit=4, out_unit=4, **extra)


def inputs_of(seed, lengths, ch, noise):
    xs = [noise(seed + s, f, ch) for s, f in enumerate(lengths)]
    xs[3] = hard_edges(xs[3])
    return xs


def carried_calls(xs, t, wants, frames_fn, has_flush, keys=None):
    """every stream in two calls cut at t + 1 frames, then (where the stage has one) the flush in a call that brings nothing.
    frames_fn(stream, frames taken before, frames emitted before, frames, flush) -> the frames the call emits"""
    n = len(xs)
    first = [min(len(x), t + 1) for x in xs]
    plan = [([0] * n, first, False), (first, [len(x) for x in xs], False)]
    if has_flush:
        plan.append(([len(x) for x in xs], [len(x) for x in xs], True))
    taken, emitted, calls = [0] * n, [0] * n, []
    for lo, hi, flush in plan:
        emits = [int(frames_fn(s, taken[s], emitted[s], hi[s] - lo[s], flush)) for s in range(n)]
        call = dict(rows=[x[a:b] for x, a, b in zip(xs, lo, hi)], emits=emits, flush=flush,
                    wants=[w[e:e + k] for w, e, k in zip(wants, emitted, emits)])
        if keys is not None:
            call["keys"] = [x[a:b] for x, a, b in zip(keys, lo, hi)]
        calls.append(call)
        taken, emitted = list(hi), [e + k for e, k in zip(emitted, emits)]
    return calls


def build_remix(ci, omx):
    co = REMIX_OUT[ci]
    t = int(remix_plan(omx, ci, co)["tile_frames"])
    matrix = np.float32(3.0) * mr.dense(1000 + 10 * ci + co, ci, co)
    xs = inputs_of(100 * ci + 10 * co, lengths_of(t), ci, mr.noise)
    wants = [mr.remix(matrix, x) for x in xs]
    return [make_case("remix", ci, co, t, xs, wants, [mr.record(w, matrix, 0, FLOOR) for w in wants], matrix=matrix)]


def build_resample(ch, omx):
    out = []
    for rates in RESAMPLE_RATES:
        rule = ResampleRule(*rates)
        pl = lib_plan(omx, *rates)
        t = int(resample_plan(omx, rule)["tile_frames"])
        xs = inputs_of(300 + ch, lengths_of(t), ch, rr.noise)
        wants, records = [], []
        for x in xs:
            r = rr.Resampler(pl, ch, FLOOR)
            wants.append(r.feed(x, flush=True))
            records.append(r.record())
        calls = carried_calls(xs, t, wants, lambda s, n, e, f, flush: resample_frames(omx, rule, n, e, f, flush), True)
        out.append(make_case("resample", ch, ch, t, xs, wants, records, calls, rates=rates, plan=pl))
    return out


def build_convolve(ch, omx):
    info = convolve_plan(omx, ch, 4096)
    t, KB = int(info["tile_frames"]), int(info["tap_block"])
    T = KB + 1
    delay = (T - 1) // 2
    taps = cr.random_taps(10 * T + ch, T)
    xs = inputs_of(500 + ch, lengths_of(t), ch, cr.noise)
    wants, records = [], []
    for x in xs:
        st = cr.Stream([taps] * ch, delay, T, FLOOR)
        wants.append(st.feed(x, flush=True))
        records.append(st.record())
    calls = carried_calls(xs, t, wants, lambda s, n, e, f, flush: convolve_frames(omx, delay, n, e, f, flush), True)
    return [make_case("convolve", ch, ch, t, xs, wants, records, calls, taps=taps, delay=delay)]


def build_dynamics(ch, omx):
    """one curve with a look-ahead longer than a peel (attack 16); once without a key, once with a key and the gain trace"""
    tl = tiles(omx, ch)
    t = tl["smooth_tile"]
    curve = dr.Curve(compressor(omx), (1 << ch) - 1, 16, 100, step_over(20.0, 3 * tl["release_tile"]))
    lengths = lengths_of(t)
    xs = [bursts(10 + s, f, ch, every=900, length=200, first=100) for s, f in enumerate(lengths)]
    xs[3] = hard_edges(xs[3])
    keys = [bursts(70 + s, f, ch, every=700, length=150, first=50) for s, f in enumerate(lengths)]
    keys[3] = hard_edges(keys[3])[::-1].copy()
    out = []
    for key in (None, keys):
        wants, traces, Es, records = [], [], [], []
        for s, x in enumerate(xs):
            o, tr, E = dr.render(curve, x, None if key is None else key[s])
            wants.append(o)
            traces.append(tr)
            Es.append(E)
            records.append(dict(dr.record(E, o), frames_in=len(x), frames_out=len(x), state=DYNAMICS_FLUSHED, latency_frames=curve.latency, curve_index=0))
        calls = carried_calls(xs, t, wants, lambda s, n, e, f, flush: dynamics_frames(omx, curve.latency, n, e, f, flush), True, keys=key)
        at = [0] * N
        for call in calls:      # the trace rides with the output
            call["traces"] = [tr[a:a + k] for tr, a, k in zip(traces, at, call["emits"])]
            at = [a + k for a, k in zip(at, call["emits"])]
        out.append(make_case("dynamics", ch, ch, t, xs, wants, records, calls, curve=curve, keys=key, traces=traces, E=Es))
    assert any((E < 0).any() for E in out[0]["E"]) and any((E == 0).any() for E in out[0]["E"]), "reduced and unity frames have to occur both"
    return out


def build_limiter(ch, omx):
    t = lr.APPLY_TILE_FLOATS // ch
    coeffs = pk.coefficients(oracle_api())
    LA = lr.latency(LIMIT_RULE)
    xs = [lr.noise(700 + 10 * ch + s, f, ch) for s, f in enumerate(lengths_of(t))]
    xs[3] = hard_edges(lr.planted(xs[3], 700 + ch))
    wants, records = [], []
    for s, x in enumerate(xs):
        lim = lr.Limiter(LIMIT_RULE, FS, coeffs, ch, FLOOR)
        o, _ = lim.feed(x, flush=True, gain=LIMIT_FACTORS[s], gain_index=s)
        wants.append(o)
        records.append(lim.record())
    calls = carried_calls(xs, t, wants, lambda s, n, e, f, flush: n + f - e if flush else max(e, n + f - LA) - e, True)
    assert sum(int(r["frames_limited"]) for r in records) > 0
    return [make_case("limiter", ch, ch, t, xs, wants, records, calls, factors=LIMIT_FACTORS)]


def build_filter(ch, omx):
    """the reference-order restatement; the records are per call (the stage writes them fresh), so the GPU file makes them from the
    call's output"""
    t = int(filter_plan(omx, ch, FS)["tile_frames"])
    filters = filter_table_for(FS)
    foc = per_channel(N, ch) if ch > 1 else None
    xs = inputs_of(900 + ch, lengths_of(t), ch, lambda seed, f, c: filter_noise(seed, f, c, 1.2))
    wants, _ = filter_restate(filters, foc, xs, ch)
    calls = carried_calls(xs, t, wants, lambda s, n, e, f, flush: f, False)
    return [make_case("filter", ch, ch, t, xs, wants, None, calls, filters=filters, foc=foc)]


def build_inspect(ch, omx):
    t = int(inspect_plan(omx, ch)["tile_frames"])
    rule = dict(clip_min_run=2, silence_min_run=2)
    xs = inputs_of(1100 + ch, lengths_of(t), ch, lambda seed, f, c: ir.noise(seed, f, c, 1.2 if c <= 3 else 0.9))
    pairs = pairs_of(ch)
    records = [ir.record(x, ch, ir.Rule(**rule), pairs) for x in xs]
    return [make_case("inspect", ch, 0, t, xs, None, records, rule=rule, pairs=pairs)]


def edit_clips(t):
    """per output of 0, 1, t - 1, t + 1 and 2 t + 3 frames: nothing; one frame under a gain; a crossfade of two parts of stream 2 whose
    sources lie a whole number of 16-byte vectors apart (four frames); a copy of stream 3, hard values included, on bits; a crossfade
    inside stream 4 whose two sources lie an ODD number of frames apart, between two silent frames and a silent tail.  No NaN lies
    under a gain or under two clips"""
    assert t >= 128
    b_dst = 2 + (t + 10) - 64
    b_src = 4 + t % 2      # (b_src - b_dst) - (1 - 2) = b_src - t + 53: odd
    assert ((b_src - b_dst) - (1 - 2)) % 2 == 1
    return [er.Clip(1, 1, 0, 0, 1, gain=0.75),
            er.Clip(2, 2, 0, 0, 40, 0, 16, 0, 1, 0, 0.9), er.Clip(2, 2, 20, 24, t - 1 - 24, 16, 0, 1, 0, 0, 0.7),
            er.Clip(3, 3, 0, 0, t + 1),
            er.Clip(4, 4, 1, 2, t + 10, 0, 64, 0, 1, 0, 0.9), er.Clip(4, 4, b_src, b_dst, t + 40, 64, 0, 2, 0, 0, 0.7)]


def build_edit(ch, omx):
    t = int(edit_plan(omx, ch)["tile_frames"])
    out_frames = lengths_of(t)
    xs = inputs_of(1300 + ch, out_frames, ch, lambda seed, f, c: er.noise(seed, f, c, 1.1))
    clips = edit_clips(t)
    wants, records = er.render(xs, clips, out_frames, ch, tabs_of(omx))
    assert wants[3].tobytes() == xs[3].tobytes() and int(records[4]["mixed_frames"]) == 64 and int(records[4]["silent_frames"]) > 2
    return [make_case("edit", ch, ch, t, xs, wants, records, clips=clips, out_frames=out_frames)]


def mix_sends(t):
    """per bus of 0, 1, t - 1, t + 1 and 2 t + 3 frames: nothing; one frame; NO send (the whole window is the zero fill); stream 3
    alone, hard values included; three sends of streams 4 and 2, two of them layered, behind two silent frames and in front of a silent
    tail"""
    assert t >= 64
    return [xr.Send(1, 1, 0, 0, 1), xr.Send(3, 3, 0, 0, t + 1),
            xr.Send(4, 4, 1, 2, t + 10, 0.75), xr.Send(2, 4, 0, 5, t - 1, -0.5), xr.Send(4, 4, 0, t + 30, t - 40, 1.25)]


def build_mix(ch, omx):
    t = int(mix_plan(omx, ch)["tile_frames"])
    out_frames = lengths_of(t)
    xs = inputs_of(1500 + ch, out_frames, ch, lambda seed, f, c: xr.noise(seed, f, c, 1.1))
    sends = mix_sends(t)
    wants, records = xr.render(xs, sends, out_frames, ch)
    assert int(records[2]["silent_frames"]) == t - 1 and int(records[2]["sends"]) == 0 and int(records[4]["mixed_frames"]) > 0
    return [make_case("mix", ch, ch, t, xs, wants, records, sends=sends, out_frames=out_frames)]


def build_import_pcm(ch, omx):
    """d_in holds integer rows: its unit is the byte, and it moves by 0, 4, 8 and 12 bytes"""
    t = pr.TILE_SAMPLES // ch
    counts = lengths_of(t)
    out = []
    for fmt in (pr.S16, pr.S24, pr.S32):
        cap = odd_above(max(counts))
        raws = [pr.random_pcm(10 * cap + s + fmt, cap, ch, fmt) for s in range(N)]
        wants = [pr.import_pcm(raw[:f * ch * pr.BYTES[fmt]], fmt, ch) for raw, f in zip(raws, counts)]
        case = make_case("import_pcm", ch, ch, t, [np.zeros((f, ch), np.float32) for f in counts], wants, None, fmt=fmt, raws=raws, counts=counts)
        case.update(in_unit=1, in_row_bytes=cap * ch * pr.BYTES[fmt], blob=np.frombuffer(b"".join(raws), np.uint8).copy())
        out.append(case)
    return out


def build_export_pcm(ch, omx):
    """d_out holds integer rows: its unit is the byte, and it moves by 0, 4, 8 and 12 bytes.  The dither rule of test_gpu_program_pcm.py"""
    t = pr.TILE_SAMPLES // ch
    counts = lengths_of(t)
    out = []
    for fmt in (pr.S16, pr.S24, pr.S32):
        rule = (fmt, pr.TPDF, 0xC0FFEE + ch)
        xs = pr.export_case_streams(100 * ch + fmt, counts, ch, fmt)
        xs[3] = hard_edges(xs[3])
        wants, records = [], []
        for s, x in enumerate(xs):
            ex = pr.Exporter(rule, s, FLOOR)
            wants.append(np.frombuffer(ex.feed(x), np.uint8).copy())
            records.append(ex.record())
        case = make_case("export_pcm", ch, ch, t, xs, [np.zeros((f, ch), np.float32) for f in counts], records, fmt=fmt, rule=rule)
        case.update(out_unit=1, out_row_bytes=case["cap"] * ch * pr.BYTES[fmt], out_cap=case["cap"], wants=wants)
        case["calls"] = [dict(rows=xs, emits=counts, wants=wants, flush=False)]
        out.append(case)
    return out


def build_apply_gains(ch, omx):
    """in place at the four offsets, through test_gpu_program_normalize.apply_case (the 16 pairs out of place are in that file); the
    tile is the pass's, in floats"""
    import program_normalize_ref as nr
    t = APPLY_TILE_FLOATS // ch
    xs = [nr.noise(1700 + 10 * ch + s, f, ch) for s, f in enumerate(lengths_of(t))]
    xs[3] = hard_edges(nr.planted(xs[3], 1700 + ch))
    factors = [1.7, 0.3, 1.0, 2.5, 1.05]
    wants = [nr.apply(x, g)[0] for x, g in zip(xs, factors)]
    return [make_case("apply_gains", ch, ch, t, xs, wants, None, factors=factors)]


def build_process(ch, omx):
    """measurement: the programmes of the loudness tests at the lowest rate of the normalize tests, cut to nothing, one frame, one frame
    either side of a 100 ms segment, and 8 s"""
    fs = PROCESS_RATE
    seg = lref.segment_frames(fs)
    lengths = [0, 1, seg - 1, seg + 1, int(8 * fs)]
    xs = [lref.programme(seed, fs, ch, 8)[:f] for seed, f in zip(PROCESS_SEEDS, lengths)]
    oracle = oracle_api()
    pos = capi.positions_fallback(ch)
    loud = [lref.restate(x, fs, pos, oracle.k_weighting_coefficients(lref.sanitize_rate(fs))) for x in xs]
    peaks = [pk.restate(x, fs, pk.coefficients(oracle), FLOOR) for x in xs]
    return [make_case("process", ch, 0, seg, xs, None, loud, peaks=peaks, fs=fs, positions=pos)]


BUILDERS = {"remix": build_remix, "resample": build_resample, "convolve": build_convolve, "dynamics": build_dynamics, "limiter": build_limiter,
            "filter": build_filter, "inspect": build_inspect, "edit": build_edit, "mix": build_mix, "import_pcm": build_import_pcm,
            "export_pcm": build_export_pcm, "apply_gains": build_apply_gains, "process": build_process}
EVERY_CASE = [(stage, ch) for stage, chans in CHANNELS.items() for ch in chans]


# ================================================================ coverage, computed
def row_units(case, side):
    """elements between the row bases of a side: floats, or bytes of an integer side"""
    if side == "in":
        return case.get("in_row_bytes", case["cap"] * case["ci"])
    return case.get("out_row_bytes", case["out_cap"] * case["co"])


def base_residues(case, side):
    """byte residues mod 16 of every stream's row base over the offsets of a side"""
    bytes_per = case["in_unit" if side == "in" else "out_unit"]
    rows = row_units(case, side)
    return {(4 * a + s * rows * bytes_per) % 16 for a in OFFSETS for s in range(N)}


def peel_of(first_float):
    """floats from a float index to the next 16-byte boundary (ps_to_aligned)"""
    return (-first_float) % 4


def short_rows(case, side, strictly):
    """(offset, stream, floats) of the f32 rows that hold some floats, but fewer than (or, not strictly, as many as) their peel asks
    for: the run ends inside the peel"""
    if case["in_unit" if side == "in" else "out_unit"] != 4:
        return []
    ch = case["ci" if side == "in" else "co"]
    rows = row_units(case, side)
    out = []
    for call in case["calls"]:
        counts = [len(r) for r in call["rows"]] if side == "in" else call["emits"]
        for a in OFFSETS:
            for s, f in enumerate(counts):
                n, peel = f * ch, peel_of(a + s * rows)
                if 0 < n and (n < peel or (not strictly and n == peel)):
                    out.append((a, s, n))
    return out


def clip_phases(case, a_in, a_out):
    """per clip of the edit case: (source float index - output float index) mod 4.  0: the source's 16-byte vectors line up with the
    output's, whatever the tile (a tile moves both by the same floats)"""
    ch, cap, out_cap = case["ci"], case["cap"], case["out_cap"]
    return [(a_in + (c.src_stream * cap + c.src_first) * ch - a_out - (c.dst_stream * out_cap + c.dst_first) * ch) % 4 for c in case["clips"]]


# ================================================================ a. accepted and in range
@pytest.mark.parametrize("stage,ch", EVERY_CASE)
def test_cases_are_accepted_and_in_range(omx, stage, ch):
    for case in case_of(stage, ch, omx):
        assert len(case["xs"]) == N and case["cap"] % 2 == 1
        longest = max(len(x) for x in case["xs"])
        assert case["cap"] in (longest + 1, longest + 2)
        if stage == "process":
            assert [len(x) for x in case["xs"]] == [0, 1, case["t"] - 1, case["t"] + 1, int(8 * case["fs"])]
            for r in case["records"]:
                assert r["gate_margin"] >= lref.GATE_MARGIN_MIN, r["gate_margin"]
            assert case["records"][4]["gating_above_relative"] > 0
            continue
        t = case["t"]
        assert [len(x) for x in case["xs"]] == lengths_of(t) and t >= 8
        if case["wants"] is None:
            continue
        assert case["out_cap"] % 2 == 1
        written = [0] * N
        for k, call in enumerate(case["calls"]):
            for s in range(N):
                assert len(call["rows"][s]) <= case["cap"] - 1
                assert call["emits"][s] <= case["out_cap"] - 1, (stage, ch, k, s, call["emits"][s], case["out_cap"])
                assert np.asarray(call["wants"][s]).reshape(-1).size == call["emits"][s] * (case["co"] if case["out_unit"] == 4 else
                                                                                            case["co"] * pr.BYTES[case["fmt"]])
                written[s] += call["emits"][s]
        if case["out_unit"] == 4:
            assert written == [len(w) for w in case["wants"]], (stage, ch, written)
        if len(case["calls"]) > 1:      # a carrying stage: two calls cut at t + 1 frames, the second at other offsets
            assert [len(r) for r in case["calls"][0]["rows"]] == [0, 1, t - 1, t + 1, t + 1]
            assert [len(r) for r in case["calls"][1]["rows"]] == [0, 0, 0, 0, t + 2]
            assert all(pair_of_call(1, a, b) == ((a + 1) % 4, (b + 3) % 4) for a, b in PAIRS)
        x3 = case["xs"][3].reshape(-1)
        if stage != "import_pcm":
            assert np.isnan(x3[0]) and np.isinf(x3[1]) and np.signbit(x3[3]) and x3[3] == 0 and np.isnan(x3[-1]) and np.isinf(x3[-4])


# ================================================================ b. coverage
@pytest.mark.parametrize("stage,ch", EVERY_CASE)
def test_every_residue_is_reached_and_a_row_ends_inside_its_peel(omx, stage, ch):
    for case in case_of(stage, ch, omx):
        sides = ["in"] + (["out"] if case["co"] else [])
        for side in sides:
            assert base_residues(case, side) >= {0, 4, 8, 12}, (stage, ch, side, base_residues(case, side))
            channels = case["ci" if side == "in" else "co"]
            if channels in (4, 8) and case["in_unit" if side == "in" else "out_unit"] == 4:      # only the base offset moves these rows
                assert {(s * row_units(case, side) * 4) % 16 for s in range(N)} == {0}
        # a run of a stream that holds floats, but fewer than its peel asks for (min(n, ps_to_aligned)).  At 3 channels a frame is 3
        # floats and a peel at most 3: there the run is as long as the peel, and no body and no tail follow
        if stage == "process" or case["ci"] > 3:
            continue
        strictly = case["ci"] <= 2
        found = [side for side in sides if short_rows(case, side, strictly)]
        assert "in" in found or stage == "import_pcm", (stage, ch, found)
        if stage in ("remix", "edit", "mix", "filter", "apply_gains", "import_pcm") and case["co"] <= 3:
            assert "out" in found, (stage, ch, found)


@pytest.mark.parametrize("ch", CHANNELS["edit"])
def test_edit_case_has_sources_on_and_off_the_outputs_phase(omx, ch):
    """single clips with the source on the output's 16-byte phase and off it; a crossfade with both sources on it, one with source A on
    it and source B off it, and (whatever the pair) none at 3 channels for the crossfade of odd distance: never both"""
    case = case_of("edit", ch, omx)[0]
    single, even, odd = [0, 3], (1, 2), (4, 5)
    phases = {pair: clip_phases(case, *pair) for pair in PAIRS}
    for k in single:
        assert {p[k] == 0 for p in phases.values()} == {True, False}, (ch, k)
    assert {(p[even[0]] == 0 and p[even[1]] == 0) for p in phases.values()} == {True, False}, ch
    assert all((p[even[0]] == 0) == (p[even[1]] == 0) for p in phases.values()), ch
    if ch % 4:      # an odd number of frames apart: at 4 and 8 channels a frame is a whole number of vectors
        assert any(p[odd[0]] == 0 and p[odd[1]] != 0 for p in phases.values()), ch
        assert any(p[odd[0]] != 0 and p[odd[1]] == 0 for p in phases.values()), ch
    if ch % 2:
        assert not any(p[odd[0]] == 0 and p[odd[1]] == 0 for p in phases.values()), ch
    a, b = case["clips"][4], case["clips"][5]
    assert a.src_stream == b.src_stream and ((b.src_first - b.dst_first) - (a.src_first - a.dst_first)) % 2 == 1


# ================================================================ c. the comparison rejects what it is there for
def rejected(*args, **kw):
    with pytest.raises(AssertionError) as err:
        check_image(*args, **kw)
    return str(err.value)


@pytest.mark.parametrize("ch", CHANNELS["remix"])
def test_comparison_rejects_a_missing_a_stray_and_a_shifted_float(omx, ch):
    import torch
    case = case_of("remix", ch, omx)[0]
    rows, wants = case["out_cap"] * case["co"], case["wants"]
    blank = np.full(N * rows, SENTINEL, np.float32)
    for a_out in OFFSETS:
        # (d) the store comes from placed(), behind a stale allocation of its size full of something else
        stale = torch.full((blank.size + pad_of(np.float32),), 3.5, dtype=torch.float32)
        del stale
        store, ptr = placed(torch, blank, a_out, SENTINEL, device="cpu")
        before = store.numpy().copy()
        assert ptr - store.data_ptr() == 4 * a_out and before.size == blank.size + 8
        assert bits_of(before).tolist() == [int(SENTINEL.view(np.uint32))] * before.size
        good = expected_image(before, wants, a_out, rows)
        check_image(good, before, wants, a_out, rows, "as it should be")
        for s in (1, 2, 3, 4):
            size, at = wants[s].size, a_out + s * rows
            bad = good.copy()                      # 1. the row's first float left at the sentinel
            bad[at] = SENTINEL
            assert "differs" in rejected(bad, before, wants, a_out, rows, "first float missing")
            bad = good.copy()                      # 2. the row's last float written one place further
            bad[at + size], bad[at + size - 1] = good[at + size - 1], SENTINEL
            rejected(bad, before, wants, a_out, rows, "last float one place further")
            bad = good.copy()
            bad[at + size] = good[at + size - 1]      # ... and written twice: only the float behind the row is wrong
            assert "beyond" in rejected(bad, before, wants, a_out, rows, "a float behind the row")
            bad = good.copy()                      # the whole row shifted by one float
            bad[at + 1:at + 1 + size], bad[at] = good[at:at + size], SENTINEL
            rejected(bad, before, wants, a_out, rows, "shifted")
        if a_out:                                  # 3. a guard float in front of d_out overwritten
            bad = good.copy()
            bad[a_out - 1] = np.float32(0.0)
            assert "in front" in rejected(bad, before, wants, a_out, rows, "front guard")
        bad = good.copy()                          # ... and one behind the last row
        bad[a_out + N * rows] = np.float32(0.0)
        assert "behind the last row" in rejected(bad, before, wants, a_out, rows, "back guard")
    # a NaN stands for a NaN only where asked to; -0.0 is not +0.0
    x = np.array([np.nan, -0.0, 1.0, 2.0], np.float32)
    other = x.copy()
    other.view(np.uint32)[0] = 0x7FA00001
    before = np.full(4 + 8, SENTINEL, np.float32)
    check_image(expected_image(before, [other], 0, 4), before, [x], 0, 4, "any NaN")
    rejected(expected_image(before, [other], 0, 4), before, [x], 0, 4, "on bytes", nan_as_nan=False)
    other = x.copy()
    other[1] = 0.0
    rejected(expected_image(before, [other], 0, 4), before, [x], 0, 4, "the sign of zero")


# ================================================================ d. placement
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_placed_puts_the_rows_at_the_offset_and_the_fill_everywhere_else(dtype):
    import torch
    rng = np.random.default_rng(9)
    host = rng.integers(1, 200, 3 * 37).astype(dtype).reshape(3, 37)
    step = 1 if dtype == np.float32 else 4
    for fill in (SENTINEL if dtype == np.float32 else SENTINEL_BYTE, input_fill(host)):
        for a in OFFSETS:
            stale = torch.from_numpy(np.full(host.size + pad_of(dtype), 7, dtype))      # an allocation of the same size, let go
            del stale
            store, ptr = placed(torch, host, a * step, fill, device="cpu")
            got = store.numpy()
            assert got.size == host.size + 32 // np.dtype(dtype).itemsize and got.dtype == dtype
            assert store.data_ptr() % 16 == 0 and ptr - store.data_ptr() == 4 * a
            assert got[a * step:a * step + host.size].tobytes() == host.tobytes()
            want = np.empty_like(got)
            want[:] = fill
            outside = np.r_[0:a * step, a * step + host.size:got.size]
            assert got[outside].tobytes() == want[outside].tobytes()
            assert store_image(host, a * step, fill).tobytes() == got.tobytes()

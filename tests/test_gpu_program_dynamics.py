"""Programme bank dynamics stage on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_dynamics / dynamics /
reset_dynamics / fetch_dynamics against the restatement in numpy and Python integers (tests/program_dynamics_ref.py, pinned by
tests/test_cpu_program_dynamics.py).

Bars.  Every float of d_out and of the gain trace equals the restatement's on bytes, with a NaN where it has a NaN (the bits of a NaN
the arithmetic produces are not defined; a frame with E = 0 and every frame of a bypassed stream is compared on bytes, NaN payloads
included); every record field equal except the dB fields, within 1e-4 dB (the family's bar).  Not written: d_out and the trace hold a
sentinel beforehand and nothing at or beyond frames_written[s] is touched; d_in and d_key keep their bytes.  Cut invariance: every
programme is rendered whole and in cuts (calls of 0, 1 and LA - 1 frames, ragged across streams, the flush on the last frames or in a
call of its own) and every schedule gives the bytes of the restatement's one-call output.
Shapes come from dynamics_plan.  The inputs are loud bursts between quiet stretches, and the tests of the release scan assert on the
restatement first that the ramp term r[n-1] + d is the smaller one on at least 100 frames on each side of a tile boundary and of a
call boundary: an input that never leaves the hold term proves nothing about the scan.  No test provokes a fault: the refusals use
only arguments the host rejects before any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_dynamics_ref as dr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (DYNAMICS_BYPASS, DYNAMICS_FLUSHED, DYNAMICS_IDLE, DYNAMICS_RUNNING, DynamicsCurve,
                                             DynamicsSpec, ProgramLoudnessBank, dynamics_design, dynamics_frames, dynamics_from_points,
                                             dynamics_plan)
from test_cpu_program_dynamics import build_demo
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
CHANNELS = (1, 2, 3, 6, 8)
EXACT = ("frames_in", "frames_out", "frames_written", "frames_reduced", "frames_boosted", "samples_over", "samples_nonfinite", "min_gain",
         "max_gain", "state", "latency_frames", "curve_index")


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def tiles(omx, ch=2):
    info = dynamics_plan(omx, ch)
    return {k: int(info[k]) for k in ("level_tile", "hold_tile", "hold_max_window", "release_tile", "smooth_tile")}


def step_over(db, frames):
    """the release step that takes `db` dB back over `frames` frames"""
    return max(1, int(db / dr.OCTAVE_DB * 4294967296.0 / frames))


def compressor(omx, threshold=-30.0, ratio=4.0, knee=6.0, makeup=0.0):
    return dynamics_design(omx, DynamicsSpec(threshold, ratio, knee, makeup_db=makeup))


def bursts(seed, n, ch, every=2600, length=350, quiet=0.003, loud=0.3, first=600):
    """noise at about -50 dB with bursts at about -10 dB: the gain of a compressor at -30 dB falls in every burst and is released
    in the stretch behind it"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, ch)) * quiet).astype(np.float32)
    for b in range(first + 37 * (seed % 7), n, every):
        x[b:b + length] *= np.float32(loud / quiet)
    return x


def ramp_frames(curve, Gt):
    """per n of a flushed stream: the ramp term r[n-1] + d is the smaller operand of the release"""
    r, _E = dr.envelope(curve, Gt, True)
    W, t0 = curve.A + curve.H, int(curve.T[0])
    ext = np.concatenate([np.full(W - 1, t0, np.int64), np.asarray(Gt, np.int64), np.full(curve.A - 1, t0, np.int64)])
    w = dr.sliding_min(ext, W) << 16
    prev = np.concatenate([[t0 << 16], r[:-1]])
    return (prev + curve.d) < w


def ramps_across(flags, boundary, side=100):
    return boundary - side >= 0 and boundary + side <= len(flags) and bool(flags[boundary - side:boundary + side].all())


def same_floats(got, want, tag, exact=None):
    """bytes, or a NaN where the restatement has a NaN; rows flagged in `exact` on bytes whatever they hold"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    if exact is not None:
        nan = nan & ~np.asarray(exact).reshape((-1,) + (1,) * (want.ndim - 1))
    assert np.isnan(got[nan]).all(), (tag, "a NaN of the restatement is not a NaN")
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (tag, bad.size, "floats differ, the first at", int(bad[0]), hex(int(g[bad[0]])), hex(int(w[bad[0]])))


def check_record(rec, want, tag):
    for f in EXACT:
        assert int(rec[f]) == int(want[f]), (tag, f, int(rec[f]), int(want[f]))
    assert rec["out_sample_peak"].tobytes() == np.float32(want["out_sample_peak"]).tobytes(), (tag, rec["out_sample_peak"], want["out_sample_peak"])
    p = float(want["out_sample_peak"])
    dbs = {"min_gain_db": want["min_gain"] * (dr.OCTAVE_DB / 4294967296.0), "max_gain_db": want["max_gain"] * (dr.OCTAVE_DB / 4294967296.0),
           "out_sample_peak_db": max(20.0 * np.log10(p), FLOOR) if p > 0.0 else FLOOR}
    for f, v in dbs.items():
        assert float(rec[f]) == v or abs(float(rec[f]) - v) <= BAR, (tag, f, float(rec[f]), v)      # (equal: an infinite output peak)


class Setup:
    """a configured bank with the restatement's view of it: per stream its curve (a bypassed stream: zeros under the longest attack)"""

    def __init__(self, omx, n, ch, curves, curve_of_stream=None):
        self.omx, self.n, self.ch = omx, n, ch
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
        self.bank.configure_dynamics([DynamicsCurve(c.T.astype(np.int32), c.mask, c.A, c.H, c.d) for c in curves], ch, curve_of_stream)
        self.index = [0] * n if curve_of_stream is None else [int(k) for k in curve_of_stream]
        longest = max(c.A for c in curves)
        self.curves = [dr.Curve(np.zeros(dr.POINTS, np.int64), 1, longest, 0, dr.MAX_STEP) if k == DYNAMICS_BYPASS else curves[k] for k in self.index]
        self.mirror = [(0, 0)] * n      # (frames taken, frames emitted)

    def call(self, torch, rows, keys=None, flush=None, filler=999, trace=True):
        """rows[s]: f32 [frames][ch] of stream s in this call (keys[s]: its side chain); frames of d_in beyond them hold other samples.
        d_out and the trace hold the sentinel beforehand.  -> (per stream the frames written, their gains, the records' pointer)"""
        n, ch = self.n, self.ch
        counts = [len(r) for r in rows]
        cap = max(max(counts), 1)
        rng = np.random.default_rng(filler)
        host = rng.standard_normal((n, cap, ch)).astype(np.float32)
        host_key = rng.standard_normal((n, cap, ch)).astype(np.float32)
        for s, r in enumerate(rows):
            host[s, :len(r)] = r
            if keys is not None:
                host_key[s, :len(r)] = keys[s]
        emits = [dynamics_frames(self.omx, self.curves[s].latency, self.mirror[s][0], self.mirror[s][1], counts[s], bool(flush and flush[s]))
                 for s in range(n)]
        out_cap = max(max(emits) + 1, 1)
        d_in, d_key = torch.from_numpy(host).cuda(), torch.from_numpy(host_key).cuda() if keys is not None else None
        d_out = torch.full((n, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
        d_tr = torch.full((n, out_cap), float(SENTINEL), dtype=torch.float32).cuda() if trace else None
        ptr = self.bank.dynamics(d_in.data_ptr(), cap, d_out.data_ptr(), out_cap, frames=counts, flush_mask=flush,
                                 d_key=d_key.data_ptr() if keys is not None else 0, d_gain_db=d_tr.data_ptr() if trace else 0,
                                 stream=stream_of(torch))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        got_tr = d_tr.cpu().numpy() if trace else np.full((n, out_cap), SENTINEL, np.float32)
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
        assert keys is None or d_key.cpu().numpy().tobytes() == host_key.tobytes(), "d_key changed"
        out, gains = [], []
        for s in range(n):
            w = int(self.bank.fetch_dynamics(s)["frames_written"])
            lat = self.curves[s].latency
            assert w == emits[s] == dr.emitted(lat, self.mirror[s][0] + counts[s], self.mirror[s][1], bool(flush and flush[s])) - self.mirror[s][1]
            assert (got[s, w:] == SENTINEL).all() and (got_tr[s, w:] == SENTINEL).all(), (s, w, "written at or beyond frames_written[s]")
            out.append(got[s, :w].copy())
            gains.append(got_tr[s, :w].copy())
            self.mirror[s] = (self.mirror[s][0] + counts[s], self.mirror[s][1] + w)
        return out, gains, ptr

    def render(self, torch, xs, keys, cuts, own_flush):
        """every stream's programme in calls that end at the frame positions cuts[i][s] (the last call takes the rest); the flush in
        the last call, or in a call of its own"""
        n = self.n
        at, parts, gains, last_written = [0] * n, [[] for _ in range(n)], [[] for _ in range(n)], [0] * n
        for i in range(len(cuts) + 1):
            last = i == len(cuts)
            rows, krows = [], []
            for s, x in enumerate(xs):
                end = len(x) if last else max(at[s], min(int(cuts[i][s]), len(x)))
                rows.append(x[at[s]:end])
                krows.append(None if keys is None else keys[s][at[s]:end])
                at[s] = end
            out, tr, ptr = self.call(torch, rows, None if keys is None else krows, flush=[1] * n if last and not own_flush else None, filler=900 + i)
            for s in range(n):
                parts[s].append(out[s])
                gains[s].append(tr[s])
                last_written[s] = len(out[s])
        if own_flush:
            out, tr, ptr = self.call(torch, [x[:0] for x in xs], None if keys is None else [k[:0] for k in keys], flush=[1] * n)
            for s in range(n):
                parts[s].append(out[s])
                gains[s].append(tr[s])
                last_written[s] = len(out[s])
        return [np.concatenate(p) for p in parts], [np.concatenate(g) for g in gains], last_written, ptr


def restate(setup, xs, keys=None):
    """per stream (out, trace, E, record) of the whole flushed programme, once"""
    wants = []
    for s, x in enumerate(xs):
        c = setup.curves[s]
        out, tr, E = dr.render(c, x, None if keys is None else keys[s])
        rec = dict(dr.record(E, out), frames_in=len(x), frames_out=len(x), state=DYNAMICS_FLUSHED, latency_frames=c.latency,
                   curve_index=setup.index[s])
        wants.append((out, tr, E, rec))
    return wants


def schedules_for(xs, latency, extra=()):
    """cut positions per call and stream: whole; a call of 0, of 1 and of LA - 1 frames, then ragged cuts, the flush apart; halves"""
    n = len(xs)
    few = max(latency - 1, 0)
    ragged = [[0] * n, [1] * n, [1 + few] * n, [int(len(x) * (0.3 + 0.05 * (s % 5))) for s, x in enumerate(xs)],
              [int(len(x) * (0.3 + 0.05 * (s % 5))) if s % 2 else int(len(x) * 0.7) for s, x in enumerate(xs)]]
    return [(([], False), "whole"), ((ragged, True), "0 / 1 / LA - 1 / ragged, flush apart"),
            (([[len(x) // 2 for x in xs]], False), "halves")] + list(extra)


def check_programmes(torch, omx, ch, curves, xs, keys=None, curve_of_stream=None, schedules=None, tag=None):
    """every schedule against the restatement's one-call output: bytes of d_out and of the trace, and the records"""
    n = len(xs)
    wants = None
    for (cuts, own_flush), name in schedules:
        setup = Setup(omx, n, ch, curves, curve_of_stream)
        if wants is None:
            wants = restate(setup, xs, keys)
        got, tr, last_written, ptr = setup.render(torch, xs, keys, cuts, own_flush)
        for s in range(n):
            out, trace, E, rec = wants[s]
            same_floats(got[s], out, (tag, name, "stream", s), exact=E == 0)
            assert tr[s].tobytes() == trace.tobytes(), (tag, name, "trace of stream", s)
            check_record(setup.bank.fetch_dynamics(s), dict(rec, frames_written=last_written[s]), (tag, name, s))
        assert device_bytes(ptr, n * 104) == b"".join(setup.bank.fetch_dynamics(s).tobytes() for s in range(n))
    return wants


def assert_scan_is_exercised(curve, x, wants, boundaries, tag):
    """the ramp term governs on 100 frames on each side of one of `boundaries`; reduced and unity frames both occur"""
    flags = ramp_frames(curve, dr.target(curve, x))
    assert any(ramps_across(flags, b) for b in boundaries), (tag, "the ramp term does not govern across any of", boundaries)
    E = wants[2]
    assert (E < 0).any() and (E == 0).any(), (tag, "reduced and unity frames have to occur both")


# ---------------------------------------------------------------- 1. lengths at every pass's tile, every channel count
@pytest.mark.parametrize("ch", CHANNELS)
def test_lengths_around_every_tile(torch_dev, omx, ch):
    """one ragged bank: t - 1, t, t + 1 and 2 t + 1 frames for each pass's tile, and streams of 0, 1 and 2 frames.  The release takes
    20 dB back over about three release tiles, so that the ramp crosses the tile boundaries of the long streams."""
    t = tiles(omx, ch)
    lengths = sorted({v for tile in set(t.values()) for v in (tile - 1, tile, tile + 1, 2 * tile + 1)}) + [0, 1, 2]
    curve = dr.Curve(compressor(omx), (1 << ch) - 1, 16, 100, step_over(20.0, 3 * t["release_tile"]))
    xs = [bursts(10 + s, f, ch) for s, f in enumerate(lengths)]
    longest = int(np.argmax(lengths))
    cut = [[0] * len(xs), [t["release_tile"] + 500 if len(x) > 3000 else len(x) // 2 for x in xs]]
    wants = check_programmes(torch_dev, omx, ch, [curve], xs,
                             schedules=[(([], False), "whole"), ((cut, True), "none / past the first release tile, flush apart")], tag=ch)
    assert_scan_is_exercised(curve, xs[longest], wants[longest], [t["release_tile"], 2 * t["release_tile"]], ch)
    assert_scan_is_exercised(curve, xs[longest], wants[longest], [t["release_tile"] + 500], (ch, "call boundary"))


# ---------------------------------------------------------------- 2. attack, hold and release step
@pytest.mark.parametrize("attack", [1, 16, 240, 4096])
@pytest.mark.parametrize("hold", [0, 100, 16384])
def test_attack_hold_and_release_steps(torch_dev, omx, attack, hold):
    """every attack and hold (W = A + H beyond a hold tile with H = 16384 or A = 4096), three streams with the three release steps:
    1 (the ramp never ends), 20 dB over about three tiles, and the maximum (an instant release: the scan's carry never governs)"""
    t = tiles(omx)
    T = compressor(omx)
    steps = [1, step_over(20.0, 3 * t["release_tile"]), dr.MAX_STEP]
    curves = [dr.Curve(T, 3, attack, hold, d) for d in steps]
    n = 3 * t["release_tile"] + 517
    xs = [bursts(20 + s, n, 2, every=2 * t["release_tile"] + 300, length=200) for s in range(3)]
    cuts = [[t["release_tile"] + 700] * 3]
    wants = check_programmes(torch_dev, omx, 2, curves, xs, curve_of_stream=[0, 1, 2],
                             schedules=[(([], False), "whole"), ((cuts, False), "cut inside the release")], tag=(attack, hold))
    if attack + hold < t["release_tile"] // 2:      # (a longer window holds the gain down over the stretch the ramp would cover)
        assert_scan_is_exercised(curves[1], xs[1], wants[1], [t["release_tile"], 2 * t["release_tile"]], (attack, hold))
        assert_scan_is_exercised(curves[1], xs[1], wants[1], [t["release_tile"] + 700], (attack, hold, "call boundary"))
        flags = ramp_frames(curves[0], dr.target(curves[0], xs[0]))
        assert ramps_across(flags, 2 * t["release_tile"]), "with d = 1 the ramp governs from the end of the first hold on"
    assert not ramp_frames(curves[2], dr.target(curves[2], xs[2])).any(), "an instant release never takes the ramp term"


# ---------------------------------------------------------------- 3. stream counts, cut schedules
@pytest.mark.parametrize("n", [1, 3, 65])
def test_stream_counts_and_cut_schedules(torch_dev, omx, n):
    """1, 3 and 65 streams (past one wavefront of the per-stream kernels) of ragged lengths, every schedule of schedules_for"""
    t = tiles(omx)
    curve = dr.Curve(compressor(omx), 3, 64, 480, step_over(20.0, 2 * t["release_tile"]))
    xs = [bursts(40 + s, 2 * t["release_tile"] + 300 + 97 * (s % 9) if s % 4 else 150 + s, 2, every=1900) for s in range(n)]
    if n == 1:
        xs = [bursts(40, 3 * t["release_tile"] + 11, 2, every=1900)]
    wants = check_programmes(torch_dev, omx, 2, [curve], xs, schedules=schedules_for(xs, curve.latency), tag=n)
    long = max(range(n), key=lambda s: len(xs[s]))
    assert_scan_is_exercised(curve, xs[long], wants[long], [t["release_tile"], 2 * t["release_tile"]], n)


# ---------------------------------------------------------------- 4. routing
def test_side_chain_mask_curves_and_bypass_in_one_bank(torch_dev, omx):
    """six streams of one bank: a key that differs from the input (ducking), a detector mask that leaves out the loud channel, an
    expander curve, a sox-style points curve with a longer attack, a curve of zeros, and a bypassed stream beside them.  The curve of
    zeros and the bypass are plain delayed copies on bytes."""
    t = tiles(omx)
    ch, n = 3, 2 * t["smooth_tile"] + 333
    duck = dr.Curve(compressor(omx, -35.0, 8.0, 0.0), 0b111, 48, 240, step_over(30.0, 4000))
    masked = dr.Curve(compressor(omx, -35.0, 8.0, 0.0), 0b101, 48, 240, step_over(30.0, 4000))
    expander = dr.Curve(dynamics_design(omx, DynamicsSpec(0.0, 1.0, 0.0, -40.0, 2.0, 30.0, 4.0)), 0b111, 8, 0, step_over(30.0, 500))
    points = dr.Curve(dynamics_from_points(omx, [(-80.0, -100.0), (-45.0, -45.0), (-20.0, -15.0), (0.0, -6.0)]), 0b011, 240, 100, step_over(20.0, 3000))
    zeros = dr.Curve(np.zeros(dr.POINTS, np.int64), 0b111, 33, 7, 12345)
    curves = [duck, masked, expander, points, zeros]
    xs = [bursts(60 + s, n, ch, every=1500) for s in range(6)]
    xs[4][5, 0], xs[4][6, 1], xs[5][7, 2] = np.float32(np.nan), np.float32(-0.0), np.uint32(0x7FA00001).view(np.float32)
    keys = [bursts(70 + s, n, ch, every=1100, length=500) for s in range(6)]
    keys[1][:, 1] = np.float32(0.9)                # the loud channel the mask leaves out
    index = [0, 1, 2, 3, 4, DYNAMICS_BYPASS]
    wants = check_programmes(torch_dev, omx, ch, curves, xs, keys=keys, curve_of_stream=index,
                             schedules=[(([], False), "whole"), (([[0] * 6, [1] * 6, [n // 3 + 5 * s for s in range(6)]], True), "cuts")])
    for s in (4, 5):
        assert wants[s][0].tobytes() == xs[s].tobytes() and not wants[s][2].any()
    assert not (wants[0][2] == dr.envelope(duck, dr.target(duck, xs[0]))[1]).all(), "the key, not the input, sets the gain"
    assert (dr.envelope(duck, dr.target(duck, keys[1]))[1] < 0).all() and (wants[1][2] == 0).any(), "the mask leaves the loud channel out"
    assert (wants[2][2] < 0).any() and (wants[2][2] > 0).any(), "the expander reduces the quiet stretches, its make-up boosts the bursts"
    assert wants[3][2].any(), "the points curve moves the gain"
    # the latency is per stream: the bypass rides on the longest attack of the table
    setup = Setup(omx, 6, ch, curves, index)
    assert [int(setup.bank.fetch_dynamics(s)["latency_frames"]) for s in range(6)] == [47, 47, 7, 239, 32, 239]
    assert [int(setup.bank.fetch_dynamics(s)["curve_index"]) for s in range(6)] == index
    assert all(int(setup.bank.fetch_dynamics(s)["state"]) == DYNAMICS_IDLE for s in range(6))


def test_a_detector_mask_without_the_loud_channel_stays_at_unity(torch_dev, omx):
    ch, n = 2, 3000
    x = bursts(80, n, ch)
    x[:, 1] = np.float32(0.8)
    T = compressor(omx)
    both, left = dr.Curve(T, 0b11, 16, 50, step_over(20.0, 2000)), dr.Curve(T, 0b01, 16, 50, step_over(20.0, 2000))
    wants = check_programmes(torch_dev, omx, ch, [both, left], [x, x], curve_of_stream=[0, 1], schedules=[(([], False), "whole")])
    assert (wants[0][2] < 0).all() and (wants[1][2] == 0).any()


# ---------------------------------------------------------------- 5. hard values
@pytest.mark.parametrize("ch", [1, 2, 8])
def test_nan_infinities_denormals_and_zeros_in_input_and_key(torch_dev, omx, ch):
    t = tiles(omx, ch)
    n = t["smooth_tile"] + 200
    curve = dr.Curve(compressor(omx, -30.0, 4.0, 6.0, 3.0), (1 << ch) - 1, 16, 30, step_over(20.0, 900))
    hard = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 2.0 ** -40, 2.0 ** -41, 255.9, 256.0, 3e38, 1.0, -1.0], np.float32)
    xs, keys = [], []
    for s in range(3):
        x, k = bursts(90 + s, n, ch, every=700, length=90), bursts(95 + s, n, ch, every=600, length=90)
        rng = np.random.default_rng(s)
        for target in ((x,) if s == 0 else (k,) if s == 1 else (x, k)):
            at = rng.integers(0, n, 60)
            target[at, rng.integers(0, ch, 60)] = hard[rng.integers(0, len(hard), 60)]
            target[t["smooth_tile"] - 1], target[t["smooth_tile"]] = hard[0], hard[1]      # whole frames of NaN and of infinity at a tile seam
        x[100:140] = 0.0          # digital silence: L_MIN
        xs.append(x)
        keys.append(k)
    wants = check_programmes(torch_dev, omx, ch, [curve], xs, keys=keys,
                             schedules=[(([], False), "whole"), (([[n // 2 + s for s in range(3)]], True), "halves, flush apart")], tag=ch)
    assert sum(w[3]["samples_nonfinite"] for w in wants) > 0 and any(np.isnan(w[0]).any() for w in wants)


# ---------------------------------------------------------------- 6. resets
def test_a_reset_of_some_streams_mid_way(torch_dev, omx):
    t = tiles(omx)
    curve = dr.Curve(compressor(omx), 3, 100, 30, step_over(20.0, 3000))
    n = t["release_tile"] + 400
    xs = [bursts(100 + s, n, 2, every=900) for s in range(3)]
    setup = Setup(omx, 3, 2, [curve])
    setup.call(torch_dev, [x[:777] for x in xs])
    setup.bank.reset_dynamics([0, 1, 0])
    setup.mirror[1] = (0, 0)
    rec = setup.bank.fetch_dynamics(1)
    assert (int(rec["state"]), int(rec["frames_in"]), int(rec["frames_reduced"]), int(rec["min_gain"])) == (DYNAMICS_IDLE, 0, 0, 0)
    assert int(setup.bank.fetch_dynamics(0)["state"]) == DYNAMICS_RUNNING
    rows = [xs[0][777:], xs[1], xs[2][777:]]
    out, tr, _ = setup.call(torch_dev, rows, flush=[1, 1, 1])
    for s in range(3):
        want, trace, E = dr.render(curve, xs[s])
        first = 0 if s == 1 else 777 - curve.latency
        same_floats(out[s], want[first:], s, exact=E[first:] == 0)
        assert tr[s].tobytes() == trace[first:].tobytes()
    with pytest.raises(capi.OmxError):      # configure is allowed only while no stream holds frames
        setup.bank.configure_dynamics([DynamicsCurve(curve.T.astype(np.int32), 3, 1, 0, 1)], 2)
    setup.bank.reset_dynamics()
    setup.bank.configure_dynamics([DynamicsCurve(curve.T.astype(np.int32), 3, 1, 0, 1)], 2)
    assert int(setup.bank.fetch_dynamics(2)["latency_frames"]) == 0


# ---------------------------------------------------------------- 7. measurement state
def test_measurement_state_keeps_its_bytes(torch_dev, omx):
    n, ch, frames = 2, 2, 48000
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
    x = np.stack([bursts(110 + s, frames, ch) for s in range(n)])
    d_in = torch_dev.from_numpy(x).cuda()
    bank.process(d_in.data_ptr(), frames, ch, 48000.0, capi.positions_fallback(ch), stream=stream_of(torch_dev))
    before = [record_array(bank.fetch(s)).tobytes() for s in range(n)]
    bank.configure_dynamics([DynamicsCurve(compressor(omx), 3, 64, 480, step_over(20.0, 5000))], ch)
    d_out = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.dynamics(d_in.data_ptr(), frames, d_out.data_ptr(), frames, flush_mask=[1, 1], stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert [record_array(bank.fetch(s)).tobytes() for s in range(n)] == before
    assert int(bank.fetch_dynamics(0)["frames_out"]) == frames and int(bank.fetch_dynamics(0)["frames_reduced"]) > 0


# ---------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing(torch_dev, omx):
    """every refusal of the bank calls, by arguments the host rejects before any launch"""
    ch, n, cap = 2, 2, 64
    T = compressor(omx).astype(np.int32)
    good = DynamicsCurve(T, 3, 16, 4, 1000)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
    d_in = torch_dev.from_numpy(bursts(1, n * cap, ch).reshape(n, cap, ch)).cuda()
    d_out = torch_dev.full((n, cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    d_tr = torch_dev.full((n, cap), float(SENTINEL), dtype=torch_dev.float32).cuda()

    def refused(f, *a, **k):
        with pytest.raises(capi.OmxError) as e:
            f(*a, **k)
        assert e.value.status == capi.ERR_INVALID, e.value
        return omx.fn("last_error", C.c_char_p, [])().decode()

    # before configure
    assert refused(bank.dynamics, d_in.data_ptr(), cap, d_out.data_ptr(), cap).startswith("program loudness dynamics: ")
    assert refused(bank.reset_dynamics).startswith("program loudness dynamics_reset: ")
    assert refused(bank.fetch_dynamics, 0).startswith("program loudness fetch_dynamics: ")
    # configure
    bad_T = T.copy()
    bad_T[300] = dr.MAX_GAIN + 1
    for curves, channels, index in (([good], 0, None), ([good], 9, None), ([], ch, None), ([good] * 65, ch, None),
                                    ([DynamicsCurve(bad_T, 3, 16, 4, 1000)], ch, None), ([DynamicsCurve(T, 0, 16, 4, 1000)], ch, None),
                                    ([DynamicsCurve(T, 0b100, 16, 4, 1000)], ch, None), ([DynamicsCurve(T, 256, 16, 4, 1000)], 8, None),
                                    ([DynamicsCurve(T, 3, 0, 4, 1000)], ch, None), ([DynamicsCurve(T, 3, 4097, 4, 1000)], ch, None),
                                    ([DynamicsCurve(T, 3, 16, 16385, 1000)], ch, None), ([DynamicsCurve(T, 3, 16, 4, 0)], ch, None),
                                    ([DynamicsCurve(T, 3, 16, 4, dr.MAX_STEP + 1)], ch, None), ([good], ch, [0, 1]), ([good], ch, [0, 0xFFFFFFFE])):
        assert refused(bank.configure_dynamics, curves, channels, index).startswith("program loudness dynamics_configure: ")
    assert refused(bank.dynamics, d_in.data_ptr(), cap, d_out.data_ptr(), cap).startswith("program loudness dynamics: "), "still not configured"
    bank.configure_dynamics([good], ch, [0, DYNAMICS_BYPASS])
    assert refused(bank.fetch_dynamics, n).startswith("program loudness fetch_dynamics: ")
    idle = [bank.fetch_dynamics(s).tobytes() for s in range(n)]
    p_in, p_out, p_tr = d_in.data_ptr(), d_out.data_ptr(), d_tr.data_ptr()
    calls = [dict(d_in=0), dict(d_out=0), dict(frames=[cap + 1, 1]), dict(frames_capacity=2 ** 32, frames=[1, 1]), dict(out_capacity=2 ** 32),
             dict(out_capacity=10), dict(d_out=p_in), dict(d_out=p_in + 8), dict(d_gain_db=p_in), dict(d_key=p_out), dict(d_gain_db=p_out + 4)]
    for change in calls:
        args = dict(d_in=p_in, frames_capacity=cap, d_out=p_out, out_capacity=cap, frames=[cap, cap], flush_mask=None, d_key=0, d_gain_db=p_tr)
        args.update(change)
        assert refused(bank.dynamics, **args).startswith("program loudness dynamics: "), change
    torch_dev.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all() and (d_tr.cpu().numpy() == SENTINEL).all()
    assert [bank.fetch_dynamics(s).tobytes() for s in range(n)] == idle, "a refused call changes no record"
    # a flushed stream takes no frames; the other still does, and a refused call does not advance it
    bank.dynamics(p_in, cap, p_out, cap, frames=[10, 10], flush_mask=[1, 0], d_gain_db=p_tr)
    assert refused(bank.dynamics, p_in, cap, p_out, cap, frames=[1, 1]).startswith("program loudness dynamics: frames for a flushed stream")
    bank.dynamics(p_in, cap, p_out, cap, frames=[0, 5])
    recs = [bank.fetch_dynamics(s) for s in range(n)]
    assert [int(r["frames_in"]) for r in recs] == [10, 15] and [int(r["state"]) for r in recs] == [DYNAMICS_FLUSHED, DYNAMICS_RUNNING]
    assert refused(bank.configure_dynamics, [good], ch).startswith("program loudness dynamics_configure: a stream of the stage holds frames")
    null_records = omx.fn("program_loudness_bank_dynamics", C.c_int, [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3)
    assert null_records(bank._h, p_in, None, cap, None, p_out, None, cap, None, None, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- 9. the C ABI from C99
def test_c99_demo_compresses_a_burst_in_two_cuts(tmp_path, omx):
    exe = build_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout.splitlines()[-1], r.stdout

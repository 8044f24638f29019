"""Programme bank edit pass on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_edit / edit / fetch_edited against the
numpy restatement (tests/program_edit_ref.py, pinned by tests/test_cpu_program_edit.py), which takes the library's curve tables as
data (edit_curve; the tables themselves are checked on the CPU side).

Bars.  Every output float equals the restatement's on bytes.  Every record field is equal, except out_sample_peak_db, which lies
within the family's 1e-4 dB.  d_out is pre-filled with a sentinel: every float at or beyond out_frames[o] * channels keeps it.  d_in has
the same bytes after every call.
Shapes.  With t = edit_plan(channels).tile_frames: lengths, offsets, fades and overlaps of 1, 2, 3, 63, 64, 65, t - 1, t, t + 1 and
3 t + 5 frames, the smallest at which a vector, a tile, their seams, an unaligned row base (rows of an odd number of floats at odd
channel counts) and every relative alignment of a source against the output can go wrong.  No test provokes a fault: the refusals use
only arguments the host rejects before any launch, and no test puts a NaN under two clips."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_edit_ref as er
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (EDIT_CLIP_DTYPE, EDIT_RECORD_DTYPE, EditClip, GainRule, InspectRule, ProgramLoudnessBank, TrimRule,
                                             edit_curve, edit_plan, edit_table, edit_trim)
from test_gpu_program_loudness import torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SIZE = 64
SENTINEL = np.float32(-12345.678)
_TABS = {}


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def tile_of(omx, ch):
    return int(edit_plan(omx, ch)["tile_frames"])


def tabs_of(omx):
    if not _TABS:
        _TABS.update({c: edit_curve(omx, c) for c in er.CURVES})
    return _TABS


def to_api(clips):
    return [EditClip(**c.__dict__) for c in clips]


def run_edit(torch, omx, bank, inputs, clips, out_frames, ch, out_first=None, cap=None, out_cap=None, tag=""):
    """inputs[s]: f32 [frames][ch] of input stream s (the frames of d_in beyond them hold other samples); clips: er.Clip.  Renders,
    checks every bar of the module's docstring against the restatement -> (device pointer to the records, the restatement's outputs,
    its records)"""
    n_in, n_out = len(inputs), len(out_frames)
    frames_in = [len(x) for x in inputs]
    cap = cap or max(max(frames_in), 1)
    out_cap = out_cap or max(out_frames) + 3
    host = er.noise(999, n_in * cap, ch).reshape(n_in, cap, ch)
    for s, x in enumerate(inputs):
        host[s, :len(x)] = x
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n_out, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
    ptr = bank.edit(d_in.data_ptr(), cap, to_api(clips), d_out.data_ptr(), out_cap, out_frames, out_first=out_first, frames_in=frames_in,
                    stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), (tag, "d_in changed")
    got = d_out.cpu().numpy()
    ys, recs = er.render(inputs, clips, out_frames, ch, tabs_of(omx), out_first=out_first)
    for o in range(n_out):
        g, w = got[o, :out_frames[o]], ys[o]
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).any(axis=1))
            raise AssertionError((tag, "output", o, "differs at", len(bad), "frames, first", bad[:6], g[bad[:3]], w[bad[:3]]))
        assert (got[o, out_frames[o]:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), (tag, o, "a float beyond the window was written")
        er.check_record(bank.fetch_edited(o), recs[o], (tag, "record", o))
    return ptr, ys, recs


def hard_values(x):
    """NaN with a payload, both infinities, -0.0 and denormals into the first frames and into a few later ones"""
    flat = x.reshape(-1)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 0.0], np.float32)
    vals.view(np.uint32)[0] = 0x7FA00001
    for i, at in enumerate(list(range(min(7, flat.size))) + [v for v in (1000, 2051, 4099, 8190) if v < flat.size]):
        flat.view(np.uint32)[at] = vals.view(np.uint32)[i % 7]
    return x


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
def test_identity_copies_the_source_bit_for_bit(torch_dev, omx, ch):
    t = tile_of(omx, ch)
    lengths = [0, 1, 3, 1001, t - 1, t, t + 1, 3 * t + 5]
    n = len(lengths)
    bank = new_bank(omx, n, ch)
    bank.configure_edit(ch, n)
    xs = [hard_values(er.noise(10 * ch + s, f, ch, 1.3)) for s, f in enumerate(lengths)]
    clips = [er.Clip(src_stream=s, dst_stream=s, frames=f) for s, f in enumerate(lengths)]
    # rows of 3 t + 5 and 3 t + 9 frames: an odd number of floats at odd channel counts, so rows sit at 4-byte offsets
    _, ys, recs = run_edit(torch_dev, omx, bank, xs, clips, lengths, ch, cap=3 * t + 5, out_cap=3 * t + 9, tag=("identity", ch))
    for s in range(n):
        assert ys[s].tobytes() == xs[s].tobytes()
        assert int(recs[s]["silent_frames"]) == 0 and int(recs[s]["faded_frames"]) == 0 and int(recs[s]["clips"]) == (1 if lengths[s] else 0)


# ---------------------------------------------------------------- 2. offsets
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_every_relative_alignment_of_source_and_output(torch_dev, omx, ch):
    t = tile_of(omx, ch)
    frames = t + 37
    combos = [(s, d) for s in (0, 1, 2, 3, 5) for d in (0, 1, 2, 3, t - 1, t + 1)]
    bank = new_bank(omx, 1, ch)
    bank.configure_edit(ch, len(combos))
    x = er.noise(20 + ch, frames + 5, ch, 1.2)
    clips = [er.Clip(dst_stream=o, src_first=s, dst_first=d, frames=frames, gain=0.75) for o, (s, d) in enumerate(combos)]
    out_frames = [d + frames + 5 for _, d in combos]
    _, ys, recs = run_edit(torch_dev, omx, bank, [x], clips, out_frames, ch, tag=("offsets", ch))
    zero = np.float32(0).tobytes()
    for o, (s, d) in enumerate(combos):
        assert ys[o][:d].tobytes() == zero * (d * ch) and ys[o][d + frames:].tobytes() == zero * (5 * ch)      # +0.0f on bits
        assert int(recs[o]["silent_frames"]) == d + 5


# ---------------------------------------------------------------- 3. fades
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_fades_of_every_length_curve_and_side(torch_dev, omx, ch):
    t = tile_of(omx, ch)
    fades = [1, 2, 3, 63, 64, 65, t - 1, t + 1, 3 * t + 5]
    x = er.noise(30 + ch, 3 * t + 80, ch, 1.1)
    clips = []
    for f in fades:
        for curve in er.CURVES:
            for gain in (1.0, 0.3):
                clips.append(er.Clip(src_first=3, dst_first=1, frames=f + 70, fade_in_frames=f, fade_in_curve=curve, gain=gain))
                clips.append(er.Clip(src_first=2, dst_first=2, frames=f + 70, fade_out_frames=f, fade_out_curve=curve, gain=gain))
    clips.append(er.Clip(src_first=7, frames=5, fade_in_frames=4, fade_out_frames=4, fade_in_curve=1, fade_out_curve=2))      # both factors on three frames
    clips.append(er.Clip(src_first=7, frames=5, fade_in_frames=4, fade_out_frames=4, gain=0.3))
    clips.append(er.Clip(src_first=1, dst_first=3, frames=100, fade_in_frames=100, fade_in_curve=2))      # the whole clip is one fade
    clips.append(er.Clip(src_first=1, dst_first=3, frames=t + 9, fade_out_frames=t + 9, fade_out_curve=1))
    clips.append(er.Clip(src_first=0, dst_first=0, frames=t + 9, fade_in_frames=t + 9, fade_out_frames=t + 9, gain=0.3))      # and two
    for o, c in enumerate(clips):
        c.dst_stream = o
    bank = new_bank(omx, 1, ch)
    bank.configure_edit(ch, len(clips))
    out_frames = [c.dst_first + c.frames + 2 for c in clips]
    _, ys, recs = run_edit(torch_dev, omx, bank, [x], clips, out_frames, ch, tag=("fades", ch))
    for o, c in enumerate(clips[:len(fades) * 12]):
        assert int(recs[o]["faded_frames"]) == max(c.fade_in_frames, c.fade_out_frames)
    assert int(recs[len(fades) * 12]["faded_frames"]) == 5 and int(recs[-1]["faded_frames"]) == t + 9


# ---------------------------------------------------------------- 4. crossfades
@pytest.mark.parametrize("ch", [2, 3])
def test_crossfades(torch_dev, omx, ch):
    t = tile_of(omx, ch)
    a_len = t + 300
    xs = [er.noise(40 + ch, 2 * t + 700, ch, 0.8), er.noise(41 + ch, 2 * t + 700, ch, 0.8)]
    clips = []

    def pair(overlap, b_src_stream, b_gain, curves=(1, 1), a_first=0, a_frames=a_len):
        o = len(clips) // 2
        clips.append(er.Clip(0, o, 5, a_first, a_frames, 0, overlap, 0, curves[0], 0, 0.9))
        clips.append(er.Clip(b_src_stream, o, 11, a_first + a_frames - overlap, overlap + t + 50, overlap, 0, curves[1], 0, 0, b_gain))

    for overlap in (1, 64, t + 1):
        pair(overlap, 1, 0.7)                  # sources from two streams
        pair(overlap, 0, 0.7)                  # and from the same stream
    pair(40, 1, 0.7, a_first=3, a_frames=t + 17)      # an overlap laid across a tile seam: output frames t - 20 .. t + 19
    pair(64, 1, 0.7, curves=(0, 2))            # unequal curves on the two sides
    pair(65, 1, 1.0)                           # the second clip has gain 1: the copy path resumes at the first frame behind the overlap
    pair(t + 1, 0, 1.0, curves=(2, 0))
    n_out = len(clips) // 2
    bank = new_bank(omx, 2, ch)
    bank.configure_edit(ch, n_out)
    out_frames = [clips[2 * o + 1].dst_first + clips[2 * o + 1].frames for o in range(n_out)]
    _, ys, recs = run_edit(torch_dev, omx, bank, xs, clips, out_frames, ch, tag=("crossfades", ch))
    for o in range(n_out):
        a, b = clips[2 * o], clips[2 * o + 1]
        assert int(recs[o]["mixed_frames"]) == b.fade_in_frames == int(recs[o]["faded_frames"]) and int(recs[o]["clips"]) == 2
        if b.gain == 1.0:      # behind the overlap: the source's bits
            behind = b.dst_first + b.fade_in_frames
            src = xs[b.src_stream][b.src_first + b.fade_in_frames:b.src_first + b.frames]
            assert ys[o][behind:].tobytes() == src.tobytes()


# ---------------------------------------------------------------- 5. windows
def test_windows_tile_the_whole(torch_dev, omx):
    ch = 3
    t = tile_of(omx, ch)
    total = 3 * t + 5
    xs = [er.noise(51, 2 * t + 100, ch, 1.05), er.noise(52, 2 * t + 100, ch, 1.05)]
    # a pad of 7 frames, a trimmed clip under two fades, a crossfade of 200 frames into the second clip, which fades out to the end
    a = er.Clip(0, 0, 31, 7, t + 400, 300, 200, 1, 2, 0, 0.8)
    b = er.Clip(1, 0, 13, 7 + t + 200, total - (7 + t + 200), 200, t + 3, 1, 0, 0, 1.0)
    clips = [a, b]
    bank = new_bank(omx, 2, ch)
    bank.configure_edit(ch, 1)
    _, (whole,), (rec,) = run_edit(torch_dev, omx, bank, xs, clips, [total], ch, tag="whole")
    assert int(rec["silent_frames"]) == 7 and int(rec["mixed_frames"]) == 200
    rng = np.random.default_rng(53)
    cuts = sorted(set([0, 1, 63, t, t + 1, total] + [int(v) for v in rng.integers(2, total - 1, 5)]))
    pieces, recs = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _, (y,), (r,) = run_edit(torch_dev, omx, bank, xs, clips, [hi - lo], ch, out_first=[lo], tag=("window", lo, hi))
        pieces.append(y)
        recs.append(bank.fetch_edited(0))
    assert b"".join(p.tobytes() for p in pieces) == whole.tobytes()
    got_whole = run_edit(torch_dev, omx, bank, xs, clips, [total], ch, tag="whole again") and bank.fetch_edited(0)
    for f in er.COUNT_FIELDS:
        assert sum(int(r[f]) for r in recs) == int(got_whole[f]), f
    assert max(np.float32(r["out_sample_peak"]) for r in recs).tobytes() == np.float32(got_whole["out_sample_peak"]).tobytes()
    # a window wholly inside a fade (the second clip's fade-out), and one wholly inside the crossfade
    for lo, n in ((total - t + 10, 100), (7 + t + 250, 33)):
        _, (y,), (r,) = run_edit(torch_dev, omx, bank, xs, clips, [n], ch, out_first=[lo], tag=("inside a fade", lo))
        assert y.tobytes() == whole[lo:lo + n].tobytes() and int(r["faded_frames"]) == n


# ---------------------------------------------------------------- 6. many short clips
def test_many_short_clips_an_empty_output_and_an_empty_clip(torch_dev, omx):
    ch = 3
    rng = np.random.default_rng(61)
    x = er.noise(62, 5000, ch, 1.0)
    clips, at = [], 0
    for k in range(300):
        n = int(rng.integers(1, 8))
        at += int(rng.integers(0, 4))
        fi, fo = (int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1))) if k % 3 == 0 else (0, 0)
        clips.append(er.Clip(0, 0, int(rng.integers(0, 5000 - n)), at, n, fi, fo, k % 3, (k + 1) % 3, 0, [1.0, 0.5, -0.7][k % 3]))
        at += n
    clips.insert(150, er.Clip(0, 0, 4, clips[150].dst_first, 0))      # a clip of 0 frames in the middle of the table
    clips.append(er.Clip(0, 2, 17, 3, 9))                              # output 1 has no clip at all
    bank = new_bank(omx, 1, ch)
    bank.configure_edit(ch, 3)
    _, ys, recs = run_edit(torch_dev, omx, bank, [x], clips, [at + 4, 777, 12], ch, tag="short clips")
    assert int(recs[0]["clips"]) == 300 and int(recs[0]["silent_frames"]) > 100
    assert not ys[1].any() and int(recs[1]["silent_frames"]) == 777 and int(recs[1]["clips"]) == 0
    assert ys[1].tobytes() == np.float32(0).tobytes() * (777 * ch)


# ---------------------------------------------------------------- 7. shapes of the table
def test_shapes_of_the_table(torch_dev, omx):
    ch = 2
    # 12 sources joined into 1 output with crossfades of 100 frames
    xs = [er.noise(70 + s, 900 + 10 * s, ch, 0.6) for s in range(12)]
    clips, at = [], 0
    for s in range(12):
        n = 900 + 10 * s
        clips.append(er.Clip(s, 0, 0, at, n, 100 if s else 0, 100 if s < 11 else 0, 1, 1, 0, 1.0))
        at += n - 100
    total = at + 100
    bank = new_bank(omx, 12, ch)
    bank.configure_edit(ch, 4)
    _, _, (rec,) = run_edit(torch_dev, omx, bank, xs, clips, [total], ch, tag="12 into 1")
    assert int(rec["mixed_frames"]) == 1100 and int(rec["clips"]) == 12 and int(rec["silent_frames"]) == 0
    # 1 source into 3 outputs; the same source range in two clips of one output (a copy with an echo) and in another output
    bank = new_bank(omx, 1, ch)
    bank.configure_edit(ch, 3)
    x = er.noise(90, 3000, ch, 0.5)
    clips = [er.Clip(0, 0, 100, 0, 2000), er.Clip(0, 0, 100, 50, 2000, gain=0.25), er.Clip(0, 1, 100, 0, 2000, 10, 10),
             er.Clip(0, 2, 2999, 5, 1)]
    run_edit(torch_dev, omx, bank, [x], clips, [2050, 2000, 6], ch, tag="1 into 3")


# ---------------------------------------------------------------- 8. records
def test_records_on_the_device_and_before_the_first_call(torch_dev, omx):
    ch = 2
    bank = new_bank(omx, 2, ch)
    bank.configure_edit(ch, 5)
    nothing = np.zeros((), EDIT_RECORD_DTYPE)
    nothing["out_sample_peak_db"] = -99.9
    for o in range(5):      # before the first call: the record of a call that brought nothing
        er.check_record(bank.fetch_edited(o), nothing, ("before the first call", o))
    xs = [er.noise(80, 700, ch, 1.4), er.noise(81, 90, ch, 1.4)]
    clips = [er.Clip(0, 0, 0, 10, 700, 30, 40), er.Clip(1, 0, 0, 690, 90, 20, 0, gain=0.5), er.Clip(1, 2, 5, 0, 50)]
    ptr, _, recs = run_edit(torch_dev, omx, bank, xs, clips, [800, 0, 40], ch, out_first=[5, 3, 20], tag="records")
    assert device_bytes(ptr, 3 * SIZE) == b"".join(bank.fetch_edited(o).tobytes() for o in range(3))
    assert [int(recs[0][f]) for f in ("out_first", "frames", "silent_frames", "faded_frames", "mixed_frames", "clips")] == [5, 800, 30, 70, 20, 2]
    assert int(recs[0]["samples_over"]) > 0 and [int(recs[1][f]) for f in ("out_first", "frames", "clips")] == [3, 0, 0]
    assert [int(recs[2][f]) for f in ("out_first", "frames", "silent_frames", "clips")] == [20, 40, 10, 1]
    er.check_record(bank.fetch_edited(3), nothing, "an output the call did not name")
    # a call whose windows hold no frame writes fresh records and nothing else
    d_out = torch_dev.full((4,), float(SENTINEL), dtype=torch_dev.float32).cuda()
    assert bank.edit(0, 0, [], d_out.data_ptr(), 1, [0, 0]) == ptr
    torch_dev.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all()
    er.check_record(bank.fetch_edited(0), nothing, "a call that brought nothing")


# ---------------------------------------------------------------- 9. slabs
def test_more_outputs_than_one_launch_holds(torch_dev, omx):
    n, ch, length = 70000, 1, 977
    bank = new_bank(omx, 1, ch)
    bank.configure_edit(ch, n)
    x = er.noise(95, length, ch, 1.5)
    table = np.zeros(n, EDIT_CLIP_DTYPE)
    table["dst_stream"] = np.arange(n)
    table["src_first"] = np.arange(n) % length
    table["frames"] = 1
    table["gain"] = np.where(np.arange(n) % 2 == 0, np.float32(1.0), np.float32(0.5))
    d_in = torch_dev.from_numpy(x).cuda()
    d_out = torch_dev.full((n, 2, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    ptr = bank.edit(d_in.data_ptr(), length, table, d_out.data_ptr(), 2, np.ones(n, np.uint32), stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    got = d_out.cpu().numpy()
    want = (x[np.arange(n) % length, 0] * table["gain"]).astype(np.float32)
    assert got[:, 0, 0].tobytes() == want.tobytes() and (got[:, 1, 0] == SENTINEL).all()
    assert d_in.cpu().numpy().tobytes() == x.tobytes()
    recs = np.frombuffer(device_bytes(ptr, n * SIZE), EDIT_RECORD_DTYPE)
    assert (recs["frames"] == 1).all() and (recs["clips"] == 1).all() and not recs["silent_frames"].any() and not recs["out_first"].any()
    assert recs["out_sample_peak"].tobytes() == np.abs(want).tobytes()
    assert (recs["samples_over"] == (np.abs(want) > 1)).all() and recs["samples_over"].sum() > 0
    for o in (0, 65534, 65535, 65536, n - 1):
        assert bank.fetch_edited(o).tobytes() == recs[o].tobytes()
        _, r = er.render_window([x], [er.Clip(0, o, int(o % length), 0, 1, gain=float(table["gain"][o]))], o, 0, 1, ch, tabs_of(omx))
        er.check_record(recs[o], r, ("slab", o))


# ---------------------------------------------------------------- 10. the chain
def test_inspect_trim_edit_process_equals_the_host_trimmed_programme(torch_dev, omx):
    ch, n, body = 2, 2, 30000
    pos = capi.positions_fallback(ch)
    tt = np.arange(body)
    progs = []
    for s in range(n):
        tone = (0.3 * np.sin(2 * np.pi * (440.0 + 300 * s) * tt / 48000.0)).astype(np.float32)
        sig = (tone[:, None] * np.float32(0.9 - 0.2 * s) + np.float32(0.01) * er.noise(100 + s, body, ch)).astype(np.float32)
        sig[sig == 0] = np.float32(1e-3)
        progs.append(np.concatenate([np.zeros((1000, ch), np.float32), sig, np.zeros((500, ch), np.float32)]))
    total = body + 1500
    bank = new_bank(omx, n, ch)
    bank.configure_inspect(InspectRule(), ch, [])
    d_in = torch_dev.from_numpy(np.stack(progs)).cuda()
    bank.inspect(d_in.data_ptr(), total, stream=stream_of(torch_dev))
    clips = []
    for s in range(n):
        rec = bank.fetch_inspected(s)
        assert int(rec["leading_silence"]) == 1000 and int(rec["trailing_silence"]) == 500
        clip, out = edit_trim(omx, rec, TrimRule(), s, s)
        assert (clip.src_first, clip.frames, out) == (1000, body, body)
        clips.append(clip)
    bank.configure_edit(ch, n)
    d_out = torch_dev.full((n, body, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.edit(d_in.data_ptr(), total, clips, d_out.data_ptr(), body, [body] * n, stream=stream_of(torch_dev))
    bank.process(d_out.data_ptr(), body, ch, 48000.0, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    trimmed = np.stack([p[1000:-500] for p in progs])
    assert d_out.cpu().numpy().tobytes() == trimmed.tobytes()
    other = new_bank(omx, n, ch)
    d_host_trimmed = torch_dev.from_numpy(trimmed).cuda()
    other.process(d_host_trimmed.data_ptr(), body, ch, 48000.0, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    for s in range(n):
        assert record_array(bank.fetch(s)).tobytes() == record_array(other.fetch(s)).tobytes()
        assert bank.fetch(s).integrated_lufs > -40.0


# ---------------------------------------------------------------- 11. nothing else moves
def test_edit_leaves_the_records_of_the_earlier_headers_alone(torch_dev, omx):
    ch, n, frames = 2, 3, 22051
    pos = capi.positions_fallback(ch)
    bank = new_bank(omx, n)
    tt = np.arange(frames)
    tone = (0.2 * np.sin(2 * np.pi * 997.0 * tt / 48000.0) * ((tt // 9000) % 2 + 1) / 2.0).astype(np.float32)
    x = np.stack([tone[:, None] * np.float32(0.9 - 0.1 * s) + np.float32(0.01) * er.noise(110 + s, frames, ch) for s in range(n)]).astype(np.float32)
    d_some = torch_dev.from_numpy(x).cuda()
    d_tmp = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.set_peaks(True)
    bank.process(d_some.data_ptr(), frames, ch, 48000.0, pos, stream=stream_of(torch_dev))
    gains = bank.plan_gains(GainRule(-20.0, -1.0, -60.0, 60.0, 0), stream=stream_of(torch_dev))
    bank.apply_gains(d_some.data_ptr(), d_tmp.data_ptr(), frames, ch, gains, n, stream=stream_of(torch_dev))
    bank.configure_inspect(InspectRule(), ch, [(0, 1)])
    bank.inspect(d_some.data_ptr(), frames, stream=stream_of(torch_dev))
    bank.configure_remix(np.array([[0.5, 0.5]], np.float32), ch, 1)
    d_mono = torch_dev.zeros((n, frames, 1), dtype=torch_dev.float32).cuda()
    bank.remix(d_some.data_ptr(), d_mono.data_ptr(), frames, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()

    def state():
        return ([record_array(bank.fetch(s)).tobytes() for s in range(n)], [bank.fetch_peaks(s).tobytes() for s in range(n)],
                [bank.fetch_inspected(s).tobytes() for s in range(n)], [bank.fetch_remixed(s).tobytes() for s in range(n)],
                [bank.fetch_applied(s).tobytes() for s in range(n)], bank.fetch_gains().tobytes(),
                [bank.fetch_segments(s).tobytes() for s in range(n)])

    before = state()
    bank.configure_edit(ch, 2)
    clips = [er.Clip(0, 0, 100, 0, 9000, 480, 480, 1, 1), er.Clip(1, 0, 0, 8520, 9000, 480, 0, 1, 0), er.Clip(2, 1, 50, 24, 5000, gain=0.5)]
    run_edit(torch_dev, omx, bank, [x[s] for s in range(n)], clips, [17520, 5100], ch, tag="beside the other stages")
    assert state() == before, "a call of program_edit.h changed a record of an earlier header"
    assert d_some.cpu().numpy().tobytes() == x.tobytes()


def test_refused_calls_change_nothing(torch_dev, omx):
    ch, n, cap, out_cap = 2, 2, 400, 500
    x = np.stack([er.noise(120 + s, cap, ch) for s in range(n)])
    d_x = torch_dev.from_numpy(x).cuda()
    d_y = torch_dev.full((3, out_cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank = new_bank(omx, n)
    table = [EditClip(0, 0, 0, 0, 300, 10, 10), EditClip(1, 0, 0, 290, 200, 10, 0), EditClip(0, 1, 100, 5, 40)]
    good = dict(d_in=d_x.data_ptr(), frames_capacity=cap, clips=table, d_out=d_y.data_ptr(), out_capacity=out_cap, out_frames=[490, 45, 7])

    def last_error():
        return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")

    def refused(call, tag):
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        assert last_error().startswith("program loudness edit: "), (tag, last_error())

    refused(lambda: bank.edit(**good), "before configure")
    with pytest.raises(capi.OmxError):
        bank.fetch_edited(0)
    for channels, outputs in ((0, 3), (9, 3), (2, 0), (2, 2 ** 24 + 1)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_edit(channels, outputs)
        assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError):
        bank.fetch_edited(0)                                         # a refused configure configured nothing
    bank.configure_edit(ch, 3)
    ptr = bank.edit(**good, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    y = d_y.cpu().numpy().copy()
    records = device_bytes(ptr, 3 * SIZE)
    assert [int(bank.fetch_edited(o)["frames"]) for o in range(3)] == [490, 45, 7] and (y[0, :490] != SENTINEL).all()

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert d_x.cpu().numpy().tobytes() == x.tobytes(), tag
        assert d_y.cpu().numpy().tobytes() == y.tobytes(), tag
        assert device_bytes(ptr, 3 * SIZE) == records, tag

    def table_with(k, **kw):
        out = [EditClip(**c.__dict__) for c in table]
        for f, v in kw.items():
            setattr(out[k], f, v)
        return out

    x_bytes = cap * ch * 4
    bad_calls = {"n_out of 0": dict(out_frames=[], clips=[]),
                 "n_out above max_outputs": dict(out_frames=[1, 1, 1, 1]),
                 "an unsorted table": dict(clips=[table[1], table[0], table[2]]),
                 "a triple overlap": dict(clips=table[:2] + [EditClip(0, 0, 0, 295, 10), table[2]]),
                 "a clip beyond frames_in": dict(frames_in=[299, cap]),
                 "a clip beyond the row": dict(clips=table_with(1, frames=401, dst_first=0, fade_in_frames=0)),
                 "frames_in beyond the row": dict(frames_in=[cap + 1, cap]),
                 "a bad curve": dict(clips=table_with(0, fade_out_curve=3)),
                 "non-zero flags": dict(clips=table_with(2, flags=2)),
                 "a NaN gain": dict(clips=table_with(2, gain=float("nan"))),
                 "a fade longer than the clip": dict(clips=table_with(2, fade_in_frames=41)),
                 "src_stream out of range": dict(clips=table_with(2, src_stream=2)),
                 "dst_stream out of range": dict(clips=table_with(2, dst_stream=3)),
                 "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32),
                 "out_capacity beyond 2^32 - 1": dict(out_capacity=2 ** 32),
                 "out_frames beyond out_capacity": dict(out_frames=[out_cap + 1, 45, 7]),
                 "out_first + out_frames beyond 2^40": dict(out_first=[2 ** 40 - 489, 0, 0]),
                 "d_in inside d_out": dict(d_in=d_y.data_ptr() + 3 * out_cap * ch * 4 - 4),
                 "d_out inside d_in": dict(d_out=d_x.data_ptr() + n * x_bytes - 4),
                 "d_in == d_out": dict(d_out=d_x.data_ptr()),
                 "null d_in": dict(d_in=0),
                 "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        refused(lambda: bank.edit(**{**good, **change}), tag)
        unchanged(tag)
    raw = omx.fn("program_loudness_bank_edit", C.c_int,
                 [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p])
    rows, counts, out_ptr = edit_table(table), np.array([490, 45, 7], np.uint32), C.c_void_p()
    args = [bank._h, C.c_void_p(d_x.data_ptr()), cap, None, rows.ctypes.data, 3, C.c_void_p(d_y.data_ptr()), out_cap, 3, None, counts.ctypes.data,
            None, C.addressof(out_ptr)]
    for k, tag in ((4, "null clips"), (10, "null out_frames"), (12, "null d_edited")):
        assert raw(*[None if i == k else a for i, a in enumerate(args)]) == capi.ERR_INVALID, tag
        assert last_error().startswith("program loudness edit: "), (tag, last_error())
        unchanged(tag)
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_edited(3)
    assert err.value.status == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_fetch_edited", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(bank._h, 0, None) == capi.ERR_INVALID
    unchanged("refused fetches")
    # windows at the far end of the range are accepted: nothing but zeros lies there
    assert bank.edit(**{**good, "out_first": [2 ** 40 - 490, 0, 0]}, stream=stream_of(torch_dev)) == ptr
    torch_dev.cuda.synchronize()
    far = d_y.cpu().numpy()
    assert far[0, :490].tobytes() == np.float32(0).tobytes() * (490 * ch) and far[1:].tobytes() == y[1:].tobytes()
    assert int(bank.fetch_edited(0)["silent_frames"]) == 490 and int(bank.fetch_edited(0)["out_first"]) == 2 ** 40 - 490


# ---------------------------------------------------------------- 12. the C99 demo
def demo_tracks():
    """tests/c_abi/program_edit_demo.c's two tracks: f32 [2][24000][2]"""
    tracks, frames, ch, state = 2, 24000, 2, 2025
    out = np.zeros((tracks, frames, ch), np.float32)
    lead, trail = (1000, 300), (500, 700)
    for t in range(tracks):
        for f in range(frames):
            for c in range(ch):
                state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
                v = ((state >> 8) & 0xFFFFFF) - 8388608
                if lead[t] <= f < frames - trail[t]:
                    out[t, f, c] = np.float32(0.25) if v == 0 else np.float32(v) / np.float32(33554432.0)
    return out


def test_c99_demo_prints_the_restatements_record(torch_dev, omx, tmp_path):
    """tests/c_abi/program_edit_demo.c: two tracks inspected, trimmed where the silence lies and joined with a crossfade, from a plain C
    host"""
    from test_cpu_program_edit import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], words[1::2]))
    x = demo_tracks()
    rule = er.Trim(fade_in_frames=480, fade_out_frames=480, fade_in_curve=1, fade_out_curve=1)
    clips = []
    for t, (lead, trail) in enumerate(((1000, 500), (300, 700))):
        clip, kept = er.trim({"frames": 24000, "leading_silence": lead, "trailing_silence": trail}, rule, t, 0)
        assert kept == 24000 - lead - trail
        clips.append(clip)
    clips[1].dst_first = clips[0].frames - 480
    (total,) = er.extent(clips, [24000, 24000], 1)
    (y,), (rec,) = er.render([x[0], x[1]], clips, [total], 2, tabs_of(omx))
    want = {"tile": tile_of(omx, 2), "src_first_0": 1000, "frames_0": 22500, "src_first_1": 300, "frames_1": 23000, "dst_first_1": 22020,
            "fade_in_0": 480, "fade_out_1": 480, "extent": 45020, "out_first": 0, "frames": 45020, "silent_frames": 0,
            "faded_frames": 480 * 3, "mixed_frames": 480, "samples_over": int(rec["samples_over"]), "clips": 2,
            "peak_bits": int(np.float32(rec["out_sample_peak"]).view(np.uint32)), "first_bits": int(y[0, 1].view(np.uint32)),
            "crossfade_bits": int(y[22027, 1].view(np.uint32)), "last_bits": int(y[total - 1, 1].view(np.uint32))}
    for key, value in want.items():
        assert int(out[key]) == int(value), (key, out[key], value)
    assert int(rec["faded_frames"]) == 1440 and int(rec["mixed_frames"]) == 480 and int(rec["frames"]) == 45020
    assert abs(float(out["peak_db"]) - float(rec["out_sample_peak_db"])) <= 1e-4

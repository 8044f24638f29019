"""Programme bank mix pass on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_mix / mix / fetch_mixed against the
numpy restatement (tests/program_mix_ref.py, pinned by tests/test_cpu_program_mix.py).

Bars.  Every output float equals the restatement's on bytes (a NaN where the restatement has a NaN: the bits of a NaN are not
defined).  Every record field is equal, except out_sample_peak_db, which lies within the family's 1e-4 dB.  d_out is pre-filled with a
sentinel: every float at or beyond out_frames[o] * channels keeps it.  d_in has the same bytes after every call.
Shapes.  With t = mix_plan(channels).tile_frames and B = layers_per_batch: lengths, offsets and staggers of 1, 2, 3, 63, 64, 65, t - 1,
t, t + 1 and 3 t + 5 frames and depths of 1, 2, 3, B - 1, B, B + 1, 2 B + 1 and 64 layers, the smallest at which a vector, a tile, a
batch, their seams, an unaligned row base (rows of an odd number of floats at odd channel counts) and every relative alignment of a
source against the output can go wrong.  No test provokes a fault: the refusals use only arguments the host rejects before any
launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_mix_ref as mr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (MIX_RECORD_DTYPE, MIX_SEND_DTYPE, EditClip, MixSend, ProgramLoudnessBank, mix_null, mix_plan,
                                             mix_table)
from test_gpu_program_loudness import torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SIZE = 64
SENTINEL = np.float32(-12345.678)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def plan_of(omx, ch):
    info = mix_plan(omx, ch)
    return int(info["tile_frames"]), int(info["layers_per_batch"])


def to_api(sends):
    return [MixSend(**s.__dict__) for s in sends]


def run_mix(torch, omx, bank, inputs, sends, out_frames, ch, out_first=None, cap=None, out_cap=None, tag=""):
    """inputs[s]: f32 [frames][ch] of input stream s (the frames of d_in beyond them hold other samples); sends: mr.Send.  Renders,
    checks every bar of the module's docstring against the restatement -> (device pointer to the records, the restatement's outputs,
    its records)"""
    n_in, n_out = len(inputs), len(out_frames)
    frames_in = [len(x) for x in inputs]
    cap = cap or max(max(frames_in), 1)
    out_cap = out_cap or max(out_frames) + 3
    host = mr.noise(999, n_in * cap, ch).reshape(n_in, cap, ch)
    for s, x in enumerate(inputs):
        host[s, :len(x)] = x
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n_out, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
    ptr = bank.mix(d_in.data_ptr(), cap, to_api(sends), d_out.data_ptr(), out_cap, out_frames, out_first=out_first, frames_in=frames_in,
                   stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), (tag, "d_in changed")
    got = d_out.cpu().numpy()
    ys, recs = mr.render(inputs, sends, out_frames, ch, out_first=out_first)
    for o in range(n_out):
        g, w = got[o, :out_frames[o]], ys[o]
        if not mr.same_bytes_nan_as_nan(g, w):
            differs = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
            bad = np.flatnonzero(differs.any(axis=1))
            raise AssertionError((tag, "bus", o, "differs at", len(bad), "frames, first", bad[:6], g[bad[:3]], w[bad[:3]]))
        assert (got[o, out_frames[o]:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), (tag, o, "a float beyond the window was written")
        mr.check_record(bank.fetch_mixed(o), recs[o], (tag, "record", o))
    return ptr, ys, recs


def hard_values(x, with_nan=False):
    """both infinities, -0.0 and denormals (and a NaN with a payload) into the first frames and into a few later ones"""
    flat = x.reshape(-1)
    vals = np.array([np.inf, -np.inf, -0.0, 1e-45, -1e-40, 0.0, 1e-39, np.nan], np.float32)
    vals.view(np.uint32)[7] = 0x7FA00001
    k = 8 if with_nan else 7
    for i, at in enumerate(list(range(min(k, flat.size))) + [v for v in (1000, 2051, 4099, 8190) if v < flat.size]):
        flat.view(np.uint32)[at] = vals.view(np.uint32)[i % k]
    return x


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
def test_identity_keeps_the_bits_of_the_source(torch_dev, omx, ch):
    t, _ = plan_of(omx, ch)
    lengths = [0, 1, 3, 1001, t - 1, t, t + 1, 3 * t + 5]
    n = len(lengths)
    bank = new_bank(omx, n, ch)
    bank.configure_mix(ch, n)
    xs = [hard_values(mr.noise(10 * ch + s, f, ch, 1.3)) for s, f in enumerate(lengths)]
    sends = [mr.Send(src_stream=s, dst_bus=s, frames=f) for s, f in enumerate(lengths)]
    # rows of an odd number of frames (3 t + 5, or 1001 where the tile is short): an odd number of floats at odd channel counts, so
    # rows sit at 4-byte offsets
    cap = max(lengths)
    _, ys, recs = run_mix(torch_dev, omx, bank, xs, sends, lengths, ch, cap=cap, out_cap=cap + 4, tag=("identity", ch))
    for s in range(n):
        assert ys[s].tobytes() == xs[s].tobytes()
        assert int(recs[s]["silent_frames"]) == 0 and int(recs[s]["mixed_frames"]) == 0 and int(recs[s]["sends"]) == (1 if lengths[s] else 0)
        assert int(recs[s]["max_layers"]) == (1 if lengths[s] else 0)


# ---------------------------------------------------------------- 2. alignment
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_every_relative_alignment_of_source_and_output(torch_dev, omx, ch):
    t, _ = plan_of(omx, ch)
    frames = t + 37
    combos = [(s, d) for s in (0, 1, 2, 3, 5) for d in (0, 1, 2, 3, t - 1, t + 1)]
    bank = new_bank(omx, 1, ch)
    bank.configure_mix(ch, len(combos))
    x = mr.noise(20 + ch, frames + 6, ch, 1.2)
    sends = []
    for o, (s, d) in enumerate(combos):      # two layers one frame apart in the source: different alignments in one span
        sends.append(mr.Send(0, o, s, d, frames, 0.75))
        sends.append(mr.Send(0, o, s + 1, d, frames, -0.5))
    out_frames = [d + frames + 5 for _, d in combos]
    _, ys, recs = run_mix(torch_dev, omx, bank, [x], sends, out_frames, ch, tag=("alignment", ch))
    zero = np.float32(0).tobytes()
    for o, (s, d) in enumerate(combos):
        assert ys[o][:d].tobytes() == zero * (d * ch) and ys[o][d + frames:].tobytes() == zero * (5 * ch)      # +0.0f on bits
        assert int(recs[o]["silent_frames"]) == d + 5 and int(recs[o]["mixed_frames"]) == frames and int(recs[o]["max_layers"]) == 2


# ---------------------------------------------------------------- 3. depth
@pytest.mark.parametrize("ch", [2, 3])
def test_depths_around_the_batch_with_staggered_starts(torch_dev, omx, ch):
    t, b = plan_of(omx, ch)
    depths = sorted(set([1, 2, 3, b - 1, b, b + 1, 2 * b + 1, 64]))
    stagger = [1, 63, 64, 65, t + 1]
    starts = np.concatenate([[0], np.cumsum([stagger[i % 5] for i in range(63)])]).astype(int)
    gains = [1.0, -0.5, 0.3, 0.7, -1.0]
    n_in = 4
    longest = int(starts[-1]) + t + 10
    xs = [mr.noise(30 + ch + s, longest + 7, ch, 0.9) for s in range(n_in)]
    sends, out_frames = [], []
    for o, depth in enumerate(depths):
        length = int(starts[depth - 1]) + t + 10      # every layer still runs where the last one starts
        for i in range(depth):
            sends.append(mr.Send(i % n_in, o, i % 7, int(starts[i]), length, gains[i % 5]))
        out_frames.append(int(starts[depth - 1]) + length)
    bank = new_bank(omx, n_in, ch)
    bank.configure_mix(ch, len(depths))
    _, _, recs = run_mix(torch_dev, omx, bank, xs, sends, out_frames, ch, tag=("depth", ch))
    assert [int(r["max_layers"]) for r in recs] == depths and [int(r["sends"]) for r in recs] == depths
    assert all(int(r["silent_frames"]) == 0 for r in recs)


# ---------------------------------------------------------------- 4. order and width
def test_order_of_the_sum_and_width_of_the_accumulator(torch_dev, omx):
    ch = 1
    t, b = plan_of(omx, ch)
    frames = t + 5      # a head, a body and a tail of constant samples: every float of the bus is the case's figure
    cases = [([2.0 ** 60, 1.0, -2.0 ** 60], 0.0), ([2.0 ** 60, -2.0 ** 60, 1.0], 1.0), ([2.0 ** 30, 1.0, -2.0 ** 30], 1.0),
             ([1.0] + [2.0 ** -25] * 4, np.uint32(0x3F800001).view(np.float32)),
             ([2.0 ** 60, 1.0] + [0.0] * (b - 2) + [-2.0 ** 60], 0.0),      # depth B + 1: the cancelling pair in two batches
             ([2.0 ** 60, 1.0] + [0.0] * 61 + [-2.0 ** 60], 0.0)]           # depth 64: in the first batch and the last
    values = sorted(set(v for samples, _ in cases for v in samples))
    xs = [np.full((frames, ch), v, np.float32) for v in values]
    sends = [mr.Send(values.index(v), o, 0, 0, frames, 1.0) for o, (samples, _) in enumerate(cases) for v in samples]
    bank = new_bank(omx, len(values), ch)
    bank.configure_mix(ch, len(cases))
    _, ys, recs = run_mix(torch_dev, omx, bank, xs, sends, [frames] * len(cases), ch, tag="order and width")
    for o, (samples, want) in enumerate(cases):
        assert ys[o].tobytes() == np.full((frames, ch), want, np.float32).tobytes(), (o, ys[o][0], want)
        assert int(recs[o]["max_layers"]) == len(samples)


# ---------------------------------------------------------------- 5. against edit
def test_a_table_without_overlaps_equals_edit_on_bytes(torch_dev, omx):
    ch = 3
    t, _ = plan_of(omx, ch)
    x = [hard_values(mr.noise(50, 2 * t + 100, ch, 1.1)), mr.noise(51, 2 * t + 100, ch, 1.1)]
    pieces = [(0, 5, 0, t + 9, 0.3), (1, 0, t + 9, 77, -1.0), (0, 31, t + 100, t + 1, 1.0), (1, 3, 2 * t + 101, 64, 0.3), (1, 2, 2 * t + 170, 1, -1.0)]
    total = 2 * t + 180
    bank = new_bank(omx, 2, ch)
    bank.configure_mix(ch, 1)
    bank.configure_edit(ch, 1)
    sends = [mr.Send(s, 0, sf, df, n, g) for s, sf, df, n, g in pieces]
    run_mix(torch_dev, omx, bank, x, sends, [total], ch, tag="beside edit")
    host = np.stack(x)
    d_in = torch_dev.from_numpy(host).cuda()
    d_mix = torch_dev.full((1, total + 3, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    d_edit = torch_dev.full((1, total + 3, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.mix(d_in.data_ptr(), 2 * t + 100, to_api(sends), d_mix.data_ptr(), total + 3, [total], stream=stream_of(torch_dev))
    bank.edit(d_in.data_ptr(), 2 * t + 100, [EditClip(s, 0, sf, df, n, gain=g) for s, sf, df, n, g in pieces], d_edit.data_ptr(), total + 3, [total],
              stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert d_mix.cpu().numpy().tobytes() == d_edit.cpu().numpy().tobytes()
    m, e = bank.fetch_mixed(0), bank.fetch_edited(0)
    for f in ("out_first", "frames", "silent_frames", "samples_over"):
        assert int(m[f]) == int(e[f]), f
    assert np.float32(m["out_sample_peak"]).tobytes() == np.float32(e["out_sample_peak"]).tobytes() and int(m["sends"]) == int(e["clips"]) == 5


# ---------------------------------------------------------------- 6. windows
def test_windows_tile_the_whole(torch_dev, omx):
    ch = 3
    t, b = plan_of(omx, ch)
    total = 3 * t + 5
    xs = [mr.noise(60 + s, total + 20, ch, 1.05) for s in range(3)]
    sends = [mr.Send(0, 0, 3, 7, total - 7, 0.8), mr.Send(1, 0, 0, 7, t + 400, -0.6), mr.Send(2, 0, 13, 70, 2 * t, 1.0),
             mr.Send(0, 0, 1, t - 1, 66, 0.25), mr.Send(1, 0, 9, t + 1, t, 0.5), mr.Send(2, 0, 0, t + 1, 3, -1.0),
             mr.Send(1, 0, 5, 2 * t + 63, t - 80, 0.9)]
    bank = new_bank(omx, 3, ch)
    bank.configure_mix(ch, 1)
    _, (whole,), (rec,) = run_mix(torch_dev, omx, bank, xs, sends, [total], ch, tag="whole")
    assert int(rec["silent_frames"]) == 7 and int(rec["max_layers"]) == 6 and int(rec["sends"]) == 7
    rng = np.random.default_rng(63)
    cuts = sorted(set([0, 1, 63, t, t + 1, total] + [int(v) for v in rng.integers(2, total - 1, 5)]))
    pieces, recs = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _, (y,), (r,) = run_mix(torch_dev, omx, bank, xs, sends, [hi - lo], ch, out_first=[lo], tag=("window", lo, hi))
        pieces.append(y)
        recs.append(bank.fetch_mixed(0))
    assert b"".join(p.tobytes() for p in pieces) == whole.tobytes()
    got_whole = run_mix(torch_dev, omx, bank, xs, sends, [total], ch, tag="whole again") and bank.fetch_mixed(0)
    for f in mr.COUNT_FIELDS:
        assert sum(int(r[f]) for r in recs) == int(got_whole[f]), f
    assert max(np.float32(r["out_sample_peak"]) for r in recs).tobytes() == np.float32(got_whole["out_sample_peak"]).tobytes()
    assert max(int(r["max_layers"]) for r in recs) == int(got_whole["max_layers"])


# ---------------------------------------------------------------- 7. shapes of the table
def test_many_short_sends_an_empty_bus_and_an_empty_send(torch_dev, omx):
    ch = 3
    rng = np.random.default_rng(71)
    x = mr.noise(72, 5000, ch, 1.0)
    sends, at = [], 0
    for k in range(300):
        n = int(rng.integers(1, 8))
        at += int(rng.integers(0, 5))
        sends.append(mr.Send(0, 0, int(rng.integers(0, 5000 - n)), at, n, [1.0, 0.5, -0.7][k % 3]))
    end = max(s.dst_first + s.frames for s in sends)
    sends.insert(150, mr.Send(0, 0, 4, sends[150].dst_first, 0))      # a send of 0 frames in the middle of the table
    sends.append(mr.Send(0, 2, 17, 3, 9))                              # bus 1 has no send at all
    bank = new_bank(omx, 1, ch)
    bank.configure_mix(ch, 3)
    _, ys, recs = run_mix(torch_dev, omx, bank, [x], sends, [end + 4, 777, 12], ch, tag="short sends")
    assert int(recs[0]["sends"]) == 300 and int(recs[0]["mixed_frames"]) > 100 and int(recs[0]["max_layers"]) >= 3
    assert not ys[1].any() and int(recs[1]["silent_frames"]) == 777 and int(recs[1]["sends"]) == 0 and int(recs[1]["max_layers"]) == 0
    assert ys[1].tobytes() == np.float32(0).tobytes() * (777 * ch)


def test_many_sources_into_one_bus_and_one_source_into_many(torch_dev, omx):
    ch = 2
    xs = [mr.noise(80 + s, 900 + 10 * s, ch, 0.3) for s in range(12)]
    sends = [mr.Send(s, 0, 0, 0, 900 + 10 * s, 1.0 - 0.1 * s) for s in range(12)]
    bank = new_bank(omx, 12, ch)
    bank.configure_mix(ch, 4)
    _, _, (rec,) = run_mix(torch_dev, omx, bank, xs, sends, [1010], ch, tag="12 into 1")
    assert int(rec["mixed_frames"]) == 1000 and int(rec["sends"]) == 12 and int(rec["max_layers"]) == 12 and int(rec["silent_frames"]) == 0
    bank = new_bank(omx, 1, ch)
    bank.configure_mix(ch, 3)
    x = mr.noise(95, 3000, ch, 0.5)
    sends = [mr.Send(0, 0, 100, 0, 2000), mr.Send(0, 0, 100, 50, 2000, 0.25), mr.Send(0, 1, 100, 0, 2000, -1.0), mr.Send(0, 2, 2999, 5, 1)]
    run_mix(torch_dev, omx, bank, [x], sends, [2050, 2000, 6], ch, tag="1 into 3")


def test_records_on_the_device_and_before_the_first_call(torch_dev, omx):
    ch = 2
    bank = new_bank(omx, 2, ch)
    bank.configure_mix(ch, 5)
    nothing = np.zeros((), MIX_RECORD_DTYPE)
    nothing["out_sample_peak_db"] = -99.9
    for o in range(5):      # before the first call: the record of a call that brought nothing
        mr.check_record(bank.fetch_mixed(o), nothing, ("before the first call", o))
    xs = [mr.noise(100, 700, ch, 1.4), mr.noise(101, 90, ch, 1.4)]
    sends = [mr.Send(0, 0, 0, 10, 700), mr.Send(1, 0, 0, 690, 90, 0.5), mr.Send(1, 2, 5, 0, 50)]
    ptr, _, recs = run_mix(torch_dev, omx, bank, xs, sends, [800, 0, 40], ch, out_first=[5, 3, 20], tag="records")
    assert device_bytes(ptr, 3 * SIZE) == b"".join(bank.fetch_mixed(o).tobytes() for o in range(3))
    assert [int(recs[0][f]) for f in ("out_first", "frames", "silent_frames", "mixed_frames", "sends", "max_layers")] == [5, 800, 30, 20, 2, 2]
    assert int(recs[0]["samples_over"]) > 0 and [int(recs[1][f]) for f in ("out_first", "frames", "sends")] == [3, 0, 0]
    assert [int(recs[2][f]) for f in ("out_first", "frames", "silent_frames", "sends")] == [20, 40, 10, 1]
    mr.check_record(bank.fetch_mixed(3), nothing, "a bus the call did not name")
    # a call whose windows hold no frame writes fresh records and nothing else
    d_out = torch_dev.full((4,), float(SENTINEL), dtype=torch_dev.float32).cuda()
    assert bank.mix(0, 0, [], d_out.data_ptr(), 1, [0, 0]) == ptr
    torch_dev.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all()
    mr.check_record(bank.fetch_mixed(0), nothing, "a call that brought nothing")


def test_more_buses_than_one_launch_holds(torch_dev, omx):
    n, ch, length = 70000, 1, 977
    bank = new_bank(omx, 1, ch)
    bank.configure_mix(ch, n)
    x = mr.noise(105, length, ch, 1.5)
    table = np.zeros(n, MIX_SEND_DTYPE)
    table["dst_bus"] = np.arange(n)
    table["src_first"] = np.arange(n) % length
    table["frames"] = 1
    table["gain"] = np.where(np.arange(n) % 2 == 0, np.float32(1.0), np.float32(-0.5))
    d_in = torch_dev.from_numpy(x).cuda()
    d_out = torch_dev.full((n, 2, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    ptr = bank.mix(d_in.data_ptr(), length, table, d_out.data_ptr(), 2, np.ones(n, np.uint32), stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    got = d_out.cpu().numpy()
    want = (x[np.arange(n) % length, 0] * table["gain"]).astype(np.float32)      # one exact product rounded once: the f32 product
    assert got[:, 0, 0].tobytes() == want.tobytes() and (got[:, 1, 0] == SENTINEL).all()
    assert d_in.cpu().numpy().tobytes() == x.tobytes()
    recs = np.frombuffer(device_bytes(ptr, n * SIZE), MIX_RECORD_DTYPE)
    assert (recs["frames"] == 1).all() and (recs["sends"] == 1).all() and (recs["max_layers"] == 1).all()
    assert not recs["silent_frames"].any() and not recs["out_first"].any() and not recs["samples_nonfinite"].any()
    assert recs["out_sample_peak"].tobytes() == np.abs(want).tobytes()
    assert (recs["samples_over"] == (np.abs(want) > 1)).all() and recs["samples_over"].sum() > 0
    for o in (0, 65534, 65535, 65536, n - 1):
        assert bank.fetch_mixed(o).tobytes() == recs[o].tobytes()
        _, r = mr.render_window([x], [mr.Send(0, o, int(o % length), 0, 1, float(table["gain"][o]))], o, 0, 1, ch)
        mr.check_record(recs[o], r, ("slab", o))


# ---------------------------------------------------------------- 8. the null test
def test_null_test_of_a_lattice_leaves_exactly_nothing(torch_dev, omx):
    ch, frames = 2, 12000
    stems, pm = mr.lattice(110, frames, ch, 3)
    table = mix_null(omx, [0, 1, 2], 3, frames, 0)
    sends = [mr.Send(*[int(r[f]) for f in MIX_SEND_DTYPE.names[:5]], float(r["gain"]), int(r["flags"])) for r in table]
    bank = new_bank(omx, 4, ch)
    bank.configure_mix(ch, 1)
    _, (y,), (rec,) = run_mix(torch_dev, omx, bank, stems + [pm], sends, [frames], ch, tag="null test")
    got = bank.fetch_mixed(0)
    assert y.tobytes() == np.zeros((frames, ch), np.float32).tobytes()
    assert float(got["out_sample_peak"]) == 0.0 and int(got["max_layers"]) == 4 and np.float32(got["out_sample_peak_db"]) == np.float32(-99.9)
    assert int(got["mixed_frames"]) == frames and int(got["samples_nonfinite"]) == 0
    stems[1][777, 1] += np.float32(2.0 ** -16)
    run_mix(torch_dev, omx, bank, stems + [pm], sends, [frames], ch, tag="null test, one step off")
    assert float(bank.fetch_mixed(0)["out_sample_peak"]) == 2.0 ** -16


# ---------------------------------------------------------------- 9. the chain
def test_mix_then_process_equals_a_bank_fed_the_restatements_pcm(torch_dev, omx):
    ch, n, body = 2, 2, 30000
    pos = capi.positions_fallback(ch)
    tt = np.arange(body)
    xs = []
    for s in range(n):
        tone = (0.3 * np.sin(2 * np.pi * (440.0 + 300 * s) * tt / 48000.0)).astype(np.float32)
        xs.append((tone[:, None] * np.float32(0.9 - 0.2 * s) + np.float32(0.01) * mr.noise(120 + s, body, ch)).astype(np.float32))
    sends = [mr.Send(0, 0, 0, 0, body, 1.0), mr.Send(1, 0, 0, 0, body, 0.5), mr.Send(0, 1, 0, 0, body, -0.25), mr.Send(1, 1, 0, 0, body, 1.0)]
    bank = new_bank(omx, n, ch)
    bank.configure_mix(ch, n)
    d_in = torch_dev.from_numpy(np.stack(xs)).cuda()
    d_out = torch_dev.full((n, body, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.mix(d_in.data_ptr(), body, to_api(sends), d_out.data_ptr(), body, [body] * n, stream=stream_of(torch_dev))
    bank.process(d_out.data_ptr(), body, ch, 48000.0, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    ys, _ = mr.render(xs, sends, [body] * n, ch)
    want = np.stack(ys)
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    other = new_bank(omx, n, ch)
    d_want = torch_dev.from_numpy(want).cuda()
    other.process(d_want.data_ptr(), body, ch, 48000.0, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    for s in range(n):
        assert record_array(bank.fetch(s)).tobytes() == record_array(other.fetch(s)).tobytes()
        assert bank.fetch(s).integrated_lufs > -40.0


# ---------------------------------------------------------------- 10. hard values
def test_nan_and_infinities_under_one_and_under_several_layers(torch_dev, omx):
    ch = 2
    t, b = plan_of(omx, ch)
    frames = t + 9
    xs = [hard_values(mr.noise(130 + s, frames, ch, 0.8), with_nan=True) for s in range(3)]
    xs[1] = np.roll(xs[1], 3, axis=0)      # its hard values meet plain samples of the others, and inf meets -inf at some
    xs[2][4, 0], xs[2][4, 1] = np.float32(-np.inf), np.float32(np.inf)
    sends = [mr.Send(0, 0, 0, 0, frames, 1.0),
             mr.Send(0, 1, 0, 0, frames, 1.0), mr.Send(1, 1, 0, 0, frames, 0.5), mr.Send(2, 1, 0, 0, frames, -1.0),
             mr.Send(0, 2, 0, 0, frames, 0.0), mr.Send(1, 2, 0, 0, frames, 1.0)]      # a gain of 0 over an infinity is a NaN
    bank = new_bank(omx, 3, ch)
    bank.configure_mix(ch, 3)
    _, ys, recs = run_mix(torch_dev, omx, bank, xs, sends, [frames] * 3, ch, tag="hard values")
    assert int(recs[0]["samples_nonfinite"]) == int((~np.isfinite(xs[0])).sum()) >= 3
    for o in range(3):
        got = bank.fetch_mixed(o)
        assert int(got["samples_nonfinite"]) == int((~np.isfinite(ys[o])).sum()) > 0, o
        assert np.isnan(ys[o]).any() and np.isinf(got["out_sample_peak"])
    assert np.isnan(ys[2][0, 0]) and np.isnan(ys[2][0, 1])      # 0 * inf under two layers


# ---------------------------------------------------------------- 11. refusals
def test_refused_calls_change_nothing(torch_dev, omx):
    ch, n, cap, out_cap = 2, 2, 400, 500
    x = np.stack([mr.noise(140 + s, cap, ch) for s in range(n)])
    d_x = torch_dev.from_numpy(x).cuda()
    d_y = torch_dev.full((3, out_cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank = new_bank(omx, n)
    table = [MixSend(0, 0, 0, 0, 300, 0.5), MixSend(1, 0, 0, 290, 200, -1.0), MixSend(0, 1, 100, 5, 40)]
    good = dict(d_in=d_x.data_ptr(), frames_capacity=cap, sends=table, d_out=d_y.data_ptr(), out_capacity=out_cap, out_frames=[490, 45, 7])

    def last_error():
        return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")

    def refused(call, tag):
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        assert last_error().startswith("program loudness mix: "), (tag, last_error())

    refused(lambda: bank.mix(**good), "before configure")
    with pytest.raises(capi.OmxError):
        bank.fetch_mixed(0)
    for channels, buses in ((0, 3), (9, 3), (2, 0), (2, 2 ** 24 + 1)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_mix(channels, buses)
        assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError):
        bank.fetch_mixed(0)                                          # a refused configure configured nothing
    bank.configure_mix(ch, 3)
    ptr = bank.mix(**good, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    y = d_y.cpu().numpy().copy()
    records = device_bytes(ptr, 3 * SIZE)
    assert [int(bank.fetch_mixed(o)["frames"]) for o in range(3)] == [490, 45, 7] and (y[0, :490] != SENTINEL).all()

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert d_x.cpu().numpy().tobytes() == x.tobytes(), tag
        assert d_y.cpu().numpy().tobytes() == y.tobytes(), tag
        assert device_bytes(ptr, 3 * SIZE) == records, tag

    def table_with(k, **kw):
        out = [MixSend(**c.__dict__) for c in table]
        for f, v in kw.items():
            setattr(out[k], f, v)
        return out

    x_bytes = cap * ch * 4
    bad_calls = {"n_out of 0": dict(out_frames=[], sends=[]),
                 "n_out above max_buses": dict(out_frames=[1, 1, 1, 1]),
                 "an unsorted table": dict(sends=[table[1], table[0], table[2]]),
                 "a 65th layer": dict(sends=[MixSend(0, 0, 0, 0, 300, 0.5)] * 65 + [table[2]]),
                 "a send beyond frames_in": dict(frames_in=[299, cap]),
                 "a send beyond the row": dict(sends=table_with(1, frames=401, dst_first=0)),
                 "frames_in beyond the row": dict(frames_in=[cap + 1, cap]),
                 "a flag set": dict(sends=table_with(2, flags=2)),
                 "a NaN gain": dict(sends=table_with(2, gain=float("nan"))),
                 "an infinite gain": dict(sends=table_with(0, gain=float("-inf"))),
                 "src_stream out of range": dict(sends=table_with(2, src_stream=2)),
                 "dst_bus out of range": dict(sends=table_with(2, dst_bus=3)),
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
        refused(lambda: bank.mix(**{**good, **change}), tag)
        unchanged(tag)
    raw = omx.fn("program_loudness_bank_mix", C.c_int,
                 [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p])
    rows, counts, out_ptr = mix_table(table), np.array([490, 45, 7], np.uint32), C.c_void_p()
    args = [bank._h, C.c_void_p(d_x.data_ptr()), cap, None, rows.ctypes.data, 3, C.c_void_p(d_y.data_ptr()), out_cap, 3, None, counts.ctypes.data,
            None, C.addressof(out_ptr)]
    for k, tag in ((4, "null sends"), (10, "null out_frames"), (12, "null d_mixed")):
        assert raw(*[None if i == k else a for i, a in enumerate(args)]) == capi.ERR_INVALID, tag
        assert last_error().startswith("program loudness mix: "), (tag, last_error())
        unchanged(tag)
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_mixed(3)
    assert err.value.status == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_fetch_mixed", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(bank._h, 0, None) == capi.ERR_INVALID
    unchanged("refused fetches")
    # windows at the far end of the range are accepted: nothing but zeros lies there
    assert bank.mix(**{**good, "out_first": [2 ** 40 - 490, 0, 0]}, stream=stream_of(torch_dev)) == ptr
    torch_dev.cuda.synchronize()
    far = d_y.cpu().numpy()
    assert far[0, :490].tobytes() == np.float32(0).tobytes() * (490 * ch) and far[1:].tobytes() == y[1:].tobytes()
    assert int(bank.fetch_mixed(0)["silent_frames"]) == 490 and int(bank.fetch_mixed(0)["out_first"]) == 2 ** 40 - 490


# ---------------------------------------------------------------- 12. the C99 demo
def demo_streams():
    """tests/c_abi/program_mix_demo.c's three stems and their printmaster: f32 [4][12000][2]"""
    stems, frames, ch, state = 3, 12000, 2, 2026
    flat = np.zeros(stems * frames * ch, np.float32)
    for i in range(flat.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        flat[i] = np.float32(((state >> 8) & 0x7FFF) - 16384) / np.float32(65536.0)
    out = np.zeros((stems + 1, frames, ch), np.float32)
    out[:stems] = flat.reshape(stems, frames, ch)
    out[stems] = (out[0] + out[1]).astype(np.float32) + out[2]
    return out


def test_c99_demo_prints_the_floor_and_then_one_step_of_the_lattice(torch_dev, omx, tmp_path):
    """tests/c_abi/program_mix_demo.c: three stems summed into a bus and null-tested against their printmaster, from a plain C host"""
    from test_cpu_program_mix import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], words[1::2]))
    x = demo_streams()
    t, b = plan_of(omx, 2)
    sends = [mr.Send(s, 0, 0, 0, 12000, 1.0) for s in range(3)] + mr.null_table([0, 1, 2], 3, 12000, 1)
    ys, recs = mr.render(list(x), sends, [12000, 12000], 2)
    assert ys[0].tobytes() == x[3].tobytes() and not ys[1].any()
    want = {"tile": t, "batch": b, "extent_0": 12000, "extent_1": 12000, "sum_frames": 12000, "sum_mixed": 12000, "sum_sends": 3, "sum_layers": 3,
            "sum_peak_bits": int(np.float32(recs[0]["out_sample_peak"]).view(np.uint32)), "sum_sample_bits": int(ys[0][777, 1].view(np.uint32)),
            "null_sends": 4, "null_layers": 4, "null_mixed": 12000, "null_nonfinite": 0, "null_peak_bits": 0,
            "off_peak_bits": int(np.float32(2.0 ** -16).view(np.uint32))}
    for key, value in want.items():
        assert int(out[key]) == int(value), (key, out[key], value)
    assert float(out["null_peak_db"]) == float(out["floor_db"]) and abs(float(out["floor_db"]) + 99.9) <= 1e-5
    assert abs(float(out["off_peak_db"]) - 20 * np.log10(2.0 ** -16)) <= 1e-4 and float(out["off_peak_db"]) > float(out["floor_db"])

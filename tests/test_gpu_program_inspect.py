"""Programme bank signal QC on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_inspect / reset_inspect / inspect /
fetch_inspected against the numpy restatement (tests/program_inspect_ref.py, pinned by tests/test_cpu_program_inspect.py).

Bars.  Every device record equals the restatement's on bytes: the record holds integers only.  The restatement sees all the PCM a stream
took since its reset as one array, whatever the calls were.  d_in has the same bytes after every call.
Shapes.  With t = inspect_plan(channels).tile_frames the streams are 0, 1, 63, 64, 65, 1001, t - 1, t, t + 1 and 3 t + 5 frames long:
the smallest at which a ballot word, a tile, their seams and an unaligned row base can go wrong (a row is (3 t + 5) * channels floats,
so at odd channel counts rows start at 4-byte, not 16-byte, offsets).  No test provokes a fault: the refusals use only arguments the
host rejects before any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_inspect_ref as ir
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (INSPECT_ANTIPHASE, INSPECT_RECORD_DTYPE, InspectRule, ProgramLoudnessBank, inspect_plan,
                                             inspect_summarize)
from test_gpu_program_loudness import torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SIZE = 704


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def tile_of(omx, ch):
    return int(inspect_plan(omx, ch)["tile_frames"])


def rules(**kw):
    """the same rule for the bank and for the restatement"""
    return InspectRule(**kw), ir.Rule(**kw)


def run_call(torch, bank, rows, ch, filler=999):
    """rows[s]: f32 [frames][ch] of stream s in this call; the frames of d_in beyond them hold other samples.  Checks that d_in is
    unchanged.  -> the device pointer to the records"""
    n = len(rows)
    counts = [len(r) for r in rows]
    cap = max(max(counts), 1)
    host = ir.noise(filler, n * cap, ch).reshape(n, cap, ch)
    for s, r in enumerate(rows):
        host[s, :len(r)] = r
    d_in = torch.from_numpy(host).cuda()
    ptr = bank.inspect(d_in.data_ptr(), cap, frames=counts, stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    return ptr


def differing_fields(got, want):
    out = [f for f in ir.STREAM_FIELDS + ("channels", "n_pairs") if got[f] != want[f]]
    for c in range(8):
        out += [(c, f) for f in ir.CHANNEL_FIELDS if got["channel"][c][f] != want["channel"][c][f]]
    for p in range(ir.MAX_PAIRS):
        out += [("pair", p, f) for f in ir.PAIR_FIELDS if got["pair"][p][f] != want["pair"][p][f]]
    return [(f, got[f] if isinstance(f, str) else None) for f in out]


def check_stream(bank, s, x, ch, rule, pairs, tag):
    got, want = bank.fetch_inspected(s), ir.record(x, ch, rule, pairs)
    if got.tobytes() != want.tobytes():
        raise AssertionError((tag, s, "record differs from the restatement", differing_fields(got, want), got, want))
    return want


def pairs_of(ch):
    return [] if ch == 1 else ([(0, 1)] if ch == 2 else [(0, 1), (ch - 1, 0), (1, ch - 1), (2, 1)])


# ---------------------------------------------------------------- 1. lengths
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
def test_records_equal_the_restatement_at_every_length(torch_dev, omx, ch):
    t = tile_of(omx, ch)
    lengths = [0, 1, 63, 64, 65, 1001, t - 1, t, t + 1, 3 * t + 5]
    n = len(lengths)
    rule, ref_rule = rules(clip_min_run=2, silence_min_run=2)
    pairs = pairs_of(ch)
    bank = new_bank(omx, n)
    bank.configure_inspect(rule, ch, pairs)
    for s in range(n):      # before the first call: a zero record that names the channels and the pairs
        assert bank.fetch_inspected(s).tobytes() == ir.record(np.zeros((0, ch), np.float32), ch, ref_rule, pairs).tobytes()
    # few channels: noise up to 1.2 with zero frames and repeated samples at 1.0 in it; many channels: hot only by the repeated samples
    xs = [ir.noise(100 * ch + s, f, ch, 1.2 if ch <= 3 else 0.9) for s, f in enumerate(lengths)]
    ptr = run_call(torch_dev, bank, xs, ch)
    hot_runs = quiet_runs = 0
    for s, x in enumerate(xs):
        want = check_stream(bank, s, x, ch, ref_rule, pairs, (ch, lengths))
        hot_runs += int(want["channel"]["clip_runs"].sum())
        quiet_runs += int(want["silent_runs"])
    assert hot_runs > 0 and quiet_runs > 0, "the input does not exercise the run counts"
    assert device_bytes(ptr, n * SIZE) == b"".join(bank.fetch_inspected(s).tobytes() for s in range(n))


# ---------------------------------------------------------------- 2. runs at seams
def test_runs_across_wavefront_tile_and_call_seams(torch_dev, omx):
    """Hot runs (channel 1 of stream 0) and quiet runs (stream 1) of min_run - 1, min_run and min_run + 1 frames, each across a
    64-frame seam, a tile seam and a call seam; stream 2 holds a quiet run over a whole tile and more (t - 5 .. 2 t + 5) and two
    hot runs of equal length, the longest of the stream; stream 3 is quiet from its first frame to its last."""
    ch = 2
    t = tile_of(omx, ch)
    total = 8 * t + 77
    cuts = [0, 3 * t + 100, 3 * t + 800, 3 * t + 1700, total]
    k3 = cuts[3]
    assert total - k3 > 3 * t
    clip_min, sil_min = 4, 6
    rule, ref_rule = rules(clip_min_run=clip_min, silence_min_run=sil_min)
    rng = np.random.default_rng(5)

    def body():      # neither hot nor quiet anywhere
        return ((rng.random((total, ch), dtype=np.float32) * np.float32(0.4) + np.float32(0.1))
                * np.where(rng.random((total, ch)) < 0.5, np.float32(-1), np.float32(1))).astype(np.float32)

    seams = []
    for i in range(3):
        seams.append((i, 64 * (3 + 4 * i)))       # a wavefront seam of the first call
        seams.append((i, (i + 1) * t))            # a tile seam of the first call
        seams.append((i, cuts[i + 1]))            # a call seam
        seams.append((i, k3 + 64 * (3 + 4 * i)))  # a wavefront seam of the last call (tiles and words count from the call's start)
        seams.append((i, k3 + (i + 1) * t))       # a tile seam of the last call
    x_hot, x_quiet, x_long, x_silent = body(), body(), body(), np.zeros((total, ch), np.float32)
    for i, at in seams:
        length = clip_min - 1 + i
        x_hot[at - length // 2:at - length // 2 + length, 1] = np.float32(-1.0) if i == 1 else np.float32(np.inf)
        length = sil_min - 1 + i
        x_quiet[at - length // 2:at - length // 2 + length] = np.float32(-0.0) if i == 1 else np.float32(0.0)
    x_long[t - 5:2 * t + 5] = 0
    x_long[2 * t + 40:2 * t + 70, 0] = 1.0      # 30 hot frames across a 64-frame seam
    x_long[5 * t - 10:5 * t + 20, 0] = 1.0      # and 30 more later: the earlier start wins
    xs = [x_hot, x_quiet, x_long, x_silent]
    bank = new_bank(omx, len(xs))
    bank.configure_inspect(rule, ch, [(0, 1)])
    for a, b in zip(cuts[:-1], cuts[1:]):
        run_call(torch_dev, bank, [x[a:b] for x in xs], ch)
        for s, x in enumerate(xs):
            check_stream(bank, s, x[:b], ch, ref_rule, [(0, 1)], ("after the call that ends at", b))
    hot, quiet, long_, silent = (bank.fetch_inspected(s) for s in range(4))
    # what the construction says, beside the restatement: per kind of seam one run below the minimum and two that reach it
    assert int(hot["channel"][1]["clip_runs"]) == 10 and int(hot["channel"][1]["clipped_samples"]) == 5 * (3 + 4 + 5)
    assert int(hot["channel"][1]["longest_clip_run"]) == 5 and int(hot["channel"][1]["longest_clip_start"]) == 64 * 11 - 2
    assert int(quiet["silent_runs"]) == 10 and int(quiet["silent_frames"]) == 5 * (5 + 6 + 7) and int(quiet["longest_silent_run"]) == 7
    assert int(long_["longest_silent_run"]) == t + 10 and int(long_["longest_silent_start"]) == t - 5 and int(long_["silent_runs"]) == 1
    assert int(long_["channel"][0]["longest_clip_run"]) == 30 and int(long_["channel"][0]["longest_clip_start"]) == 2 * t + 40
    assert int(long_["channel"][0]["clip_runs"]) == 2
    for f in ("silent_frames", "longest_silent_run", "leading_silence", "trailing_silence"):
        assert int(silent[f]) == total, f
    assert int(silent["silent_runs"]) == 1 and int(silent["longest_silent_start"]) == 0


# ---------------------------------------------------------------- 3. cuts
def test_record_does_not_depend_on_the_cuts(torch_dev, omx):
    ch = 3
    t = tile_of(omx, ch)
    total = 3 * t + 5
    rule, ref_rule = rules(clip_min_run=2, silence_min_run=3)
    pairs = pairs_of(ch)
    x = ir.noise(41, total, ch)
    x[t - 40:t + 90] = 0              # silence across a tile seam
    x[2 * t - 3:2 * t + 300, 2] = -1.5      # a long flat top across another
    x[7, 1], x[total - 1, 0] = np.nan, np.inf
    other = ir.noise(42, 777, ch)
    bank = new_bank(omx, 2)
    bank.configure_inspect(rule, ch, pairs)
    run_call(torch_dev, bank, [x, other], ch)
    whole = check_stream(bank, 0, x, ch, ref_rule, pairs, "whole").tobytes()
    bystander = check_stream(bank, 1, other, ch, ref_rule, pairs, "whole").tobytes()
    rng = np.random.default_rng(43)
    plans = [[1, 63, t, t + 1], sorted(set(int(v) for v in rng.integers(1, total, 9))), sorted(set(int(v) for v in rng.integers(1, total, 4)))]
    for cuts in plans:
        bank.reset_inspect([1, 0])      # stream 0 alone
        assert bank.fetch_inspected(1).tobytes() == bystander, "a reset of stream 0 changed stream 1"
        assert bank.fetch_inspected(0).tobytes() == ir.record(x[:0], ch, ref_rule, pairs).tobytes()
        edges = [0] + cuts + [total]
        for a, b in zip(edges[:-1], edges[1:]):
            run_call(torch_dev, bank, [x[a:b], other[:0]], ch)
        assert bank.fetch_inspected(0).tobytes() == whole, ("the record depends on the cuts", cuts)
        assert bank.fetch_inspected(1).tobytes() == bystander


# ---------------------------------------------------------------- 4. hard values
def test_hard_values(torch_dev, omx):
    ch, pairs = 2, [(0, 1)]
    clip = np.float32(0.99996948)
    below = np.nextafter(clip, np.float32(0))
    tiny, level = np.float32(1e-45), np.float32(1e-4)
    x = ir.noise(51, 900, ch, 0.5)
    x[3], x[4], x[5], x[6] = (np.nan, 0.25), (np.inf, -np.inf), (-0.0, 0.0), (tiny, -tiny)
    x[10:14, 0], x[10:14, 1] = clip, below      # at clip_level exactly: hot; one ulp below: not
    x[20:24, 0], x[20:24, 1] = -clip, -below
    x[30], x[31], x[32] = (level, -level), (np.nextafter(level, np.float32(1)), 0.0), (0.0, 0.0)
    x[40], x[41] = (5.0, -5.0), (1.5, 1.5)       # the DC clamp at 4, the product clamp at 1
    x[42], x[43] = (np.inf, 0.0), (np.nan, np.nan)      # inf * 0 is NaN: that product gives 0; a frame of NaN
    x[100:110] = tiny                                   # denormals are not digital silence
    x[200:210] = 0.0
    silent = []
    for kw in (dict(silence_level=0.0), dict(silence_level=float(level))):
        rule, ref_rule = rules(clip_min_run=4, silence_min_run=1, **kw)
        bank = new_bank(omx, 1)
        bank.configure_inspect(rule, ch, pairs)
        run_call(torch_dev, bank, [x], ch)
        want = check_stream(bank, 0, x, ch, ref_rule, pairs, kw)
        assert [int(want["channel"][c]["nan_samples"]) for c in range(2)] == [2, 1]
        assert [int(want["channel"][c]["clip_runs"]) for c in range(2)] == [2, 0]
        silent.append(int(want["silent_frames"]))
    # level 0: the frames of zeros of either sign, not the denormal ones; with the level also frame 30 (exactly the level), frame 6
    # and frames 100 .. 109 (denormals), not frame 31 (one ulp above it)
    assert silent[0] == int((x == 0).all(axis=1).sum()) and silent[0] >= 12 and silent[1] - silent[0] == 12


def test_a_silent_channel_has_no_correlation_and_an_inverted_copy_is_antiphase(torch_dev, omx):
    ch, pairs = 3, [(0, 1), (0, 2), (2, 0)]
    t = tile_of(omx, ch)
    x = ir.noise(61, t + 70, ch, 0.7)
    x[:, 1] = 0.0
    x[:, 2] = -x[:, 0]
    rule, ref_rule = rules()
    bank = new_bank(omx, 1)
    bank.configure_inspect(rule, ch, pairs)
    run_call(torch_dev, bank, [x], ch)
    check_stream(bank, 0, x, ch, ref_rule, pairs, "pairs")
    got = inspect_summarize(omx, rule, bank.fetch_inspected(0))
    want = ir.summarize(ref_rule, bank.fetch_inspected(0))
    assert list(got["correlation_valid"]) == [0, 1, 1, 0] and float(got["correlation"][0]) == 0.0
    assert float(got["correlation"][1]) == -1.0 and float(got["correlation"][2]) == -1.0
    assert int(got["verdict"]) == want["verdict"] and int(got["verdict"]) & INSPECT_ANTIPHASE


# ---------------------------------------------------------------- 5. nothing else moves
def test_inspect_leaves_the_records_of_the_earlier_headers_alone(torch_dev, omx):
    ch, n, frames = 2, 3, 22051
    pos = capi.positions_fallback(ch)
    bank = new_bank(omx, n)
    tt = np.arange(frames)
    tone = (0.2 * np.sin(2 * np.pi * 997.0 * tt / 48000.0) * ((tt // 9000) % 2 + 1) / 2.0).astype(np.float32)
    x = np.stack([tone[:, None] * np.float32(0.9 - 0.1 * s) + np.float32(0.01) * ir.noise(70 + s, frames, ch) for s in range(n)]).astype(np.float32)
    d_some = torch_dev.from_numpy(x).cuda()
    bank.set_peaks(True)
    bank.process(d_some.data_ptr(), frames, ch, 48000.0, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()

    def state():
        return ([record_array(bank.fetch(s)).tobytes() for s in range(n)], [bank.fetch_peaks(s).tobytes() for s in range(n)],
                [bank.fetch_segments(s).tobytes() for s in range(n)])

    before = state()
    rule, ref_rule = rules()
    bank.configure_inspect(rule, ch, [(0, 1)])
    run_call(torch_dev, bank, [x[s] for s in range(n)], ch)
    for s in range(n):
        check_stream(bank, s, x[s], ch, ref_rule, [(0, 1)], "beside process")
    assert state() == before, "a call of program_inspect.h changed a record of an earlier header"
    assert d_some.cpu().numpy().tobytes() == x.tobytes()


def test_refused_calls_change_nothing(torch_dev, omx):
    ch, n, cap = 2, 3, 400
    pairs = [(0, 1)]
    x = np.stack([ir.noise(90 + s, cap, ch) for s in range(n)])
    d_x = torch_dev.from_numpy(x).cuda()
    d_in = d_x.data_ptr()
    bank = new_bank(omx, n)
    good = dict(d_in=d_in, frames_capacity=cap, frames=[300, 0, 150])
    for call in (lambda: bank.inspect(**good), lambda: bank.fetch_inspected(0), lambda: bank.reset_inspect()):      # before configure
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID
    rule, ref_rule = rules(clip_min_run=2, silence_min_run=2)

    def bad_configures(tag):
        bad_rules = [dict(clip_level=0.0), dict(clip_level=-1.0), dict(clip_level=np.nan), dict(clip_level=np.inf), dict(clip_min_run=0),
                     dict(clip_min_run=65536), dict(silence_level=-1e-9), dict(silence_level=np.nan), dict(silence_level=np.inf),
                     dict(silence_min_run=0), dict(silence_min_run=2 ** 24 + 1), dict(dc_limit=-1.0), dict(dc_limit=np.nan),
                     dict(correlation_min=-1.5), dict(correlation_min=1.5), dict(correlation_min=np.nan), dict(flags=1)]
        attempts = [(InspectRule(**kw), ch, pairs) for kw in bad_rules]
        attempts += [(rule, 0, []), (rule, 9, []), (rule, ch, [(0, 1)] * 5), (rule, ch, [(0, 2)]), (rule, ch, [(2, 0)]), (rule, ch, [(1, 1)])]
        for r, c, p in attempts:
            with pytest.raises(capi.OmxError) as err:
                bank.configure_inspect(r, c, p)
            assert err.value.status == capi.ERR_INVALID, (tag, r, c, p)
        configure = omx.fn("program_loudness_bank_inspect_configure", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])
        assert configure(bank._h, None, ch, None, 0) == capi.ERR_INVALID, tag          # a null rule
        c_rule = rule.to_c()
        assert configure(bank._h, C.byref(c_rule), ch, None, 1) == capi.ERR_INVALID, tag      # null pairs with n_pairs 1

    bad_configures("new bank")
    with pytest.raises(capi.OmxError):
        bank.fetch_inspected(0)                                         # a refused configure configured nothing
    bank.configure_inspect(rule, ch, pairs)
    ptr = bank.inspect(**good, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    records = device_bytes(ptr, n * SIZE)
    assert [int(bank.fetch_inspected(s)["frames"]) for s in range(n)] == [300, 0, 150]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert d_x.cpu().numpy().tobytes() == x.tobytes(), tag
        assert device_bytes(ptr, n * SIZE) == records, tag

    bad_configures("configured bank")
    unchanged("refused configures")
    with pytest.raises(capi.OmxError) as err:      # a good configure is refused too while a stream holds frames
        bank.configure_inspect(rule, ch, pairs)
    assert err.value.status == capi.ERR_INVALID
    unchanged("configure while streams hold frames")
    bad_calls = {"frames[s] > frames_capacity": dict(frames=[cap + 1, 0, 0]),
                 "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                 "more than 2^32 - 1 frames since the reset": dict(frames_capacity=2 ** 32 - 1, frames=[2 ** 32 - 300, 0, 0]),
                 "null d_in": dict(d_in=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.inspect(**{**good, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    raw_fn = omx.fn("program_loudness_bank_inspect", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p])
    counts = np.array([1, 1, 1], np.uint32)
    assert raw_fn(bank._h, C.c_void_p(d_in), cap, counts.ctypes.data, None, None) == capi.ERR_INVALID      # null d_inspected
    unchanged("null d_inspected")
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_inspected(n)
    assert err.value.status == capi.ERR_INVALID
    fetch = omx.fn("program_loudness_bank_fetch_inspected", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])
    assert fetch(bank._h, 0, None) == capi.ERR_INVALID
    unchanged("refused fetches")
    # a null buffer is accepted where no stream brings a frame, and nothing moves
    assert bank.inspect(d_in=0, frames_capacity=cap, frames=[0, 0, 0]) == ptr
    unchanged("a call without frames")
    # the host's mirror did not move either: the streams go on from 300, 0 and 150 frames
    run_call(torch_dev, bank, [x[0, 300:377], x[1], x[2, 150:150]], ch)
    for s, f in enumerate((377, cap, 150)):
        check_stream(bank, s, x[s, :f], ch, ref_rule, pairs, "after the refusals")
    # after a reset of every stream a new configure is allowed
    bank.reset_inspect()
    bank.configure_inspect(rule, 1, [])
    assert bank.fetch_inspected(2).tobytes() == ir.record(np.zeros((0, 1), np.float32), 1, ref_rule, []).tobytes()


# ---------------------------------------------------------------- 6. many streams
def test_more_streams_than_one_launch_holds(torch_dev, omx):
    n, ch = 70000, 1
    rule, ref_rule = rules(clip_min_run=1, silence_min_run=1)
    rng = np.random.default_rng(7)
    x = rng.choice(np.array([0.0, 1.0, -0.5, 0.25, np.nan], np.float32), size=(n, 1, ch))
    bank = new_bank(omx, n, ch)
    bank.configure_inspect(rule, ch, [])
    d_in = torch_dev.from_numpy(x).cuda()
    ptr = bank.inspect(d_in.data_ptr(), 1, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    got = np.frombuffer(device_bytes(ptr, n * SIZE), INSPECT_RECORD_DTYPE)
    assert d_in.cpu().numpy().tobytes() == x.tobytes()
    # one frame of one channel: the record follows from the sample's kind
    kinds = {float(v): ir.record(np.array([[v]], np.float32), ch, ref_rule, []) for v in (0.0, 1.0, -0.5, 0.25)}
    nan_record = ir.record(np.array([[np.nan]], np.float32), ch, ref_rule, [])
    want = np.zeros(n, INSPECT_RECORD_DTYPE)
    flat = x.reshape(n)
    for v, rec in kinds.items():
        want[flat == np.float32(v)] = rec
    want[np.isnan(flat)] = nan_record
    assert got.tobytes() == want.tobytes(), np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])[:8]
    for s in (0, 65534, 65535, 65536, n - 1):
        assert bank.fetch_inspected(s).tobytes() == want[s].tobytes()


# ---------------------------------------------------------------- 7. the C99 demo
def demo_programme():
    """tests/c_abi/program_inspect_demo.c's programme: f32 [96000][2]"""
    frames, state = 96000, 2024
    left = np.zeros(frames, np.float32)
    for f in range(frames):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        left[f] = np.float32(((state >> 8) & 0xFFFFFF) - 8388608) / np.float32(33554432.0)
    left[10000:10400] = 1.0
    left[30000:30400] = -1.0
    left[50000:51000] = 0.0
    return np.stack([left, -left], 1)


def test_c99_demo_prints_the_restatements_verdict(torch_dev, omx, tmp_path):
    """tests/c_abi/program_inspect_demo.c: a stereo programme with a clipped passage, a dropout and an inverted right channel, inspected
    in two calls from a plain C host"""
    from test_cpu_program_inspect import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], words[1::2]))
    x = demo_programme()
    rec = ir.record(x, 2, ir.Rule(), [(0, 1)])
    summary = ir.summarize(ir.Rule(), rec)
    left, right, pair = rec["channel"][0], rec["channel"][1], rec["pair"][0]
    want = {"tile": tile_of(omx, 2), "frames": 96000, "silent_frames": rec["silent_frames"], "silent_runs": rec["silent_runs"],
            "longest_silent_run": rec["longest_silent_run"], "longest_silent_start": rec["longest_silent_start"],
            "leading": rec["leading_silence"], "trailing": rec["trailing_silence"], "clipped_left": left["clipped_samples"],
            "clip_runs_left": left["clip_runs"], "longest_clip_run_left": left["longest_clip_run"],
            "longest_clip_start_left": left["longest_clip_start"], "clip_runs_right": right["clip_runs"], "dc_sum_left": left["dc_sum"],
            "sum_ab": pair["sum_ab"], "sum_aa": pair["sum_aa"], "interior_silent_runs": summary["interior_silent_runs"],
            "correlation_valid": 1, "verdict": summary["verdict"]}
    for key, value in want.items():
        assert int(out[key]) == int(value), (key, out[key], value)
    assert summary["verdict"] == ir.CLIPPED | ir.DROPOUT | ir.ANTIPHASE
    assert [int(out[k]) for k in ("nan", "clipped", "dropout", "all_silent", "dc", "antiphase")] == [0, 1, 1, 0, 0, 1]
    assert int(out["longest_clip_run_left"]) == 400 and int(out["longest_clip_start_left"]) == 10000 and int(out["clip_runs_right"]) == 2
    assert int(out["longest_silent_run"]) >= 1000 and int(out["interior_silent_runs"]) == 1
    assert float(out["correlation"]) == -1.0
    assert abs(float(out["dc_offset_left"]) - summary["dc_offset"][0]) <= 1e-6 * abs(summary["dc_offset"][0])

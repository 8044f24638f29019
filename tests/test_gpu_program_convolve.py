"""Programme bank convolve stage on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_convolve / convolve /
reset_convolve / fetch_convolved against the numpy restatement (tests/program_convolve_ref.py, pinned by
tests/test_cpu_program_convolve.py).

Bars.  Every float of the output equals the restatement's on bytes, with a NaN where it has a NaN (the bits of a NaN the arithmetic
produces are not defined; a bypassed channel is compared on bytes, NaN payloads included); every record field equal except
out_sample_peak_db, within 1e-4 dB (the family's bar).  Not written: d_out is filled with a sentinel float beforehand and every float
at or beyond frames_written[s] * channels keeps it; d_in keeps its bytes.  Cut invariance: every programme is rendered whole and in
cuts (one cut brings fewer than max_taps - 1 frames, one brings none; the flush rides on the last frames or comes in a call of its
own), and every schedule gives the bytes of the restatement's one-call output.
Shapes come from convolve_plan: t = tile_frames, R = frames_per_thread, KB = tap_block.  No test provokes a fault: the refusals use
only arguments the host rejects before any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_convolve_ref as cr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (CONVOLVE_BYPASS, CONVOLVE_RECORD_DTYPE, ConvolveSpec, ProgramLoudnessBank, convolve_design,
                                             convolve_frames, convolve_plan)
from test_cpu_program_convolve import build_demo
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
CHANNELS = (1, 2, 3, 6, 8)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def plan_of(omx, ch):
    info = convolve_plan(omx, ch, 4096)
    return int(info["tile_frames"]), int(info["frames_per_thread"]), int(info["tap_block"])


class Setup:
    """a configured bank with the restatement's view of it: per stream the taps of every channel (None: bypass)"""

    def __init__(self, omx, n, ch, table, delay, fir_of_channel=None):
        self.omx, self.n, self.ch, self.delay = omx, n, ch, delay
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
        self.bank.configure_convolve(table, ch, fir_of_channel, delay)
        foc = np.zeros((n, ch), np.uint32) if fir_of_channel is None else np.asarray(fir_of_channel, np.uint32).reshape(n, ch)
        self.firs = [[None if f == CONVOLVE_BYPASS else np.asarray(table[f], np.float32) for f in row] for row in foc]
        self.max_taps = max([len(t) for row in self.firs for t in row if t is not None] + [1])
        self.mirror = [(0, 0)] * n      # (frames taken, frames emitted)

    def reference(self, s):
        return cr.Stream(self.firs[s], self.delay, self.max_taps, FLOOR)

    def call(self, torch, rows, flush=None, filler=999):
        """rows[s]: f32 [frames][ch] of stream s in this call; frames of d_in beyond them hold other samples.  d_out holds the
        sentinel beforehand.  Checks that d_in keeps its bytes, that every stream wrote what the streaming formula says and nothing at
        or beyond it.  -> (per stream the frames written, the device pointer to the records)"""
        n, ch = self.n, self.ch
        counts = [len(r) for r in rows]
        cap = max(max(counts), 1)
        host = cr.noise(filler, n * cap, ch).reshape(n, cap, ch)
        for s, r in enumerate(rows):
            host[s, :len(r)] = r
        emits = [convolve_frames(self.omx, self.delay, self.mirror[s][0], self.mirror[s][1], counts[s], bool(flush and flush[s]))
                 for s in range(n)]
        out_cap = max(max(emits) + 1, 1)
        d_in = torch.from_numpy(host).cuda()
        d_out = torch.full((n, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
        ptr = self.bank.convolve(d_in.data_ptr(), cap, d_out.data_ptr(), out_cap, frames=counts, flush_mask=flush, stream=stream_of(torch))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
        out = []
        for s in range(n):
            w = int(self.bank.fetch_convolved(s)["frames_written"])
            assert w == emits[s] == cr.emitted(self.delay, self.mirror[s][0] + counts[s], self.mirror[s][1], bool(flush and flush[s])) - self.mirror[s][1]
            assert (got[s, w:] == SENTINEL).all(), (s, w, "floats at or beyond frames_written[s] * channels were written")
            out.append(got[s, :w].copy())
            self.mirror[s] = (self.mirror[s][0] + counts[s], self.mirror[s][1] + w)
        return out, ptr

    def reset(self, mask=None):
        self.bank.reset_convolve(mask)
        self.mirror = [(0, 0) if mask is None or mask[s] else m for s, m in enumerate(self.mirror)]

    def render(self, torch, xs, cuts, own_flush):
        """every stream's programme in the calls of `cuts` (fractions of each stream's length; 0 brings nothing, "few" brings fewer
        than max_taps - 1 frames where the stream has them); the flush in the last call, or in a call of its own"""
        n = self.n
        at, parts, last_written = [0] * n, [[] for _ in range(n)], [0] * n
        few = max(1, min(self.max_taps - 2, 5))
        for i, cut in enumerate(cuts):
            last = i == len(cuts) - 1
            rows = []
            for s, x in enumerate(xs):
                f = len(x) - at[s] if last else (min(few, len(x) - at[s]) if cut == "few" else min(int(cut * len(x)), len(x) - at[s]))
                rows.append(x[at[s]:at[s] + f])
                at[s] += f
            out, ptr = self.call(torch, rows, flush=[1] * n if last and not own_flush else None, filler=900 + i)
            for s in range(n):
                parts[s].append(out[s])
                last_written[s] = len(out[s])
        if own_flush:
            out, ptr = self.call(torch, [x[:0] for x in xs], flush=[1] * n)
            for s in range(n):
                parts[s].append(out[s])
                last_written[s] = len(out[s])
        return [np.concatenate(p) for p in parts], last_written, ptr


SCHEDULES = ((((1.0,), False), "whole"), ((("few", 0, 0.4, 1.0), True), "few / none / 0.4 / rest, flush apart"),
             (((0.5, 1.0), False), "halves"), (((0.3, 0.3, 0, 1.0), True), "thirds, flush apart"))


def check_programmes(torch, omx, ch, table, delay, xs, fir_of_channel=None, schedules=SCHEDULES, tag=None):
    """every schedule against the restatement's one-call output, bytes and records"""
    n = len(xs)
    wants = None
    for (cuts, own_flush), name in schedules:
        setup = Setup(omx, n, ch, table, delay, fir_of_channel)
        if wants is None:      # the restatement, once
            wants = []
            for s, x in enumerate(xs):
                ref = setup.reference(s)
                wants.append((ref.feed(x, flush=True), ref.record()))
        got, last_written, ptr = setup.render(torch, xs, cuts, own_flush)
        for s in range(n):
            want, rec = wants[s]
            cr.same_floats(got[s], want, (tag, name, "stream", s))
            for c, t in enumerate(setup.firs[s]):
                if t is None:
                    assert got[s][:, c].tobytes() == xs[s][:, c].tobytes(), (tag, name, s, c, "a bypassed channel is a copy on bits")
            cr.check_record(setup.bank.fetch_convolved(s), dict(rec, frames_written=last_written[s]), (tag, name, s), BAR)
        assert device_bytes(ptr, n * 64) == b"".join(setup.bank.fetch_convolved(s).tobytes() for s in range(n))
    return wants


def tap_counts(omx, ch):
    t, R, KB = plan_of(omx, ch)
    return [1, 2, 3, R, R + 1, KB - 1, KB, KB + 1, 2 * KB + 1]


def frame_counts(omx, ch):
    t, R, KB = plan_of(omx, ch)
    return [0, 1, 3, R - 1, R + 1, t - 1, t, t + 1, 3 * t + 5]


# ---------------------------------------------------------------- 1. bits, records, nothing else written
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("which", range(9))
def test_tap_counts_and_frame_counts(torch_dev, omx, which, ch):
    """T = 1, 2, 3, R, R + 1, KB - 1, KB, KB + 1, 2 KB + 1 (`which` picks one) with D = (T - 1) / 2, nine streams of 0, 1, 3, R - 1,
    R + 1, t - 1, t, t + 1 and 3 t + 5 frames.  Stream 2 runs a shorter FIR on its last channel and stream 5 bypasses its first; with
    more than one channel stream 7 runs the short FIR on channel 0 and bypasses the last."""
    T = tap_counts(omx, ch)[which]
    lengths = frame_counts(omx, ch)
    n = len(lengths)
    table = [cr.random_taps(10 * T + ch, T), cr.random_taps(10 * T + ch + 1, max(1, T // 3))]
    foc = np.zeros((n, ch), np.uint32)
    foc[2, ch - 1] = 1
    foc[5, 0] = CONVOLVE_BYPASS
    if ch > 1:
        foc[7, 0], foc[7, ch - 1] = 1, CONVOLVE_BYPASS
    xs = [cr.noise(1000 * which + 10 * ch + s, f, ch) for s, f in enumerate(lengths)]
    check_programmes(torch_dev, omx, ch, table, (T - 1) // 2, xs, foc, tag=(T, ch))


# ---------------------------------------------------------------- 2. delays
@pytest.mark.parametrize("ch", (2, 3))
@pytest.mark.parametrize("which", (4, 7))
def test_delays_with_and_without_a_flush(torch_dev, omx, which, ch):
    """D in {0, 1, (T - 1) / 2, T - 1} at T = R + 1 and KB + 1; the unflushed runs end D frames short and stay RUNNING"""
    t, R, KB = plan_of(omx, ch)
    T = tap_counts(omx, ch)[which]
    table = [cr.random_taps(T + 7, T)]
    foc = np.zeros((3, ch), np.uint32)
    foc[1, ch - 1] = CONVOLVE_BYPASS
    xs = [cr.noise(50 + s + T, f, ch) for s, f in enumerate((t + R + 3, 2 * KB + 9, T - 1))]
    for delay in sorted({0, 1, (T - 1) // 2, T - 1}):
        check_programmes(torch_dev, omx, ch, table, delay, xs, foc, schedules=SCHEDULES[:2], tag=(T, ch, delay))
        # without a flush: the same frames up to N - D, in one call and in cuts
        for cuts in ((1.0,), ("few", 0, 0.6, 1.0)):
            setup = Setup(omx, 3, ch, table, delay, foc)
            at, parts = [0] * 3, [[] for _ in range(3)]
            for i, cut in enumerate(cuts):
                rows = []
                for s, x in enumerate(xs):
                    f = len(x) - at[s] if i == len(cuts) - 1 else min(5 if cut == "few" else int(cut * len(x)), len(x) - at[s])
                    rows.append(x[at[s]:at[s] + f])
                    at[s] += f
                out, _ = setup.call(torch_dev, rows)
                for s in range(3):
                    parts[s].append(out[s])
            for s, x in enumerate(xs):
                ref = setup.reference(s)
                want = ref.feed(x)
                got = np.concatenate(parts[s])
                assert len(want) == max(len(x) - delay, 0)
                cr.same_floats(got, want, (T, ch, delay, cuts, s))
                rec = setup.bank.fetch_convolved(s)
                cr.check_record(rec, dict(ref.record(), frames_written=len(parts[s][-1])), (T, ch, delay, cuts, s), BAR)
                assert int(rec["state"]) == cr.RUNNING and int(rec["frames_out"]) == len(want)


# ---------------------------------------------------------------- 3. many streams
@pytest.mark.parametrize("n", (65, 130))
def test_many_ragged_streams(torch_dev, omx, n):
    """past one wavefront of records: ragged lengths around a tile, every fifth stream empty, a bypass on every third"""
    ch = 2
    t, R, KB = plan_of(omx, ch)
    table = [cr.random_taps(3, 15), cr.random_taps(4, R + 1)]
    rng = np.random.default_rng(n)
    lengths = [0 if s % 5 == 4 else int(rng.integers(1, t + 40)) for s in range(n)]
    lengths[0], lengths[n - 1] = t + 1, t - 1
    foc = np.array([[s % 2, CONVOLVE_BYPASS if s % 3 == 0 else 0] for s in range(n)], np.uint32)
    xs = [cr.noise(7000 + s, f, ch, amplitude=0.5 + (s % 4)) for s, f in enumerate(lengths)]
    wants = check_programmes(torch_dev, omx, ch, table, 7, xs, foc, tag=("streams", n))
    assert sum(int(rec["samples_over"]) for _, rec in wants) > 0      # (the bypassed channels of the louder streams alone)


# ---------------------------------------------------------------- 4. reset
def test_a_reset_of_some_streams_mid_way(torch_dev, omx):
    ch = 3
    t, R, KB = plan_of(omx, ch)
    T = 33
    table = [cr.random_taps(33, T)]
    xs = [cr.noise(300 + s, f, ch) for s, f in enumerate((200, t + 9, 50, 120))]
    setup = Setup(omx, 4, ch, table, 16)
    first, _ = setup.call(torch_dev, [x[:len(x) // 2] for x in xs])
    setup.reset([0, 1, 1, 0])
    for s in (1, 2):
        rec = setup.bank.fetch_convolved(s)
        want = np.array([(0, 0, 0, 0, 0, 0.0, FLOOR, cr.IDLE, 16, T, 0)], CONVOLVE_RECORD_DTYPE)
        assert rec.tobytes() == want.tobytes(), rec
    # streams 0 and 3 go on where they were; streams 1 and 2 start over with the whole programme
    second, _ = setup.call(torch_dev, [xs[0][100:], xs[1], xs[2], xs[3][60:]], flush=[1] * 4)
    for s in range(4):
        ref = setup.reference(s)
        want = ref.feed(xs[s], flush=True)
        got = np.concatenate([first[s], second[s]]) if s in (0, 3) else second[s]
        cr.same_floats(got, want, ("reset", s))
        cr.check_record(setup.bank.fetch_convolved(s), dict(ref.record(), frames_written=len(second[s])), ("reset", s), BAR)
    # a flushed stream takes frames again after its reset
    setup.reset([1, 0, 0, 0])
    again, _ = setup.call(torch_dev, [xs[0], xs[1][:0], xs[2][:0], xs[3][:0]], flush=[1, 0, 0, 0])
    cr.same_floats(again[0], setup.reference(0).feed(xs[0], flush=True), ("reset", "again"))


# ---------------------------------------------------------------- 5. hard values
@pytest.mark.parametrize("ch", (1, 2, 6))
def test_hard_values_at_the_start_at_tile_seams_and_under_a_zero_tap(torch_dev, omx, ch):
    """+-inf, -0.0, denormals and a NaN with a payload at frame 0, either side of the first tile's end and of a register window's end,
    on a FIR with zero taps (an infinity under a zero tap is a NaN); the last channel of stream 1 is bypassed and keeps the payload"""
    t, R, KB = plan_of(omx, ch)
    T = 2 * R + 3
    h = cr.random_taps(77, T, zeros=False)
    h[[0, 3, R, T - 1]] = 0.0
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    hard = [np.inf, -np.inf, -0.0, 1e-45, -1e-40, nan, 3.0e38, -0.0]
    n_frames = t + 3 * R + 5
    xs = []
    for s in range(3):
        x = cr.noise(400 + s + ch, n_frames, ch)
        spots = [0, 1, R - 1, R, t - 2, t - 1, t, t + 1, t + R, n_frames - 1][s::3] if s else [0, t - 1, t, n_frames - 1]
        for i, at in enumerate(spots):
            x[at, (i + s) % ch] = hard[(i + 2 * s) % len(hard)]
        xs.append(x)
    xs[2][:, :] = np.where(np.arange(n_frames)[:, None] % 7 == 0, np.float32(-0.0), xs[2])
    foc = np.zeros((3, ch), np.uint32)
    foc[1, ch - 1] = CONVOLVE_BYPASS
    wants = check_programmes(torch_dev, omx, ch, [h], (T - 1) // 2, xs, foc, schedules=SCHEDULES[:2], tag=("hard", ch))
    assert sum(int(rec["samples_nonfinite"]) for _, rec in wants) > 0
    assert any(np.isnan(w).sum() > 1 for w, _ in wants)      # one infinity spreads under the zero taps


def test_a_unit_impulse_at_the_delay_against_a_bypass(torch_dev, omx):
    """Channel 0 runs the FIR (0, .., 0, 1) with the 1 at k = D, channel 1 is bypassed: the outputs are equal except for the sign of
    zero (a term 0 * x of the FIR is +0.0 unless x is negative, and -0.0 plus +0.0 is +0.0) and except where an infinity or NaN of
    the input lies under a zero tap, which the test's input does not hold.  A FIR of ONE tap 1.0 at D = 0 equals the bypass on bits,
    -0.0 included."""
    t, R, KB = plan_of(omx, 2)
    for D in (1, R, KB + 2):
        h = np.zeros(D + 1, np.float32)
        h[D] = 1.0
        x = cr.noise(D, t + 50, 1)
        x[5::11] = -0.0
        x[7] = 1e-45
        both = np.repeat(x, 2, axis=1)
        setup = Setup(omx, 1, 2, [h], D, [[0, CONVOLVE_BYPASS]])
        (got,), _ = setup.call(torch_dev, [both], flush=[1])
        assert got[:, 1].tobytes() == x[:, 0].tobytes()
        cr.same_floats(got[:, 0], setup.reference(0).feed(both, flush=True)[:, 0], ("impulse", D))
        assert (got[:, 0] == got[:, 1]).all()      # equal as numbers
        differ = got[:, 0].view(np.uint32) != got[:, 1].view(np.uint32)
        # on bits only -0.0 samples differ: those whose window holds a sample that is not negative under a zero tap (0 * x = +0.0)
        assert differ.sum() > 0 and (x[differ, 0].view(np.uint32) == 0x80000000).all()
        assert (got[differ, 0].view(np.uint32) == 0).all()
    x = cr.noise(9, 300, 1)
    x[3::5] = -0.0
    setup = Setup(omx, 1, 2, [np.ones(1, np.float32)], 0, [[0, CONVOLVE_BYPASS]])
    (got,), _ = setup.call(torch_dev, [np.repeat(x, 2, axis=1)])
    assert got[:, 0].tobytes() == got[:, 1].tobytes() == x[:, 0].tobytes()


# ---------------------------------------------------------------- 6. the longest FIR
@pytest.mark.parametrize("ch", (1, 8))
def test_4096_taps_on_a_few_hundred_frames(torch_dev, omx, ch):
    """sixteen tap blocks with the accumulators kept in registers; the cuts bring fewer than 4095 frames each"""
    table = [cr.random_taps(4096, 4096), convolve_design(omx, ConvolveSpec(0, 4095, 0.0, 6000.0, 9.0), 48000.0)]
    foc = np.zeros((2, ch), np.uint32)
    foc[1, :] = 1
    foc[1, ch - 1] = 0 if ch > 1 else 1
    xs = [cr.noise(4096 + s + ch, f, ch) for s, f in enumerate((300, 517))]
    check_programmes(torch_dev, omx, ch, table, 2047, xs, foc, schedules=SCHEDULES[:2], tag=("4096", ch))


# ---------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing(torch_dev, omx):
    torch = torch_dev
    ch, n = 2, 2
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
    d_in = torch.zeros((n, 64, ch), dtype=torch.float32).cuda()
    d_out = torch.full((n, 64, ch), float(SENTINEL), dtype=torch.float32).cuda()

    def refused(f, who="convolve"):
        with pytest.raises(capi.OmxError) as e:
            f()
        assert e.value.status == capi.ERR_INVALID
        assert omx.fn("last_error", C.c_char_p, [])().decode().startswith(f"program loudness {who}: "), omx.fn("last_error", C.c_char_p, [])()

    # before configure
    refused(lambda: bank.convolve(d_in.data_ptr(), 64, d_out.data_ptr(), 64))
    refused(lambda: bank.reset_convolve(), "convolve_reset")
    refused(lambda: bank.fetch_convolved(0), "fetch_convolved")
    h = cr.random_taps(1, 9)
    for bad in (lambda: bank.configure_convolve([h], 0), lambda: bank.configure_convolve([h], 9), lambda: bank.configure_convolve([], ch),
                lambda: bank.configure_convolve([h] * 65, ch), lambda: bank.configure_convolve([h], ch, [[0, 1], [0, 0]]),
                lambda: bank.configure_convolve([h], ch, None, 9), lambda: bank.configure_convolve([h, np.ones(4096)], ch, [[0, 0], [0, 0]], 9),
                lambda: bank.configure_convolve([np.array([1.0, np.nan])], ch), lambda: bank.configure_convolve([np.array([np.inf])], ch),
                lambda: bank.configure_convolve([np.ones(4097)], ch), lambda: bank.configure_convolve([h], ch, [[CONVOLVE_BYPASS] * 2] * 2, 1)):
        refused(bad, "convolve_configure")
    refused(lambda: bank.fetch_convolved(0), "fetch_convolved")      # still not configured
    bank.configure_convolve([h], ch, None, 4)
    x = cr.noise(1, n * 64, ch).reshape(n, 64, ch)
    d_in.copy_(torch.from_numpy(x))
    bank.convolve(d_in.data_ptr(), 64, d_out.data_ptr(), 64, frames=[20, 30], stream=stream_of(torch))
    torch.cuda.synchronize()
    before = [bank.fetch_convolved(s).tobytes() for s in range(n)]
    d_out.fill_(float(SENTINEL))
    torch.cuda.synchronize()
    base = d_in.data_ptr()
    for bad in (lambda: bank.convolve(base, 64, d_out.data_ptr(), 64, frames=[65, 1]),                 # frames[s] > frames_capacity
                lambda: bank.convolve(base, 64, d_out.data_ptr(), 10, frames=[11, 0]),                 # beyond out_capacity
                lambda: bank.convolve(base, 2 ** 32, d_out.data_ptr(), 64, frames=[1, 1]),             # a capacity beyond 2^32 - 1
                lambda: bank.convolve(base, 64, d_out.data_ptr(), 2 ** 32, frames=[1, 1]),
                lambda: bank.convolve(0, 64, d_out.data_ptr(), 64, frames=[1, 0]),                     # a null buffer that is needed
                lambda: bank.convolve(base, 64, 0, 64, frames=[1, 0]),
                lambda: bank.convolve(base, 64, base, 64, frames=[1, 1]),                              # any overlap
                lambda: bank.convolve(base, 64, base + 64 * ch * 4 * n - 4, 64, frames=[1, 1]),
                lambda: bank.convolve(base + 4, 32, base, 64, frames=[1, 1])):
        refused(bad)
    refused(lambda: bank.configure_convolve([h], ch), "convolve_configure")      # a stream holds frames
    refused(lambda: bank.fetch_convolved(n), "fetch_convolved")
    torch.cuda.synchronize()
    assert [bank.fetch_convolved(s).tobytes() for s in range(n)] == before
    assert (d_out.cpu().numpy() == SENTINEL).all() and d_in.cpu().numpy().tobytes() == x.tobytes()
    # the state is as it was: the streams go on and end as the whole does
    bank.convolve(d_in.data_ptr() + 20 * ch * 4, 44, d_out.data_ptr(), 64, frames=[44, 0], flush_mask=[1, 0], stream=stream_of(torch))
    torch.cuda.synchronize()
    rec = bank.fetch_convolved(0)
    assert int(rec["frames_in"]) == 64 and int(rec["frames_out"]) == 64 and int(rec["state"]) == cr.FLUSHED and int(rec["frames_written"]) == 48
    want = cr.convolve([h, h], 4, x[0])
    cr.same_floats(d_out.cpu().numpy()[0, :48], want[16:], "after the refusals")
    refused(lambda: bank.convolve(base, 64, d_out.data_ptr(), 64, frames=[1, 0]))      # frames for a flushed stream
    assert bank.convolve(base, 64, d_out.data_ptr(), 64, frames=[0, 0]) != 0            # a call that brings nothing is fine
    assert int(bank.fetch_convolved(0)["frames_written"]) == 0


# ---------------------------------------------------------------- 8. the C99 host
def test_c99_demo_filters_an_impulse_in_two_cuts(tmp_path, omx):
    """tests/c_abi/program_convolve_demo.c: the 255-tap low-pass on a unit impulse, D = 127, two cuts and a flush; the filtered channel
    is the taps centred on the impulse, the bypassed one the impulse where it was (the program's exit code says so)"""
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("response 1000 Hz") and abs(float(lines[0].split()[3])) < 0.01      # the passband
    assert float(lines[2].split()[3]) < -80.0                                                       # 12 kHz: the stopband
    assert "emits 73 312 127" in lines[3]
    assert "frames_in 512 frames_out 512 state 2 delay 127 max_taps 255 peak 1 " in lines[-1] and lines[-1].endswith("wrong 0")

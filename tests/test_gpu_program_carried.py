"""The hand-over between calls of the programme bank's carried stages on the GPU (`-m gpu`): resample, convolve, dynamics and the
limiter share one stream ledger, one ring carry and one record begin (openmeters_amd/csrc/program/program_carried.hpp and
program_stage_device.hpp), and this file drives all four through the calls where that protocol can slip: a ring partly overwritten, a
ring wrapped, a call of nothing, a reset of one stream among running ones, a stream flushed ahead of the others.

Shapes.  3 streams at 2 and at 3 channels, the shortest ring the stage allows beside 8 frames: convolve 9 taps (a ring of 8), the
resampler 2 : 1 at half_width 8 (32 taps, a ring of 31), the limiter attack 1 (rings of 24 frames and 24 values), dynamics attack 3
without hold (rings of 2).  With h the ring's length, every stream's programme has 3 h + 1 frames (at most 4 h + 5) and comes in calls
of h - 1, 0, 1, h and h + 1 frames and an empty flushing call.  Stream 1 is reset by mask behind the second call and goes on as a new
stream; stream 2 is flushed with the call of h frames and brings nothing afterwards.

Bars, each the one of the stage's own GPU file.  Per call the output of every stream against the stage's restatement fed the same
calls (tests/program_*_ref.py, pinned by the CPU files): convolve and dynamics on bytes with a NaN where the restatement has one, the
dynamics trace and the resampler on bytes, the limiter on bits with a NaN for a NaN; behind the last call every record field equal
except the dB fields, within 1e-4 dB.  d_out (and the trace) hold a sentinel beforehand, one frame longer than the longest emission,
and nothing at or beyond frames_written[s] is touched.  No test provokes a fault."""
import numpy as np
import pytest

import program_convolve_ref as cr
import program_dynamics_ref as dr
import program_limit_ref as lr
import program_peaks_ref as pk
import program_resample_ref as rr
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (DYNAMICS_FLUSHED, DYNAMICS_IDLE, DYNAMICS_RUNNING, DynamicsCurve, LimitRule, ProgramLoudnessBank,
                                             ResampleRule)
from test_cpu_program_resample import lib_plan
from test_gpu_program_dynamics import check_record as check_dynamics_record
from test_gpu_program_dynamics import compressor, same_floats as same_dynamics_floats, step_over
from test_gpu_program_limit import gains_on_device, same_floats as same_limit_floats
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
N, FS = 3, 48000.0


class Convolve:
    def __init__(self, torch, omx, oracle, ch):
        taps, delay = cr.random_taps(31, 9), 4
        self.h = len(taps) - 1
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), N, ch, 10)
        self.bank.configure_convolve([taps], ch, None, delay)
        self.refs = [cr.Stream([taps] * ch, delay, len(taps), FLOOR) for _ in range(N)]

    def programme(self, s, frames, ch):
        return cr.noise(40 + s, frames, ch)

    def call(self, d_in, cap, d_out, d_trace, out_cap, counts, flush, stream):
        return self.bank.convolve(d_in, cap, d_out, out_cap, frames=counts, flush_mask=flush, stream=stream)

    def feed(self, s, x, flush):
        return self.refs[s].feed(x, flush=flush), None, None

    def reset(self, mask):
        self.bank.reset_convolve(mask)
        for s in np.flatnonzero(mask):
            self.refs[s].reset()

    def same(self, got, want, E, tag):
        cr.same_floats(got, want, tag)

    def check_record(self, s, tag):
        cr.check_record(self.bank.fetch_convolved(s), self.refs[s].record(), tag, BAR)


class Resample:
    def __init__(self, torch, omx, oracle, ch):
        rate_in, rate_out, half_width = 96000, 48000, 8
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), N, ch, 10)
        self.bank.configure_resampler(ResampleRule(rate_in, rate_out, half_width), ch)
        pl = lib_plan(omx, rate_in, rate_out, half_width=half_width)
        self.h = pl["T"] - 1
        self.refs = [rr.Resampler(pl, ch, FLOOR) for _ in range(N)]

    def programme(self, s, frames, ch):
        return rr.noise(50 + s, frames, ch)

    def call(self, d_in, cap, d_out, d_trace, out_cap, counts, flush, stream):
        return self.bank.resample(d_in, cap, d_out, out_cap, frames=counts, flush_mask=flush, stream=stream)

    def feed(self, s, x, flush):
        return self.refs[s].feed(x, flush=flush), None, None

    def reset(self, mask):
        self.bank.reset_resampler(mask)
        for s in np.flatnonzero(mask):
            self.refs[s].reset()

    def same(self, got, want, E, tag):
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, "output differs from the restatement")

    def check_record(self, s, tag):
        rr.check_record(self.bank.fetch_resampled(s), self.refs[s].record(), tag, BAR)


class Limit:
    GAINS = (2.0, 0.5, 1.5)      # read when a stream takes its first frame, and again behind its reset

    def __init__(self, torch, omx, oracle, ch):
        rule = (lr.CEILING_DB, 1, 0)
        self.h = lr.latency(rule)
        assert self.h == lr.window(rule) + rule[1] - 2 == 24      # the PCM ring's LA and the q ring's W + A - 2
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), N, ch, 10)
        self.bank.configure_limiter(LimitRule(*rule), ch, FS)
        self.d_gains, _ = gains_on_device(torch, self.GAINS)
        coeffs = pk.coefficients(oracle)
        self.refs = [lr.Limiter(rule, FS, coeffs, ch, FLOOR) for _ in range(N)]

    def programme(self, s, frames, ch):
        return lr.noise(60 + s, frames, ch)

    def call(self, d_in, cap, d_out, d_trace, out_cap, counts, flush, stream):
        return self.bank.apply_limited(d_in, cap, d_out, out_cap, self.d_gains.data_ptr(), N, frames=counts, flush_mask=flush, stream=stream)

    def feed(self, s, x, flush):
        return self.refs[s].feed(x, flush=flush, gain=self.GAINS[s], gain_index=s)[0], None, None

    def reset(self, mask):
        self.bank.reset_limiter(mask)
        for s in np.flatnonzero(mask):
            self.refs[s].reset()

    def same(self, got, want, E, tag):
        assert same_limit_floats(got, want), (tag, "output differs from the restatement")

    def check_record(self, s, tag):
        lr.check_record(self.bank.fetch_limited(s), self.refs[s].record(), tag)


class Dynamics:
    def __init__(self, torch, omx, oracle, ch):
        self.ch = ch
        self.curve = dr.Curve(compressor(omx), (1 << ch) - 1, 3, 0, step_over(20.0, 6))
        self.h = self.curve.latency
        assert self.h == self.curve.A + self.curve.H - 1 == 2      # the PCM and r rings, and the Gt ring
        self.bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), N, ch, 10)
        c = self.curve
        self.bank.configure_dynamics([DynamicsCurve(c.T.astype(np.int32), c.mask, c.A, c.H, c.d)], ch)
        self.refs = [dr.Stream(c, ch) for _ in range(N)]
        self.outs = [[] for _ in range(N)]      # what a stream has emitted since its reset
        self.written = [0] * N

    def programme(self, s, frames, ch):
        x = (np.random.default_rng(70 + s).standard_normal((frames, ch)) * 0.003).astype(np.float32)
        x[1 + s::4] *= np.float32(100.0)      # loud frames between quiet ones: the gain falls and is released inside every call
        return x

    def call(self, d_in, cap, d_out, d_trace, out_cap, counts, flush, stream):
        return self.bank.dynamics(d_in, cap, d_out, out_cap, frames=counts, flush_mask=flush, d_gain_db=d_trace, stream=stream)

    def feed(self, s, x, flush):
        out, trace, E = self.refs[s].push(x, flush=flush)
        self.outs[s].append(out)
        self.written[s] = len(out)
        return out, trace, E

    def reset(self, mask):
        self.bank.reset_dynamics(mask)
        for s in np.flatnonzero(mask):
            self.refs[s], self.outs[s], self.written[s] = dr.Stream(self.curve, self.ch), [], 0

    def same(self, got, want, E, tag):
        same_dynamics_floats(got, want, tag, exact=E == 0)      # (a frame with E = 0 is a copy on bits)

    def check_record(self, s, tag):
        r = self.refs[s]
        state = DYNAMICS_FLUSHED if r.flushed else (DYNAMICS_RUNNING if r.n else DYNAMICS_IDLE)
        want = dict(dr.record(r.E_all, np.concatenate(self.outs[s] + [np.zeros((0, self.ch), np.float32)])), frames_in=r.n, frames_out=r.e,
                    frames_written=self.written[s], state=state, latency_frames=self.curve.latency, curve_index=0)
        check_dynamics_record(self.bank.fetch_dynamics(s), want, tag)


@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("stage", [Resample, Convolve, Dynamics, Limit], ids=lambda c: c.__name__.lower())
def test_hand_over_between_calls(torch_dev, omx, oracle, stage, ch):
    torch = torch_dev
    st = stage(torch, omx, oracle, ch)
    h = st.h
    sizes = [h - 1, 0, 1, h, h + 1, 0]
    xs = [st.programme(s, sum(sizes), ch) for s in range(N)]
    at = [0] * N
    flushed_early = False
    for k, size in enumerate(sizes):
        last = k == len(sizes) - 1
        counts = [size, size, 0 if flushed_early else size]
        flush = [1, 1, 1] if last else ([0, 0, 1] if size == h else None)
        rows = [x[a:a + f] for x, a, f in zip(xs, at, counts)]
        wants = [st.feed(s, rows[s], bool(flush and flush[s])) for s in range(N)]
        emits = [len(want[0]) for want in wants]
        cap, out_cap = max(max(counts), 1), max(emits) + 1
        host = cr.noise(900 + k, N * cap, ch).reshape(N, cap, ch)      # frames of d_in beyond frames[s] hold other samples
        for s, r in enumerate(rows):
            host[s, :len(r)] = r
        d_in = torch.from_numpy(host).cuda()
        d_out = torch.full((N, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
        d_trace = torch.full((N, out_cap), float(SENTINEL), dtype=torch.float32).cuda()
        st.call(d_in.data_ptr(), cap, d_out.data_ptr(), d_trace.data_ptr(), out_cap, counts, flush, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got, got_trace = d_out.cpu().numpy(), d_trace.cpu().numpy()
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
        for s in range(N):
            tag = (stage.__name__, ch, "call", k, counts, "stream", s)
            (out, trace, E), w = wants[s], emits[s]
            assert (got[s, w:] == SENTINEL).all(), (tag, "floats at or beyond frames_written[s] * channels were written")
            if trace is not None:
                assert got_trace[s, :w].tobytes() == trace.tobytes() and (got_trace[s, w:] == SENTINEL).all(), (tag, "the trace")
            st.same(got[s, :w], out, E, tag)
            st.check_record(s, tag)
            at[s] += counts[s]
        if k == 1:
            st.reset([0, 1, 0])      # stream 1 starts over among running ones; what it is fed next is a new stream's first frame
            for s in range(N):
                st.check_record(s, (stage.__name__, ch, "behind the reset of stream 1", "stream", s))
        flushed_early = flushed_early or size == h
    assert at == [sum(sizes), sum(sizes), sum(sizes[:4])]

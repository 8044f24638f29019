"""Programme bank sample-rate conversion on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_resampler / resample /
reset_resampler / fetch_resampled against the numpy restatement (tests/program_resample_ref.py, pinned by
tests/test_cpu_program_resample.py), which runs on the LIBRARY's tap table here.

Bars.  Every float of the output equals the restatement's, bit for bit (NaN payloads included: the comparison is on bytes); every
record field equal except out_sample_peak_db, within 1e-4 dB (the family's bar).  Not written: d_out is filled with a sentinel float
beforehand and every float at or beyond frames_written[s] keeps it; d_in is unchanged.  Cut invariance: the concatenated output of any
schedule of calls is the one-call output, and the final records are equal.  Chain: `process` measures the device's output exactly as
it measures the restated output uploaded from the host.
The plan's tile_frames is the main kernel's tile; rr.lengths_beside_a_tile puts a stream's emission one frame either side of a tile's
end.  No test provokes a fault: the refusals use only arguments the host rejects before any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_pcm_ref as pr
import program_resample_ref as rr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (RESAMPLE_RECORD_DTYPE, ExportRule, GainRule, LimitRule, ProgramLoudnessBank, ResampleRule,
                                             resample_frames, resample_plan)
from test_cpu_program_resample import PAIRS, lib_plan
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
CHANNELS = (1, 2, 3, 8)
RATES = [(a, b) for a, b, *_ in PAIRS]      # L / M = 160/147, 147/160, 1/2, 2/1, 147/640


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def first_difference(got, want):
    g, w = got.reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)
    at = int(np.flatnonzero(g != w)[0])
    return at, got.reshape(-1)[max(at - 2, 0):at + 4], want.reshape(-1)[max(at - 2, 0):at + 4]


def run_call(torch, bank, rows, ch, flush=None, out_cap=None, filler=999):
    """rows[s]: f32 [frames][ch] of stream s in this call; frames of d_in beyond them hold other samples.  d_out holds the sentinel
    beforehand.  Checks that d_in is unchanged and that nothing at or beyond frames_written[s] was written.
    -> (per stream the frames written, the device pointer to the records)"""
    n = len(rows)
    counts = [len(r) for r in rows]
    cap = max(max(counts), 1)
    host = pr.noise(filler, n * cap, ch).reshape(n, cap, ch)
    for s, r in enumerate(rows):
        host[s, :len(r)] = r
    if out_cap is None:
        out_cap = max(max(int(bank.fetch_resampled(s)["frames_in"]) + counts[s] for s in range(n)) * bank._rs_L // bank._rs_M + 2, 1)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
    ptr = bank.resample(d_in.data_ptr(), cap, d_out.data_ptr(), out_cap, frames=counts, flush_mask=flush, stream=stream_of(torch))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    out = []
    for s in range(n):
        w = int(bank.fetch_resampled(s)["frames_written"])
        assert (got[s, w:] == SENTINEL).all(), (s, w, "frames at or beyond frames_written[s] were written")
        out.append(got[s, :w].copy())
    return out, ptr


def configured(omx, n, ch, rate_in, rate_out, **kw):
    bank = new_bank(omx, n, ch)
    bank.configure_resampler(ResampleRule(rate_in, rate_out, **kw), ch)
    info = resample_plan(omx, ResampleRule(rate_in, rate_out, **kw))
    bank._rs_L, bank._rs_M = int(info["L"]), int(info["M"])      # (run_call sizes d_out with them)
    return bank, lib_plan(omx, rate_in, rate_out, **kw)


def check_stream(bank, s, got, pl, x, ch, tag, flushed=True):
    r = rr.Resampler(pl, ch, FLOOR)
    want = r.feed(x, flush=flushed)
    assert got.shape == want.shape, (tag, s, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        raise AssertionError((tag, s, "output differs from the restatement", first_difference(got, want)))
    rr.check_record(bank.fetch_resampled(s), r.record(), (tag, s), BAR)
    return r.record()


# ---------------------------------------------------------------- 1. bits, records, nothing else written
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("rates", RATES)
def test_output_and_records_equal_the_restatement(torch_dev, omx, rates, ch):
    """streams of 0, 1, H, H + 1 and 1001 frames and streams whose emission ends one output frame either side of a tile's end, flushed
    and not flushed; noise at +-1, one row with a NaN and infinities; with 8 channels also 5 streams x 3 tiles"""
    rate_in, rate_out = rates
    pl = rr.plan(rate_in, rate_out)
    H, tile = pl["H"], pl["tile"]
    shapes = [([0, 1, H, H + 1, 1001] + rr.lengths_beside_a_tile(pl, tile, 1, True), True),
              ([1001, 0] + rr.lengths_beside_a_tile(pl, tile, 1, False) + [H, 1], False)]
    if ch == 8:
        ends = rr.lengths_beside_a_tile(pl, tile, 3, True)
        shapes.append(([ends[0], ends[-1], ends[0] - 300, 0, ends[-1] - 1], True))
    over = 0
    for k, (lengths, flush) in enumerate(shapes):
        n = len(lengths)
        bank, pl = configured(omx, n, ch, rate_in, rate_out)
        for s in range(n):
            idle = bank.fetch_resampled(s)
            want = np.array([(0, 0, 0, 0, 0.0, FLOOR, rr.IDLE, pl["L"], pl["M"], pl["T"], pl["H"], 0)], RESAMPLE_RECORD_DTYPE)
            assert idle.tobytes() == want.tobytes(), idle
        xs = [rr.hard(100 * ch + 10 * k + s, f, ch) if s == 4 else rr.noise(100 * ch + 10 * k + s, f, ch) for s, f in enumerate(lengths)]
        got, ptr = run_call(torch_dev, bank, xs, ch, flush=[1] * n if flush else None)
        for s, x in enumerate(xs):
            rec = check_stream(bank, s, got[s], pl, x, ch, (rates, ch, lengths, flush), flushed=flush)
            assert rec["frames_out"] == rr.emitted(pl, len(x), 0, flush) == resample_frames(omx, ResampleRule(rate_in, rate_out), 0, 0, len(x), flush)
            over += rec["samples_over"]
        assert device_bytes(ptr, n * 64) == b"".join(bank.fetch_resampled(s).tobytes() for s in range(n))
        if ch == 8 and k == 2:
            assert max(len(g) for g in got) > 2 * tile
    assert over > 0


# ---------------------------------------------------------------- 2. cut invariance
def fit(schedule, xs):
    """the calls of `schedule` clipped to what every stream has left"""
    left, out = [len(x) for x in xs], []
    for counts in schedule:
        row = [min(int(c), l) for c, l in zip(counts, left)]
        left = [l - r for l, r in zip(left, row)]
        out.append(row)
    return out, left


def in_calls(torch, bank, xs, ch, schedule, flush_in_last):
    """the schedule, then the rest; the flush in the call that brings the last frames, or in a call of its own that brings none"""
    n = len(xs)
    calls, left = fit(schedule, xs)
    calls.append(left)
    taken, parts = [0] * n, [[] for _ in xs]
    for i, counts in enumerate(calls):
        last = i == len(calls) - 1
        rows = [xs[s][taken[s]:taken[s] + f] for s, f in enumerate(counts)]
        got, _ = run_call(torch, bank, rows, ch, flush=[1] * n if (last and flush_in_last) else None)
        for s, f in enumerate(counts):
            parts[s].append(got[s])
            taken[s] += f
    if not flush_in_last:
        got, _ = run_call(torch, bank, [x[:0] for x in xs], ch, flush=[1] * n)
        for s in range(n):
            parts[s].append(got[s])
    assert all(taken[s] == len(x) for s, x in enumerate(xs))
    return [np.concatenate(p) for p in parts]


@pytest.mark.parametrize("rates,ch", [((44100, 48000), 2), ((48000, 44100), 3), ((96000, 48000), 8), ((48000, 96000), 1), ((192000, 44100), 2)])
def test_output_does_not_depend_on_the_cuts(torch_dev, omx, rates, ch):
    rate_in, rate_out = rates
    pl0 = rr.plan(rate_in, rate_out)
    T, tile = pl0["T"], pl0["tile"]
    lengths = [(2 * tile + 77) * pl0["M"] // pl0["L"], 4 * T + 333, 1001]
    n = len(lengths)
    bank, pl = configured(omx, n, ch, rate_in, rate_out)
    xs = [rr.hard(300 + s, f, ch) if s == 1 else rr.noise(300 + s, f, ch) for s, f in enumerate(lengths)]
    whole = in_calls(torch_dev, bank, xs, ch, [], True)
    records = [bank.fetch_resampled(s) for s in range(n)]
    for s, x in enumerate(xs):
        want = rr.resample(pl, x)
        assert whole[s].tobytes() == want.tobytes(), (s, first_difference(whole[s], want))
    rng = np.random.default_rng(5)
    named = [[0] * n, [1] * n, [3] * n, [T - 2] * n, [T - 1] * n, [T] * n]
    small = [[5, 0, 1], [7, 3, 0]] * 12 + [[T - 2] * n] * 3      # pieces smaller than the carry, several in a row
    ragged = [[int(rng.integers(0, 900)) if rng.random() < 0.7 else 0 for _ in range(n)] for _ in range(5)]
    for name, schedule, flush_in_last in (("0, 1, 3, T - 2, T - 1, T", named, True), ("0, 1, 3, T - 2, T - 1, T; flush alone", named, False),
                                          ("smaller than the carry", small, False), ("ragged", ragged, True)):
        bank.reset_resampler()
        assert all(int(bank.fetch_resampled(s)["frames_in"]) == 0 and int(bank.fetch_resampled(s)["state"]) == rr.IDLE for s in range(n))
        parts = in_calls(torch_dev, bank, xs, ch, schedule, flush_in_last)
        for s in range(n):
            assert parts[s].tobytes() == whole[s].tobytes(), (rates, ch, name, s, first_difference(parts[s], whole[s]))
            got = bank.fetch_resampled(s)
            for f in rr.RECORD_FIELDS:
                if f != "frames_written":
                    assert got[f].tobytes() == records[s][f].tobytes(), (name, s, f, got[f], records[s][f])


# ---------------------------------------------------------------- 3. per-stream state
def test_streams_keep_their_own_state(torch_dev, omx):
    ch, n = 2, 3
    bank, pl = configured(omx, n, ch, 44100, 48000)
    xs = [rr.noise(40 + s, 2000, ch) for s in range(n)]
    refs = [rr.Resampler(pl, ch, FLOOR) for _ in range(n)]
    got, _ = run_call(torch_dev, bank, [x[:700] for x in xs], ch)
    for s in range(n):
        assert got[s].tobytes() == refs[s].feed(xs[s][:700]).tobytes()
    bank.reset_resampler([0, 1, 0])      # stream 1 starts over, the others run on
    refs[1].reset()
    assert [int(bank.fetch_resampled(s)["frames_in"]) for s in range(n)] == [700, 0, 700]
    assert [int(bank.fetch_resampled(s)["state"]) for s in range(n)] == [rr.RUNNING, rr.IDLE, rr.RUNNING]
    rows = [xs[0][700:1500], xs[1][:900], xs[2][700:700]]
    got, _ = run_call(torch_dev, bank, rows, ch, flush=[0, 0, 1])
    for s in range(n):
        assert got[s].tobytes() == refs[s].feed(rows[s], flush=(s == 2)).tobytes(), s
        rr.check_record(bank.fetch_resampled(s), refs[s].record(), s, BAR)
    assert int(bank.fetch_resampled(2)["state"]) == rr.FLUSHED
    before = [bank.fetch_resampled(s).tobytes() for s in range(n)]
    with pytest.raises(capi.OmxError) as err:      # a flushed stream takes no frames
        run_call(torch_dev, bank, [xs[0][1500:1600], xs[1][900:1000], xs[2][700:800]], ch, out_cap=400)
    assert err.value.status == capi.ERR_INVALID
    assert [bank.fetch_resampled(s).tobytes() for s in range(n)] == before
    got, _ = run_call(torch_dev, bank, [xs[0][1500:], xs[1][900:], xs[2][:0]], ch, flush=[1, 1, 0])      # it still takes a call of none
    assert len(got[2]) == 0
    for s in (0, 1):
        assert got[s].tobytes() == refs[s].feed([xs[0][1500:], xs[1][900:]][s], flush=True).tobytes()
    bank.reset_resampler([0, 0, 1])
    got, _ = run_call(torch_dev, bank, [xs[0][:0], xs[1][:0], xs[2]], ch, flush=[0, 0, 1])
    assert got[2].tobytes() == rr.resample(pl, xs[2]).tobytes()


# ---------------------------------------------------------------- 4. the chain, and the measurement state
def records_of(bank):
    return [record_array(bank.fetch(s)).tobytes() for s in range(bank.n_streams)]


def test_resample_then_process_measures_what_the_restated_output_measures(torch_dev, omx):
    """44.1 -> 48 kHz on the device, then process at 48 kHz: the programme records and the segment energies are those of process fed
    the restatement's output from the host.  Every record of the earlier headers has the same bytes before and after the new calls."""
    ch, n, fs_out = 2, 3, 48000.0
    pos = capi.positions_fallback(ch)
    lengths = [44100, 30000, 22051]
    bank, pl = configured(omx, n, ch, 44100, 48000)
    xs = []
    for s, f in enumerate(lengths):      # a tone under a slow gate plus a little noise: every stream completes gating blocks
        t = np.arange(f)
        tone = 0.25 * np.sin(2 * np.pi * 997.0 * t / 44100.0) * ((t // 9000) % 2 + 1) / 2.0
        xs.append((tone[:, None] + 0.01 * rr.noise(80 + s, f, ch)).astype(np.float32))
    # the earlier headers' state, made first: a measurement, a plan, an apply, a limiter call, an export
    d_some = torch_dev.from_numpy(np.stack([x[:22051] for x in xs])).cuda()
    bank.set_peaks(True)
    bank.process(d_some.data_ptr(), 22051, ch, 44100.0, pos, stream=stream_of(torch_dev))
    ptr = bank.plan_gains(GainRule(-20.0, -1.0, -60.0, 60.0, 0), stream=stream_of(torch_dev))
    d_tmp = torch_dev.zeros((n, 22051, ch), dtype=torch_dev.float32).cuda()
    bank.apply_gains(d_some.data_ptr(), d_tmp.data_ptr(), 22051, ch, ptr, n, stream=stream_of(torch_dev))
    bank.configure_limiter(LimitRule(-1.0, 64, 0), ch, 44100.0)
    bank.apply_limited(d_some.data_ptr(), 22051, d_tmp.data_ptr(), 22051, ptr, n, flush_mask=[1] * n, stream=stream_of(torch_dev))
    bank.configure_export(ExportRule(pr.S16, pr.TPDF, 3), ch)
    d_pcm = torch_dev.zeros((n * 22051 * ch * 2,), dtype=torch_dev.uint8).cuda()
    bank.export_pcm(d_tmp.data_ptr(), d_pcm.data_ptr(), 22051, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()

    def state():
        return (records_of(bank), [bank.fetch_peaks(s).tobytes() for s in range(n)], bank.fetch_gains().tobytes(),
                [bank.fetch_applied(s).tobytes() for s in range(n)], [bank.fetch_limited(s).tobytes() for s in range(n)],
                [bank.fetch_exported(s).tobytes() for s in range(n)])

    before = state()
    cap, out_cap = max(lengths), 48000
    host = np.zeros((n, cap, ch), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    d_in = torch_dev.from_numpy(host).cuda()
    d_out = torch_dev.full((n, out_cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.resample(d_in.data_ptr(), cap, d_out.data_ptr(), out_cap, frames=lengths, flush_mask=[1] * n, stream=stream_of(torch_dev))
    bank.reset_resampler([1, 0, 0])
    torch_dev.cuda.synchronize()
    assert state() == before, "a call of program_resample.h changed a record of an earlier header"
    wants = [rr.resample(pl, x) for x in xs]
    emitted = [len(w) for w in wants]
    assert emitted == [48000, 32654, 24002]
    got = d_out.cpu().numpy()
    restated = np.zeros((n, out_cap, ch), np.float32)
    for s, w in enumerate(wants):
        assert got[s, :len(w)].tobytes() == w.tobytes(), s
        restated[s, :len(w)] = w
    via, direct = new_bank(omx, n, ch, fs_out), new_bank(omx, n, ch, fs_out)
    for b in (via, direct):
        b.set_peaks(True)
    via.process(d_out.data_ptr(), out_cap, ch, fs_out, pos, frames=emitted, stream=stream_of(torch_dev))
    d_host = torch_dev.from_numpy(restated).cuda()
    direct.process(d_host.data_ptr(), out_cap, ch, fs_out, pos, frames=emitted, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert records_of(via) == records_of(direct)
    assert [via.fetch_peaks(s).tobytes() for s in range(n)] == [direct.fetch_peaks(s).tobytes() for s in range(n)]
    for s in range(n):
        assert via.fetch_segments(s).tobytes() == direct.fetch_segments(s).tobytes(), s
        assert len(via.fetch_segments(s)) == emitted[s] // 4800
    assert all(np.isfinite(direct.fetch(s).integrated_lufs) and direct.fetch(s).integrated_lufs > -40.0 for s in range(n))


# ---------------------------------------------------------------- 5. refusals
def test_refused_calls_change_nothing(torch_dev, omx):
    ch, n, cap, out_cap = 2, 3, 400, 500
    x = np.stack([rr.noise(70 + s, cap, ch, 0.8) for s in range(n)])
    in_bytes, out_bytes = x.size * 4, n * out_cap * ch * 4
    store = torch_dev.full(((in_bytes + out_bytes) // 4 + 16,), float(SENTINEL), dtype=torch_dev.float32).cuda()
    store[:x.size] = torch_dev.from_numpy(x.reshape(-1)).cuda()
    d_in, d_out = store.data_ptr(), store.data_ptr() + in_bytes
    bank = new_bank(omx, n, ch)
    good = dict(d_in=d_in, frames_capacity=cap, d_out=d_out, out_capacity=out_cap, frames=[300, 0, 150])
    for call in (lambda: bank.resample(**good), lambda: bank.fetch_resampled(0), lambda: bank.reset_resampler()):      # before configure
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID
    for bad, status in ((dict(rate_in=48000, rate_out=48000), capi.ERR_INVALID), (dict(half_width=7), capi.ERR_INVALID),
                        (dict(beta=21.0), capi.ERR_INVALID), (dict(cutoff=0.5), capi.ERR_INVALID), (dict(flags=1), capi.ERR_INVALID),
                        (dict(rate_in=44101), capi.ERR_UNSUPPORTED), (dict(rate_in=3000), capi.ERR_UNSUPPORTED),
                        (dict(rate_in=768000, rate_out=12000, half_width=10), capi.ERR_UNSUPPORTED)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_resampler(ResampleRule(**bad), ch)
        assert err.value.status == status, bad
    for channels in (0, 9):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_resampler(ResampleRule(), channels)
        assert err.value.status == capi.ERR_INVALID, channels
    with pytest.raises(capi.OmxError):
        bank.fetch_resampled(0)                                         # a refused configure configured nothing
    bank.configure_resampler(ResampleRule(), ch)
    bank.configure_resampler(ResampleRule(96000, 48000), ch)            # again, while no stream holds frames
    bank.configure_resampler(ResampleRule(), ch)
    ptr = bank.resample(**good)
    torch_dev.cuda.synchronize()
    everything, records = store.cpu().numpy().tobytes(), device_bytes(ptr, n * 64)
    assert [int(bank.fetch_resampled(s)["frames_in"]) for s in range(n)] == [300, 0, 150]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert store.cpu().numpy().tobytes() == everything, tag
        assert device_bytes(ptr, n * 64) == records, tag

    bad_calls = {"d_out inside d_in": dict(d_out=d_in + 4), "d_out one float below the end of d_in": dict(d_out=d_in + in_bytes - 4),
                 "d_in inside d_out": dict(d_in=d_out + 8), "the same buffer": dict(d_out=d_in),
                 "frames[s] > frames_capacity": dict(frames=[cap + 1, 0, 0]),
                 "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                 "out_capacity beyond 2^32 - 1": dict(out_capacity=2 ** 32, frames=[0, 0, 1]),
                 "more than out_capacity": dict(out_capacity=100, frames=[100, 0, 0]),
                 "more than out_capacity in a flush": dict(out_capacity=10, frames=[0, 0, 0], flush_mask=[1, 0, 0]),
                 "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.resample(**{**good, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    raw_fn = omx.fn("program_loudness_bank_resample", C.c_int,
                    [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p])
    counts = np.array([1, 1, 1], np.uint32)
    assert raw_fn(bank._h, C.c_void_p(d_in), cap, counts.ctypes.data, C.c_void_p(d_out), out_cap, None, None, None) == capi.ERR_INVALID      # null d_resampled
    unchanged("null d_resampled")
    with pytest.raises(capi.OmxError) as err:                           # configure while a stream holds frames
        bank.configure_resampler(ResampleRule(96000, 48000), ch)
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_resampled(n)
    assert err.value.status == capi.ERR_INVALID
    unchanged("configure while a stream holds frames")
    # a null d_out is accepted where no stream emits, a null d_in where none brings frames
    bank.resample(d_in=0, frames_capacity=cap, d_out=0, out_capacity=0, frames=[0, 0, 0])
    bank.resample(d_in=d_in, frames_capacity=cap, d_out=0, out_capacity=0, frames=[0, 10, 0])
    # none of the refusals moved the host's mirror: the streams go on where they stood
    pl = lib_plan(omx, 44100, 48000)
    bank._rs_L, bank._rs_M = pl["L"], pl["M"]
    got, _ = run_call(torch_dev, bank, [x[0, 300:400], x[1, 10:60], x[2, 150:150]], ch, flush=[1, 1, 1])
    for s, (upto, part) in enumerate(((400, 300), (60, 0), (150, 150))):
        whole = rr.resample(pl, x[s, :upto])
        held = rr.emitted(pl, part, 0, False)
        assert got[s].tobytes() == whole[held:].tobytes(), s
    bank.reset_resampler()
    bank.configure_resampler(ResampleRule(96000, 48000), ch)            # after a reset of every stream it is allowed again
    assert int(bank.fetch_resampled(0)["taps"]) == 128


# ---------------------------------------------------------------- 6. the C99 host
def demo_programme():
    state, out = 12345, np.zeros(88200 * 2, np.int16)
    for i in range(out.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        v = ((state >> 16) & 0x3FFF) - 8192
        out[i] = 3 * v if (i // 2) % 22050 < 2205 else v
    return out


def test_c99_demo_prints_the_python_routes_records(torch_dev, omx, tmp_path):
    """tests/c_abi/program_resample_demo.c: import S16 at 44.1 kHz, the conversion to 48 kHz in two calls, process, plan_gains,
    apply_limited and the export as S24 from a plain C host"""
    from test_cpu_program_resample import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    printed = {tok[i]: tok[i + 1] for i in range(0, len(tok), 2)}
    ch, frames_in, frames_out, first = 2, 88200, 96000, 50000
    rule = ResampleRule()
    bank = new_bank(omx, 1, ch, 48000.0)
    d_pcm = torch_dev.from_numpy(demo_programme().view(np.uint8).copy()).cuda()
    d_f32 = torch_dev.zeros((frames_in, ch), dtype=torch_dev.float32).cuda()
    d_48k, d_lim = (torch_dev.zeros((1, frames_out, ch), dtype=torch_dev.float32).cuda() for _ in range(2))
    d_out = torch_dev.zeros((frames_out * ch * 3,), dtype=torch_dev.uint8).cuda()
    bank.import_pcm(d_pcm.data_ptr(), pr.S16, d_f32.data_ptr(), frames_in, ch)
    bank.configure_resampler(rule, ch)
    first_out = resample_frames(omx, rule, 0, 0, first, False)
    bank.resample(d_f32.data_ptr(), frames_in, d_48k.data_ptr(), frames_out, frames=[first])
    bank.resample(d_f32.data_ptr() + first * ch * 4, frames_in - first, d_48k.data_ptr() + first_out * ch * 4, frames_out - first_out,
                  frames=[frames_in - first], flush_mask=[1])
    bank.process(d_48k.data_ptr(), frames_out, ch, 48000.0, capi.positions_fallback(ch))
    ptr = bank.plan_gains(GainRule(-10.0, -1.0, -60.0, 60.0, 0))
    bank.configure_limiter(LimitRule(-1.0, 64, 0), ch, 48000.0)
    bank.apply_limited(d_48k.data_ptr(), frames_out, d_lim.data_ptr(), frames_out, ptr, 1, flush_mask=[1])
    bank.configure_export(ExportRule(pr.S24, pr.TPDF, 2024), ch)
    bank.export_pcm(d_lim.data_ptr(), d_out.data_ptr(), frames_out)
    torch_dev.cuda.synchronize()
    s, rec, g, lim, e = bank.fetch_resampled(0), bank.fetch(0), bank.fetch_gains()[0], bank.fetch_limited(0), bank.fetch_exported(0)
    checksum = 1469598103934665603
    for byte in d_out.cpu().numpy().tobytes():
        checksum = ((checksum ^ byte) * 1099511628211) & (2 ** 64 - 1)
    want = {"L": "160", "M": "147", "taps": "64", "latency": "32", "resampled_in": str(int(s["frames_in"])), "resampled_out": str(int(s["frames_out"])),
            "resampled_written": str(int(s["frames_written"])), "resampled_over": str(int(s["samples_over"])),
            "resampled_peak": f"{float(s['out_sample_peak']):.6f}", "state": str(int(s["state"])), "integrated_lufs": f"{float(rec.integrated_lufs):.4f}",
            "gain_db": f"{float(g['gain_db']):.4f}", "frames_limited": str(int(lim["frames_limited"])), "min_envelope": f"{float(lim['min_envelope']):.6f}",
            "frames_out": str(int(e["frames_out"])), "samples_clipped": str(int(e["samples_clipped"])), "out_peak": str(int(e["out_peak"])),
            "format": "2", "checksum": str(checksum)}
    assert printed == want, (printed, want)
    assert (int(s["frames_in"]), int(s["frames_out"]), int(s["frames_written"]), int(s["state"])) == (frames_in, frames_out, frames_out - first_out, rr.FLUSHED)
    # the device's 48 kHz programme is the restatement's
    pl = lib_plan(omx, 44100, 48000)
    x = pr.import_pcm(demo_programme().tobytes(), pr.S16, ch)
    assert d_48k.cpu().numpy()[0].tobytes() == rr.resample(pl, x).tobytes()

"""Programme bank long-term spectrum on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_spectrum / reset_spectrum /
spectrum / fetch_spectrum against the numpy restatement (tests/program_spectrum_ref.py, pinned by tests/test_cpu_program_spectrum.py).

Bars.  The restatement works in f64 (np.fft.rfft of the f32 window times the f32 samples, |.|^2, summed); the device transforms in
f32.  The project's bars for f32 spectra ("spectrum traces": 1e-5 of the row maximum, 0.01 dB within 60 dB of
the maximum) carried to sums: per stream and channel |S - S_ref| <= 1e-5 * (the sum over the transforms of the largest bin of each),
and |dB| <= 0.01 for the bins within 60 dB of the channel's largest.  Records (integers) equal the restatement's on bytes.  Every
cutting of a programme into calls gives the bytes of the whole, records and sums.  Every test prints the worst case it saw.
Shapes.  N = 2048 (H = 1024) unless said otherwise; programmes of 7 H + 333 frames: a handful of transforms, a frame that
straddles the carried frames and the call's, an open run; 2 R H + N + 5 frames at N = 8192: a full run, an open run and the chain.
No test provokes a fault: the refusals use only arguments the host rejects before any launch."""
import re
import subprocess

import numpy as np
import pytest

import program_spectrum_ref as sr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (ProgramLoudnessBank, SpectrumMatchSpec, SpectrumRule, spectrum_density,
                                             spectrum_match, spectrum_plan, spectrum_transforms, spectrum_window)
from test_cpu_program_spectrum import build_demo
from test_gpu_program_loudness import torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes

pytestmark = pytest.mark.gpu
N = 2048
H = N // 2
FS = 48000.0
SUM_BAR, DB_BAR = 1e-5, 0.01


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n_streams, ch, n=N):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), n_streams, 2, 10)
    bank.configure_spectrum(SpectrumRule(n), ch)
    return bank


def signal(kind, seed, frames, ch, n=N):
    """white noise, a sine between two bins, an impulse train, DC: f32 [frames][ch], every channel its own level"""
    t = np.arange(frames, dtype=np.float64)
    if kind == "noise":
        return sr.noise(seed, frames, ch, 0.8)
    if kind == "sine":
        x = np.stack([0.7 / (c + 1) * np.sin(2 * np.pi * (100.5 + 37 * c) / n * t + c) for c in range(ch)], 1)
    elif kind == "impulses":
        x = np.stack([np.where((t.astype(np.int64) + 13 * c) % 777 == 0, 0.9 / (c + 1), 0.0) for c in range(ch)], 1)
    else:
        x = np.stack([np.full(frames, 0.25 * (-1) ** c / (c + 1)) for c in range(ch)], 1)
    return x.astype(np.float32)


KINDS = ("noise", "sine", "impulses", "dc")


def call(torch, bank, rows, ch, finish=None, check_input=False, lead=0, slack=0, filler=999):
    """rows[s]: f32 [frames][ch] of stream s in this call.  d_in starts `lead` floats into its allocation, holds `slack` more frames
    per stream than the longest row, and everything around the rows is noise.  -> (status, d_records, d_sums)"""
    n = len(rows)
    counts = [len(r) for r in rows]
    cap = max(max(counts), 1) + slack
    host = sr.noise(filler, lead + n * cap * ch + 4, 1)[:, 0]
    body = host[lead:lead + n * cap * ch].reshape(n, cap, ch)
    for s, r in enumerate(rows):
        body[s, :len(r)] = r
    dev = torch.from_numpy(host).cuda()
    out = bank.spectrum(dev.data_ptr() + 4 * lead, cap, frames=counts, finish_mask=finish, stream=stream_of(torch))
    torch.cuda.synchronize()
    if check_input:
        assert dev.cpu().numpy().tobytes() == host.tobytes(), "d_in, or the memory around it, changed"
    return out


def feed(torch, bank, xs, ch, pieces, finish=False):
    """every stream walks its own programme xs[s] in its own pieces[s] (frame counts; streams that have run out bring 0 frames);
    -> calls in which no stream completed a transform"""
    at, idle_calls = [0] * len(xs), 0
    for i in range(max(len(p) for p in pieces)):
        rows = []
        for s, x in enumerate(xs):
            f = pieces[s][i] if i < len(pieces[s]) else 0
            rows.append(x[at[s]:at[s] + f])
            at[s] += f
        before = [int(bank.fetch_spectrum(s)[0]["transforms"][0]) for s in range(len(xs))] if i < 12 else None
        status, _, _ = call(torch, bank, rows, ch)
        assert status == (1 if any(len(r) for r in rows) else 0)
        if before is not None and before == [int(bank.fetch_spectrum(s)[0]["transforms"][0]) for s in range(len(xs))]:
            idle_calls += 1
    assert at == [len(x) for x in xs], "the pieces do not add up to the programmes"
    if finish:
        status, _, _ = call(torch, bank, [x[:0] for x in xs], ch, finish=[1] * len(xs))
        assert status == 1
    return idle_calls


def snapshot(bank, n_streams):
    out = []
    for s in range(n_streams):
        rec, sums = bank.fetch_spectrum(s)
        out.append(rec.tobytes() + sums.tobytes())
    return out


def check_against_restatement(bank, s, x, n, finished, w, worst, tag):
    """records on bytes, sums at the two bars; worst: [sum error over its bar's scale, dB]"""
    rec, sums = bank.fetch_spectrum(s)
    want_rec, want, scale = sr.record(x, n, finished, w)
    assert rec.tobytes() == want_rec.tobytes(), (tag, s, "record", rec, want_rec)
    for c in range(x.shape[1]):
        if scale[c] == 0.0:
            assert not sums[c].any(), (tag, s, c, "sums without a transform")
            continue
        err = float(np.abs(sums[c] - want[c]).max() / scale[c])
        near = want[c] >= want[c].max() * 1e-6
        db = float(np.abs(10 * np.log10(sums[c][near] / want[c][near])).max())
        worst[0], worst[1] = max(worst[0], err), max(worst[1], db)
        assert err <= SUM_BAR and db <= DB_BAR, (tag, s, c, err, db)


# ---------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("n_streams,ch,n", [(1, 1, N), (3, 2, N), (65, 3, N), (3, 8, N), (2, 2, 4096), (2, 1, 8192)])
def test_sums_meet_the_f32_bars_against_the_restatement(torch_dev, omx, n_streams, ch, n):
    h = n // 2
    w = spectrum_window(omx, n)
    assert w.tobytes() == sr.window(n).tobytes()
    lengths = [7 * h + 333, 0, n - 1, n, 3 * h + 1, 18 * h + 5]
    xs = [signal(KINDS[s % 4], 10 * s + ch, lengths[s % len(lengths)] if n_streams > 1 else 7 * h + 333, ch, n) for s in range(n_streams)]
    bank = new_bank(omx, n_streams, ch, n)
    status, d_rec, d_sums = call(torch_dev, bank, xs, ch, check_input=True)
    assert status == 1
    worst = [0.0, 0.0]
    for s, x in enumerate(xs):
        check_against_restatement(bank, s, x, n, False, w, worst, "open")
    assert device_bytes(d_rec, n_streams * 152) == b"".join(bank.fetch_spectrum(s)[0].tobytes() for s in range(n_streams))
    assert device_bytes(d_sums, n_streams * ch * (h + 1) * 8) == b"".join(bank.fetch_spectrum(s)[1].tobytes() for s in range(n_streams))
    call(torch_dev, bank, [x[:0] for x in xs], ch, finish=[1] * n_streams)
    for s, x in enumerate(xs):
        check_against_restatement(bank, s, x, n, True, w, worst, "finished")
        assert int(bank.fetch_spectrum(s)[0]["transforms"][0]) == spectrum_transforms(omx, len(x), True, n)
    print(f"N {n}, {n_streams} streams x {ch} ch: worst sum error {worst[0]:.3g} of the scale (bar {SUM_BAR}), worst dB {worst[1]:.3g} (bar {DB_BAR})")


def test_a_quiet_channel_keeps_its_own_bars(torch_dev, omx):
    """the second channel lies 120 dB under the first and holds other content: its bars are taken against ITS OWN maxima, which a
    transform that packed both channels into one complex transform would miss by orders of magnitude"""
    frames = 7 * H + 333
    loud = signal("noise", 3, frames, 1)
    quiet = (signal("sine", 4, frames, 1).astype(np.float64) * 1e-6).astype(np.float32)
    x = np.concatenate([loud, quiet], 1)
    bank = new_bank(omx, 1, 2)
    call(torch_dev, bank, [x], 2, finish=[1])
    worst = [0.0, 0.0]
    check_against_restatement(bank, 0, x, N, True, spectrum_window(omx, N), worst, "isolation")
    swapped = new_bank(omx, 1, 2)
    call(torch_dev, swapped, [x[:, ::-1].copy()], 2, finish=[1])
    assert swapped.fetch_spectrum(0)[1][::-1].tobytes() == bank.fetch_spectrum(0)[1].tobytes(), "a channel's sums depend on its neighbour"
    print(f"channel 120 dB down: worst sum error {worst[0]:.3g} of its own scale, worst dB {worst[1]:.3g}")


# ---------------------------------------------------------------- 2. cuts, on bytes
def cuttings(total, n, n_streams):
    h = n // 2
    sizes = [1, 17, h - 1, h, h + 1, 3 * n + 5]

    def cycle(start, zeros_at=()):
        out, left, i = [], total, start
        while left:
            if len(out) in zeros_at:
                out.append(0)
                continue
            f = min(sizes[i % len(sizes)], left)
            out.append(f)
            left -= f
            i += 1
        return out

    return {"whole": [[total]] * n_streams,
            "every size in turn": [cycle(0)] * n_streams,
            "other cuts per stream, idle calls": [cycle(s + 1, zeros_at=(1, 2 + s, 5)) for s in range(n_streams)],
            "single frames across a transform's end": [[n - 3] + [1] * 6 + [h - 4, 1, 1, 17, total - n - h - 18]] * n_streams,
            "halves": [[total // 2, total - total // 2]] * n_streams}


@pytest.mark.parametrize("n,total,ch", [(N, 7 * H + 333, 2), (N, 7 * H + 333, 3), (8192, 2 * sr.RUN * 4096 + 8192 + 5, 1)])
def test_any_cutting_gives_the_bytes_of_the_whole(torch_dev, omx, n, total, ch):
    n_streams = 3
    xs = [signal(KINDS[s], 50 + s, total, ch, n) for s in range(n_streams)]
    per_group = int(spectrum_plan(omx, SpectrumRule(n), ch)["transforms_per_workgroup"])
    taken = sr.transforms(total, False, n)
    assert taken % sr.RUN and (per_group == 1 or taken % per_group), "the programme ends on a run or a workgroup boundary"
    whole_open = whole_done = None
    idle = 0
    for tag, pieces in cuttings(total, n, n_streams).items():
        bank = new_bank(omx, n_streams, ch, n)
        idle += feed(torch_dev, bank, xs, ch, pieces)
        open_bytes = snapshot(bank, n_streams)
        call(torch_dev, bank, [x[:0] for x in xs], ch, finish=[1] * n_streams)
        done_bytes = snapshot(bank, n_streams)
        if whole_open is None:
            whole_open, whole_done = open_bytes, done_bytes
            rec = bank.fetch_spectrum(0)[0]
            assert int(rec["transforms"][0]) == sr.transforms(total, True, n) and int(rec["finished"]) == 1
            continue
        for s in range(n_streams):
            assert open_bytes[s] == whole_open[s], (tag, s, "not finished: bytes differ from the whole programme's")
            assert done_bytes[s] == whole_done[s], (tag, s, "finished: bytes differ from the whole programme's")
    assert idle > 0, "no call without a completed transform"
    if n == 8192:
        assert taken > 2 * sr.RUN, "no full run"


def test_finish_together_with_the_last_frames_equals_finish_alone(torch_dev, omx):
    total, ch = 7 * H + 333, 2
    xs = [signal("noise", 70, total, ch), signal("sine", 71, total, ch)]
    a, b = new_bank(omx, 2, ch), new_bank(omx, 2, ch)
    call(torch_dev, a, xs, ch, finish=[1, 1])
    call(torch_dev, b, [x[:5 * H + 7] for x in xs], ch)
    call(torch_dev, b, [xs[0][5 * H + 7:], xs[1][5 * H + 7:6 * H]], ch, finish=[1, 0])
    call(torch_dev, b, [xs[0][:0], xs[1][6 * H:]], ch, finish=[1, 1])      # (a finish of a finished stream is no event)
    assert snapshot(a, 2) == snapshot(b, 2)


# ---------------------------------------------------------------- 3. finish, reset
def test_short_and_empty_programmes_finish_and_reset(torch_dev, omx):
    ch = 2
    w = spectrum_window(omx, N)
    xs = [signal("noise", 80, 700, ch), signal("noise", 81, 0, ch), signal("sine", 82, N, ch), signal("dc", 83, H + 1, ch)]
    bank = new_bank(omx, 4, ch)
    assert call(torch_dev, bank, xs, ch)[0] == 1
    worst = [0.0, 0.0]
    for s, x in enumerate(xs):
        check_against_restatement(bank, s, x, N, False, w, worst, "short, open")
    assert call(torch_dev, bank, [x[:0] for x in xs], ch, finish=[1, 1, 1, 1])[0] == 1
    for s, x in enumerate(xs):
        check_against_restatement(bank, s, x, N, True, w, worst, "short, finished")
        assert int(bank.fetch_spectrum(s)[0]["transforms"][0]) == spectrum_transforms(omx, len(x), True, N)
    assert [spectrum_transforms(omx, len(x), True, N) for x in xs] == [1, 0, 2, 2]
    assert call(torch_dev, bank, [x[:0] for x in xs], ch, finish=[1, 1, 1, 1])[0] == 0, "finishing twice is no event"
    before = snapshot(bank, 4)
    with pytest.raises(capi.OmxError, match="finished"):
        call(torch_dev, bank, [xs[0][:0], xs[0][:5], xs[0][:0], xs[0][:0]], ch)
    assert snapshot(bank, 4) == before, "a refused call changed something"
    bank.reset_spectrum([0, 1, 0, 1])
    assert snapshot(bank, 4)[0::2] == before[0::2], "a reset touched a stream it did not flag"
    # streams 1 and 3 start over: the same bytes as the same streams of a new bank
    empty = xs[0][:0]
    call(torch_dev, bank, [empty, xs[0], empty, xs[2]], ch, finish=[0, 1, 0, 1])
    fresh = new_bank(omx, 4, ch)
    call(torch_dev, fresh, [empty, xs[0], empty, xs[2]], ch, finish=[0, 1, 0, 1])
    got, want = snapshot(bank, 4), snapshot(fresh, 4)
    assert got[1] == want[1] and got[3] == want[3], "a stream that was reset differs from a new bank's"
    assert got[0] == before[0] and got[2] == before[2]
    print(f"short programmes: worst sum error {worst[0]:.3g}, worst dB {worst[1]:.3g}")


# ---------------------------------------------------------------- 4. NaN
def test_a_nan_skips_the_transforms_that_cover_it_in_its_channel_only(torch_dev, omx):
    total, ch = 7 * H + 333, 2
    clean = signal("noise", 90, total, ch)
    for value, at in ((np.nan, 3 * H + 5), (np.inf, 0), (-np.inf, 6 * H + 1)):
        dirty = clean.copy()
        dirty[at, 1] = value
        a, b = new_bank(omx, 1, ch), new_bank(omx, 1, ch)
        call(torch_dev, a, [clean], ch, finish=[1])
        feed(torch_dev, b, [dirty], ch, [[2 * H + 9, H, total - 3 * H - 9]], finish=True)
        (rec_a, sums_a), (rec_b, sums_b) = a.fetch_spectrum(0), b.fetch_spectrum(0)
        covering = [k for k in range(sr.transforms(total, True, N)) if k * H <= at < k * H + N]
        assert int(rec_b["skipped"][1]) == len(covering) and int(rec_b["skipped"][0]) == 0, (value, rec_b)
        assert int(rec_b["transforms"][1]) == int(rec_a["transforms"][1]) - len(covering) and int(rec_b["transforms"][0]) == int(rec_a["transforms"][0])
        assert sums_b[0].tobytes() == sums_a[0].tobytes(), "the other channel's bytes changed"
        assert np.isfinite(sums_b).all()
        check_against_restatement(b, 0, dirty, N, True, spectrum_window(omx, N), [0.0, 0.0], ("nan", value))


# ---------------------------------------------------------------- 5. Parseval
def test_density_keeps_parseval(torch_dev, omx):
    total, ch = 18 * H + 5, 3
    x = signal("noise", 95, total, ch)
    x[:, 1] = signal("sine", 96, total, 1)[:, 0]
    bank = new_bank(omx, 1, ch)
    call(torch_dev, bank, [x], ch)
    rec, sums = bank.fetch_spectrum(0)
    want = sr.windowed_mean_square(x, N)
    worst = 0.0
    for c in range(ch):
        got = float(np.sum(spectrum_density(omx, rec, sums, c)))
        worst = max(worst, abs(got - want[c]) / want[c])
    print(f"Parseval: worst relative difference {worst:.3g} (bar {SUM_BAR})")
    assert worst <= SUM_BAR


# ---------------------------------------------------------------- 6. alignment and capacity
def test_every_alignment_of_d_in_and_a_capacity_beyond_the_frames(torch_dev, omx):
    total = 7 * H + 333
    for ch in (1, 3):
        xs = [signal(KINDS[s], 20 + s, total - 100 * s, ch) for s in range(3)]
        seen = []
        for lead in range(4):
            bank = new_bank(omx, 3, ch)
            call(torch_dev, bank, [x[:2 * H + 3] for x in xs], ch, check_input=True, lead=lead, slack=lead * 7 + 1, filler=lead)
            call(torch_dev, bank, [x[2 * H + 3:] for x in xs], ch, finish=[1, 1, 1], check_input=True, lead=(lead + 1) % 4, slack=333, filler=lead + 9)
            seen.append(snapshot(bank, 3))
        assert all(s == seen[0] for s in seen), "the bytes depend on the alignment of d_in or on what lies behind the frames"
        worst = [0.0, 0.0]
        for s, x in enumerate(xs):
            check_against_restatement(bank, s, x, N, True, spectrum_window(omx, N), worst, "alignment")


# ---------------------------------------------------------------- 7. refusals, and a bank that never configures
def test_every_refusal_has_its_own_message_and_changes_nothing(torch_dev, omx):
    torch = torch_dev
    ch = 2
    # The suite holds no allocation counter: free device memory stands in for it.  Two banks of 64 streams are created, one after
    # the other; only the second configures the stage.  What the first costs is what a bank cost before the stage existed, and the
    # second costs that plus the stage's state, so the stage's memory appears at configure and not at create.
    dev = torch.zeros(2 * 64 * ch, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    free_0 = torch.cuda.mem_get_info()[0]
    plain = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), 64, 2, 10)
    free_1 = torch.cuda.mem_get_info()[0]
    big = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), 64, 2, 10)
    free_2 = torch.cuda.mem_get_info()[0]
    state = int(spectrum_plan(omx, SpectrumRule(8192), 8, 64)["state_bytes"])
    assert abs((free_1 - free_2) - (free_0 - free_1)) < state // 4, "free memory (the substitute for an allocation counter): two equal banks cost differently"
    big.configure_spectrum(SpectrumRule(8192), 8)
    free_3 = torch.cuda.mem_get_info()[0]
    assert free_2 - free_3 >= state // 2, "free memory (the substitute for an allocation counter): configure did not allocate the stage's state"
    assert free_0 - free_1 < state // 2, "free memory (the substitute for an allocation counter): a bank that never configures the stage pays for it"
    del plain, big
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=FS), 2, 2, 10)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    messages = []

    def refused(fn, *args, **kw):
        with pytest.raises(capi.OmxError) as e:
            fn(*args, **kw)
        assert e.value.status == capi.ERR_INVALID
        messages.append(str(e.value))

    refused(bank.spectrum, dev.data_ptr(), 64)                        # before configure
    refused(bank.reset_spectrum)
    refused(bank.fetch_spectrum, 0)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before, "free memory (the substitute for an allocation counter): refused calls before configure allocated something"
    for rule in (SpectrumRule(1024), SpectrumRule(16384), SpectrumRule(4096, flags=1)):
        refused(bank.configure_spectrum, rule, ch)
    assert "come next" in messages[-1]
    refused(bank.configure_spectrum, SpectrumRule(N), 0)
    refused(bank.configure_spectrum, SpectrumRule(N), 9)
    refused(bank.spectrum, dev.data_ptr(), 64)                        # still not configured: the refusals above changed nothing
    bank.configure_spectrum(SpectrumRule(N), ch)
    zero = snapshot(bank, 2)
    refused(bank.spectrum, dev.data_ptr(), 64, frames=[65, 0])        # frames[s] > frames_capacity
    refused(bank.spectrum, 0, 64, frames=[0, 3])                      # a null d_in with frames
    refused(bank.spectrum, dev.data_ptr(), 2 ** 32)                   # a capacity beyond 2^32 - 1
    refused(bank.fetch_spectrum, 2)                                   # a stream index out of range
    assert "out of range" in messages[-1] and "not configured" not in messages[-1]
    assert snapshot(bank, 2) == zero
    assert bank.spectrum(0, 0)[0] == 0 and bank.spectrum(0, 64, frames=[0, 0])[0] == 0, "a call without frames needs no d_in"
    assert bank.spectrum(dev.data_ptr(), 64, frames=[64, 0], stream=stream_of(torch))[0] == 1
    held = snapshot(bank, 2)
    refused(bank.configure_spectrum, SpectrumRule(N), ch)             # configure while a stream holds frames
    assert snapshot(bank, 2) == held
    bank.reset_spectrum()
    bank.configure_spectrum(SpectrumRule(4096), 1)
    assert int(bank.fetch_spectrum(1)[0]["fft_size"]) == 4096 and bank.fetch_spectrum(1)[1].shape == (1, 2049)
    distinct = {m for m in messages}
    print("\n".join(sorted(distinct)))
    assert len(distinct) >= 10 and all("program loudness" in m for m in messages), messages


# ---------------------------------------------------------------- 8. match, through the convolve stage
def test_match_fir_through_convolve_meets_the_restatements_residual(torch_dev, omx):
    torch = torch_dev
    n, taps_n, frames = sr.MATCH_N, sr.MATCH_TAPS, sr.MATCH_FRAMES
    ref_residual, ref_taps, _, _ = sr.closed_loop()
    src, tgt = sr.match_inputs()
    bank = new_bank(omx, 2, 1, n)
    call(torch, bank, [src, tgt], 1, finish=[1, 1])
    (rec_s, sums_s), (rec_t, sums_t) = bank.fetch_spectrum(0), bank.fetch_spectrum(1)
    d_src, d_tgt = spectrum_density(omx, rec_s, sums_s, 0), spectrum_density(omx, rec_t, sums_t, 0)
    taps = spectrum_match(omx, d_src, d_tgt, n, FS, SpectrumMatchSpec(), taps_n)
    bank.configure_convolve([taps], 1, delay_frames=(taps_n - 1) // 2)
    d_in = torch.from_numpy(np.stack([src, src])).cuda()
    d_out = torch.zeros((2, frames, 1), dtype=torch.float32).cuda()
    bank.convolve(d_in.data_ptr(), frames, d_out.data_ptr(), frames, flush_mask=[1, 1], stream=stream_of(torch))
    torch.cuda.synchronize()
    assert int(bank.fetch_convolved(0)["frames_written"]) == frames
    bank.reset_spectrum()
    bank.spectrum(d_out.data_ptr(), frames, finish_mask=[1, 1], stream=stream_of(torch))
    rec_o, sums_o = bank.fetch_spectrum(0)
    residual = sr.third_octave_residual(spectrum_density(omx, rec_o, sums_o, 0), d_tgt, n, FS)
    before = sr.third_octave_residual(d_src, d_tgt, n, FS)
    print(f"match on the device: third-octave residual {residual:.4f} dB (before the filter {before:.2f} dB); the restatement alone {ref_residual:.4f} dB; "
          f"taps differ from the restatement's by up to {float(np.abs(taps - ref_taps).max()):.3g}")
    assert residual <= ref_residual + 0.1


# ---------------------------------------------------------------- 9. the C ABI from C99
def test_c99_demo_measures_a_sine_in_two_calls(tmp_path, omx):
    """tests/c_abi/program_spectrum_demo.c checks its own figures and ends with "ok"; the table it prints is read here as well"""
    exe = build_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok", r.stdout
    head = re.search(r"frames (\d+) transforms (\d+) expected (\d+) skipped (\d+) finished (\d+)", r.stdout)
    assert head and [int(v) for v in head.groups()] == [96000, sr.transforms(96000, True, 4096), sr.transforms(96000, True, 4096), 0, 1], r.stdout
    bands = {round(float(c)): float(v) for c, v in re.findall(r"band\s+([0-9.]+) Hz\s+(-?[0-9.]+) dB", r.stdout)}
    x = (0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(96000) / 48000.0)).astype(np.float32).reshape(-1, 1)
    want_c, want_l = sr.bands(sr.measured_density(x, 4096), 4096, FS, 3)
    want = float(want_l[int(np.argmin(np.abs(want_c - 1000.0)))])
    print("demo: 1 kHz band", bands[1000], "dB; the restatement of the same programme", want, "dB")
    # (two decimals are printed; the finished programme's last transforms are partly zeros, hence a little under -6.02 dB)
    assert abs(bands[1000] - want) <= 0.006 and abs(bands[1000] + 6.02) < 0.1 and max(v for c, v in bands.items() if c != 1000) < bands[1000] - 30.0

"""Programme bank channel remix on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_remix / remix / fetch_remixed
against the numpy restatement (tests/program_remix_ref.py, pinned by tests/test_cpu_program_remix.py).

Bars.  Every float of the output equals the restatement's, bit for bit (NaN payloads and the sign of zero included: the comparison is
on bytes); every record field equal except out_sample_peak_db, within 1e-4 dB (the family's bar).  Not written: d_out is filled with a
sentinel float beforehand and every float at or beyond frames[s] * channels_out keeps it; d_in is unchanged.
Shapes.  With t = remix_plan(...).tile_frames the streams are 0, 1, 3, 1001, t - 1, t, t + 1 and 3 t + 5 frames long: the smallest at
which the head, the tail, a tile seam and an unaligned row base can go wrong (a row is (3 t + 5) * channels floats, so at odd channel
counts rows start at 4-byte, not 16-byte, offsets).  No test provokes a fault: the refusals use only arguments the host rejects before
any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_pcm_ref as pr
import program_remix_ref as mr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (REMIX_RECORD_DTYPE, DownmixRule, ExportRule, GainRule, LimitRule, ProgramLoudnessBank, ResampleRule,
                                             remix_downmix, remix_plan, remix_select)
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
PAIRS = [(6, 2), (8, 2), (2, 1), (1, 2), (3, 3), (5, 7), (8, 8), (2, 6)]


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def tile_of(omx, ci, co):
    return int(remix_plan(omx, ci, co)["tile_frames"])


def lengths_of(t):
    return [0, 1, 3, 1001, t - 1, t, t + 1, 3 * t + 5]


def first_difference(got, want):
    g, w = got.reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)
    at = int(np.flatnonzero(g != w)[0])
    return at, got.reshape(-1)[max(at - 2, 0):at + 4], want.reshape(-1)[max(at - 2, 0):at + 4]


def run_call(torch, bank, rows, ci, co, matrix_of_stream=None, filler=999):
    """rows[s]: f32 [frames][ci] of stream s; frames of d_in beyond them hold other samples.  d_out holds the sentinel beforehand.
    Checks that d_in is unchanged and that nothing at or beyond frames[s] was written.  -> (per stream the frames written, the device
    pointer to the records)"""
    n = len(rows)
    counts = [len(r) for r in rows]
    cap = max(max(counts), 1)
    host = mr.noise(filler, n * cap, ci).reshape(n, cap, ci)
    for s, r in enumerate(rows):
        host[s, :len(r)] = r
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n, cap, co), float(SENTINEL), dtype=torch.float32).cuda()
    ptr = bank.remix(d_in.data_ptr(), d_out.data_ptr(), cap, frames=counts, matrix_of_stream=matrix_of_stream, stream=stream_of(torch))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    out = []
    for s, f in enumerate(counts):
        assert (got[s, f:] == SENTINEL).all(), (s, f, "floats at or beyond frames[s] * channels_out were written")
        out.append(got[s, :f].copy())
    return out, ptr


def check_stream(bank, s, got, matrix, x, tag, matrix_index=0):
    want = mr.remix(matrix, x)
    assert got.shape == want.shape, (tag, s, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        raise AssertionError((tag, s, "output differs from the restatement", first_difference(got, want)))
    rec = mr.record(want, matrix, matrix_index, FLOOR)
    mr.check_record(bank.fetch_remixed(s), rec, (tag, s), BAR)
    return rec


# ---------------------------------------------------------------- 1. bits, records, nothing else written
@pytest.mark.parametrize("pair", PAIRS)
def test_output_and_records_equal_the_restatement(torch_dev, omx, pair):
    ci, co = pair
    lengths = lengths_of(tile_of(omx, ci, co))
    n = len(lengths)
    # coefficients up to 3 (some samples go over) with zeros of either sign among them; (1, 2) and (2, 6) get a row without a term
    matrix = np.float32(3.0) * mr.dense(1000 + 10 * ci + co, ci, co)
    bank = new_bank(omx, n)
    bank.configure_remix(matrix, ci, co)
    for s in range(n):      # before the first call: the record of a call that brought nothing
        want = np.array([(0, 0, 0.0, FLOOR, 0, mr.terms(matrix))], REMIX_RECORD_DTYPE)
        assert bank.fetch_remixed(s).tobytes() == want.tobytes()
    xs = [mr.noise(100 * ci + 10 * co + s, f, ci) for s, f in enumerate(lengths)]
    got, ptr = run_call(torch_dev, bank, xs, ci, co)
    over = 0
    for s, x in enumerate(xs):
        over += check_stream(bank, s, got[s], matrix, x, (pair, lengths))["samples_over"]
    assert device_bytes(ptr, n * 32) == b"".join(bank.fetch_remixed(s).tobytes() for s in range(n))
    assert over > 0 or np.abs(matrix).sum(axis=1).max() <= 1.0      # (a row that cannot exceed full scale: (2, 1) with this seed)


# ---------------------------------------------------------------- 2. a matrix per stream
def test_every_stream_uses_its_own_matrix(torch_dev, omx):
    ci, co = 8, 2
    t = tile_of(omx, ci, co)
    lengths = [3 * t, 3 * t - 1, 2 * t + 1, 3 * t, 3 * t - 7]
    fold, _ = remix_downmix(omx, DownmixRule(), ci, capi.positions_fallback(ci))
    pair, missing = remix_select(omx, ci, capi.positions_fallback(ci), co, [mr.POS_SL, mr.POS_SR])
    assert missing == 0
    table = np.stack([fold, pair, mr.dense(5, ci, co), np.zeros((co, ci), np.float32)])
    of_stream = [2, 1, 0, 1, 3]
    bank = new_bank(omx, len(lengths))
    bank.configure_remix(table, ci, co)
    xs = [mr.noise(200 + s, f, ci) for s, f in enumerate(lengths)]
    got, _ = run_call(torch_dev, bank, xs, ci, co, matrix_of_stream=of_stream)
    for s, x in enumerate(xs):
        rec = check_stream(bank, s, got[s], table[of_stream[s]], x, "matrix_of_stream", of_stream[s])
        assert int(bank.fetch_remixed(s)["matrix_index"]) == of_stream[s] and int(bank.fetch_remixed(s)["terms"]) == rec["terms"]
    assert [int(bank.fetch_remixed(s)["terms"]) for s in range(5)] == [mr.terms(table[2]), 2, 8, 2, 0]
    assert got[1].tobytes() == xs[1][:, 6:8].tobytes() and not got[4].any() and not np.signbit(got[4]).any()


# ---------------------------------------------------------------- 3. NaN, infinities, -0.0f
def test_a_permutation_copies_bits_and_a_dropped_channel_stays_out(torch_dev, omx):
    ci = 6
    pos = capi.positions_fallback(ci)
    t = tile_of(omx, ci, ci)
    x = mr.noise(31, t + 9, ci)
    x[2, 0], x[3, 1], x[4, 2], x[5] = np.nan, np.inf, -np.inf, -0.0
    x[t + 1, 5], x[t + 2, 4] = np.nan, -0.0
    film = [mr.POS_FC, mr.POS_FL, mr.POS_FR, mr.POS_RL, mr.POS_RR, mr.POS_LFE]
    m, missing = remix_select(omx, ci, pos, ci, film)
    assert missing == 0
    bank = new_bank(omx, 1)
    bank.configure_remix(m, ci, ci)
    got, _ = run_call(torch_dev, bank, [x], ci, ci)
    assert got[0].tobytes() == x[:, [2, 0, 1, 4, 5, 3]].tobytes()
    check_stream(bank, 0, got[0], m, x, "permutation")
    fold, pos_out = remix_downmix(omx, DownmixRule(), ci, pos)
    y = mr.noise(32, t + 9, ci, 0.25)
    y[7, 3], y[t, 3], y[t + 3, 3] = np.inf, -np.inf, np.nan      # the LFE, level 0
    bank.configure_remix(fold, ci, 2)
    got, _ = run_call(torch_dev, bank, [y], ci, 2)
    assert np.isfinite(got[0]).all()
    check_stream(bank, 0, got[0], fold, y, "dropped LFE")


# ---------------------------------------------------------------- 4. the record's count and peak
def test_a_fold_of_correlated_full_scale_channels_goes_over(torch_dev, omx):
    ci = 6
    t = tile_of(omx, ci, 2)
    fold, _ = remix_downmix(omx, DownmixRule(), ci, capi.positions_fallback(ci))
    safe, _ = remix_downmix(omx, DownmixRule(flags=mr.NORMALIZE), ci, capi.positions_fallback(ci))
    common = mr.noise(41, 2 * t + 3, 1)
    common[t] = 1.0      # every channel at full scale in one frame: the fold's largest value, 1 + c + s
    x = np.repeat(common, ci, axis=1)
    bank = new_bank(omx, 2)
    bank.configure_remix(np.stack([fold, safe]), ci, 2)
    got, _ = run_call(torch_dev, bank, [x, x], ci, 2, matrix_of_stream=[0, 1])
    rec = check_stream(bank, 0, got[0], fold, x, "fold", 0)
    assert rec["samples_over"] > t // 2 and float(rec["out_sample_peak"]) > 2.4
    rec = check_stream(bank, 1, got[1], safe, x, "normalised fold", 1)
    # three weights, each half an ulp from its quotient, and two rounded sums: the full-scale frame lands within one ulp of 1.0
    assert rec["samples_over"] <= 2 and 0.99 < float(rec["out_sample_peak"]) <= 1.0 + 2.0 ** -23


# ---------------------------------------------------------------- 5. cut invariance
def test_output_does_not_depend_on_the_cuts(torch_dev, omx):
    ci, co = 5, 3
    t = tile_of(omx, ci, co)
    matrix = mr.dense(51, ci, co)
    xs = [mr.noise(52, 2 * t + 100, ci), mr.noise(53, t + 50, ci)]
    bank = new_bank(omx, 2)
    bank.configure_remix(matrix, ci, co)
    whole, _ = run_call(torch_dev, bank, xs, ci, co)
    for s, x in enumerate(xs):
        assert whole[s].tobytes() == mr.remix(matrix, x).tobytes()
    at, parts = [0, 0], [[], []]
    for cut in (1, 7, t - 1, 10 ** 9):
        rows = [x[a:a + cut] for x, a in zip(xs, at)]
        got, _ = run_call(torch_dev, bank, rows, ci, co)
        for s in range(2):
            parts[s].append(got[s])
            at[s] += len(rows[s])
    for s in range(2):
        assert np.concatenate(parts[s]).tobytes() == whole[s].tobytes(), s


# ---------------------------------------------------------------- 6. the chain
def records_of(bank):
    return [record_array(bank.fetch(s)).tobytes() for s in range(bank.n_streams)]


def surround_programme(seed, frames, ci=6):
    """a tone under a slow gate in every channel, each at its own level, plus a little noise: every stream completes gating blocks"""
    tt = np.arange(frames)
    tone = 0.2 * np.sin(2 * np.pi * 997.0 * tt / 48000.0) * ((tt // 9000) % 2 + 1) / 2.0
    levels = np.array([1.0, 0.8, 0.6, 1.0, 0.9, 0.7, 0.5, 0.4])[:ci]
    return (tone[:, None] * levels[None] + 0.01 * mr.noise(seed, frames, ci)).astype(np.float32)


def test_remix_then_process_measures_what_the_restated_output_measures(torch_dev, omx):
    ci, n, fs = 6, 2, 48000.0
    pos = capi.positions_fallback(ci)
    fold, pos_out = remix_downmix(omx, DownmixRule(), ci, pos)
    lengths = [96000, 70001]
    xs = [surround_programme(60 + s, f) for s, f in enumerate(lengths)]
    cap = max(lengths)
    host = np.zeros((n, cap, ci), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    bank = new_bank(omx, n)
    bank.configure_remix(fold, ci, 2)
    d_in = torch_dev.from_numpy(host).cuda()
    d_out = torch_dev.full((n, cap, 2), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.remix(d_in.data_ptr(), d_out.data_ptr(), cap, frames=lengths, stream=stream_of(torch_dev))
    restated = np.zeros((n, cap, 2), np.float32)
    for s, x in enumerate(xs):
        restated[s, :len(x)] = mr.remix(fold, x)
    via, direct, surround = new_bank(omx, n), new_bank(omx, n), new_bank(omx, n, ci)
    for b in (via, direct, surround):
        b.set_peaks(True)
    via.process(d_out.data_ptr(), cap, 2, fs, pos_out, frames=lengths, stream=stream_of(torch_dev))
    d_host = torch_dev.from_numpy(restated).cuda()
    direct.process(d_host.data_ptr(), cap, 2, fs, pos_out, frames=lengths, stream=stream_of(torch_dev))
    surround.process(d_in.data_ptr(), cap, ci, fs, pos, frames=lengths, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    got = d_out.cpu().numpy()
    for s, f in enumerate(lengths):
        assert got[s, :f].tobytes() == restated[s, :f].tobytes(), s
    assert records_of(via) == records_of(direct)
    assert [via.fetch_peaks(s).tobytes() for s in range(n)] == [direct.fetch_peaks(s).tobytes() for s in range(n)]
    for s in range(n):
        assert via.fetch_segments(s).tobytes() == direct.fetch_segments(s).tobytes(), s
        a, b = via.fetch(s).integrated_lufs, surround.fetch(s).integrated_lufs
        print(f"stream {s}: {a:.3f} LUFS as Lo/Ro, {b:.3f} LUFS as 5.1")
        assert np.isfinite(a) and a > -40.0 and np.isfinite(b) and abs(a - b) > 0.1      # the layout matters to the figure


# ---------------------------------------------------------------- 7. the records of the earlier headers
def test_remix_leaves_the_records_of_the_earlier_headers_alone(torch_dev, omx):
    ch, n, frames = 2, 3, 22051
    pos = capi.positions_fallback(ch)
    bank = new_bank(omx, n)
    x = np.stack([surround_programme(70 + s, frames, ch) for s in range(n)])
    d_some = torch_dev.from_numpy(x).cuda()
    bank.set_peaks(True)
    bank.process(d_some.data_ptr(), frames, ch, 44100.0, pos, stream=stream_of(torch_dev))
    ptr = bank.plan_gains(GainRule(-20.0, -1.0, -60.0, 60.0, 0), stream=stream_of(torch_dev))
    d_tmp = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.apply_gains(d_some.data_ptr(), d_tmp.data_ptr(), frames, ch, ptr, n, stream=stream_of(torch_dev))
    bank.configure_limiter(LimitRule(-1.0, 64, 0), ch, 44100.0)
    bank.apply_limited(d_some.data_ptr(), frames, d_tmp.data_ptr(), frames, ptr, n, flush_mask=[1] * n, stream=stream_of(torch_dev))
    bank.configure_export(ExportRule(pr.S16, pr.TPDF, 3), ch)
    d_pcm = torch_dev.zeros((n * frames * ch * 2,), dtype=torch_dev.uint8).cuda()
    bank.export_pcm(d_tmp.data_ptr(), d_pcm.data_ptr(), frames, stream=stream_of(torch_dev))
    bank.configure_resampler(ResampleRule(44100, 48000), ch)
    d_48k = torch_dev.zeros((n, 24002, ch), dtype=torch_dev.float32).cuda()
    bank.resample(d_some.data_ptr(), frames, d_48k.data_ptr(), 24002, flush_mask=[1] * n, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()

    def state():
        return (records_of(bank), [bank.fetch_peaks(s).tobytes() for s in range(n)], bank.fetch_gains().tobytes(),
                [bank.fetch_applied(s).tobytes() for s in range(n)], [bank.fetch_limited(s).tobytes() for s in range(n)],
                [bank.fetch_exported(s).tobytes() for s in range(n)], [bank.fetch_resampled(s).tobytes() for s in range(n)],
                [bank.fetch_segments(s).tobytes() for s in range(n)])

    before = state()
    assert int(bank.fetch_resampled(0)["frames_out"]) == 24002 and int(bank.fetch_exported(0)["frames_out"]) == frames
    mono, _ = remix_downmix(omx, DownmixRule(kind=mr.KIND_MONO), ch, pos)
    bank.configure_remix(mono, ch, 1)
    got, _ = run_call(torch_dev, bank, [x[s] for s in range(n)], ch, 1)
    for s in range(n):
        check_stream(bank, s, got[s], mono, x[s], "mono fold")
    assert state() == before, "a call of program_remix.h changed a record of an earlier header"


# ---------------------------------------------------------------- 8. a second table
def test_a_second_configure_replaces_the_table(torch_dev, omx):
    bank = new_bank(omx, 2)
    first, second = mr.dense(81, 6, 2), mr.dense(82, 3, 5)
    bank.configure_remix(first, 6, 2)
    xs = [mr.noise(83, 700, 6), mr.noise(84, 9, 6)]
    got, _ = run_call(torch_dev, bank, xs, 6, 2)
    for s in range(2):
        check_stream(bank, s, got[s], first, xs[s], "first table")
    bank.configure_remix(np.stack([second, mr.dense(85, 3, 5)]), 3, 5)
    assert int(bank.fetch_remixed(0)["frames"]) == 0 and int(bank.fetch_remixed(0)["terms"]) == mr.terms(second)
    ys = [mr.noise(86, 1200, 3), mr.noise(87, 33, 3)]
    got, _ = run_call(torch_dev, bank, ys, 3, 5, matrix_of_stream=[0, 1])
    check_stream(bank, 0, got[0], second, ys[0], "second table", 0)
    check_stream(bank, 1, got[1], mr.dense(85, 3, 5), ys[1], "second table", 1)


# ---------------------------------------------------------------- 9. refusals
def test_refused_calls_change_nothing(torch_dev, omx):
    ci, co, n, cap = 6, 2, 3, 400
    x = np.stack([mr.noise(90 + s, cap, ci, 0.8) for s in range(n)])
    in_bytes, out_bytes = x.size * 4, n * cap * co * 4
    store = torch_dev.full(((in_bytes + out_bytes) // 4 + 16,), float(SENTINEL), dtype=torch_dev.float32).cuda()
    store[:x.size] = torch_dev.from_numpy(x.reshape(-1)).cuda()
    d_in, d_out = store.data_ptr(), store.data_ptr() + in_bytes
    bank = new_bank(omx, n)
    good = dict(d_in=d_in, d_out=d_out, frames_capacity=cap, frames=[300, 0, 150])
    for call in (lambda: bank.remix(**good), lambda: bank.fetch_remixed(0)):      # before configure
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID
    fold = mr.downmix(ci, capi.positions_fallback(ci))[0]
    configure = omx.fn("program_loudness_bank_remix_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32])

    def bad_configures(tag):
        for a, b in ((0, 2), (9, 2), (6, 0), (6, 9)):
            assert configure(bank._h, a, b, fold.ctypes.data, 1) == capi.ERR_INVALID, (tag, a, b)
        assert configure(bank._h, ci, co, None, 1) == capi.ERR_INVALID, tag                       # a null table
        assert configure(bank._h, ci, co, fold.ctypes.data, 0) == capi.ERR_INVALID, tag
        assert configure(bank._h, ci, co, fold.ctypes.data, mr.MAX_MATRICES + 1) == capi.ERR_INVALID, tag
        for v in (np.nan, np.inf, -np.inf):
            m = fold.copy()
            m[1, 5] = v
            with pytest.raises(capi.OmxError) as err:
                bank.configure_remix(m, ci, co)
            assert err.value.status == capi.ERR_INVALID, (tag, v)

    bad_configures("new bank")
    with pytest.raises(capi.OmxError):
        bank.fetch_remixed(0)                                           # a refused configure configured nothing
    bank.configure_remix(np.stack([fold, fold]), ci, co)
    ptr = bank.remix(**good, matrix_of_stream=[0, 1, 1])
    torch_dev.cuda.synchronize()
    everything, records = store.cpu().numpy().tobytes(), device_bytes(ptr, n * 32)
    assert [int(bank.fetch_remixed(s)["frames"]) for s in range(n)] == [300, 0, 150]
    assert [int(bank.fetch_remixed(s)["matrix_index"]) for s in range(n)] == [0, 1, 1]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert store.cpu().numpy().tobytes() == everything, tag
        assert device_bytes(ptr, n * 32) == records, tag

    bad_configures("configured bank")
    unchanged("refused configures")
    bad_calls = {"d_out inside d_in": dict(d_out=d_in + 4), "d_out one float below the end of d_in": dict(d_out=d_in + in_bytes - 4),
                 "d_in inside d_out": dict(d_in=d_out + 8), "the same buffer": dict(d_out=d_in),
                 "d_in one float below the end of d_out": dict(d_in=d_out + out_bytes - 4),
                 "frames[s] > frames_capacity": dict(frames=[cap + 1, 0, 0]),
                 "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                 "matrix index out of range": dict(matrix_of_stream=[0, 2, 0]),
                 "matrix index far out of range": dict(matrix_of_stream=[2 ** 32 - 1, 0, 0]),
                 "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.remix(**{**good, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    raw_fn = omx.fn("program_loudness_bank_remix", C.c_int,
                    [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    counts = np.array([1, 1, 1], np.uint32)
    assert raw_fn(bank._h, C.c_void_p(d_in), cap, counts.ctypes.data, C.c_void_p(d_out), None, None, None) == capi.ERR_INVALID      # null d_remixed
    unchanged("null d_remixed")
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_remixed(n)
    assert err.value.status == capi.ERR_INVALID
    fetch = omx.fn("program_loudness_bank_fetch_remixed", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])
    assert fetch(bank._h, 0, None) == capi.ERR_INVALID
    unchanged("refused fetches")
    # null buffers are accepted where no stream brings a frame
    assert bank.remix(d_in=0, d_out=0, frames_capacity=cap, frames=[0, 0, 0]) != 0
    assert [int(bank.fetch_remixed(s)["frames"]) for s in range(n)] == [0, 0, 0]
    # and the bank goes on as if nothing had been refused
    got, _ = run_call(torch_dev, bank, [x[0, :77], x[1], x[2, :0]], ci, co)
    for s, f in enumerate((77, cap, 0)):
        check_stream(bank, s, got[s], fold, x[s, :f], "after the refusals")


# ---------------------------------------------------------------- 10. the C99 host
def demo_programme():
    """tests/c_abi/program_remix_demo.c's programme: (the packed S24 bytes, the integer samples [frames][6])"""
    frames, ci = 96000, 6
    state, v = 12345, np.zeros(frames * ci, np.int64)
    for i in range(v.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        v[i] = ((state >> 10) & 0x3FFFFF) - 2097152
    v = v.reshape(frames, ci)
    loud = (np.arange(frames) % 24000 < 2400)[:, None] & (np.arange(ci) != 3)[None]
    v = np.where(loud, 3 * v, v)
    v[:, 3] *= 4
    u = (v.reshape(-1) & 0xFFFFFF).astype(np.uint32)
    raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).reshape(-1)
    return raw, v


def test_c99_demo_prints_the_python_routes_records(torch_dev, omx, tmp_path):
    """tests/c_abi/program_remix_demo.c: import S24 5.1 at 48 kHz, the fold-down to Lo/Ro, process, plan_gains, apply_limited and the
    export as S16 stereo from a plain C host"""
    from test_cpu_program_remix import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    printed = {tok[i]: tok[i + 1] for i in range(0, len(tok), 2)}
    ci, co, frames, fs = 6, 2, 96000, 48000.0
    raw, samples = demo_programme()
    fold, pos_out = remix_downmix(omx, DownmixRule(), ci, capi.positions_fallback(ci))
    bank = new_bank(omx, 1, co, fs)
    d_pcm = torch_dev.from_numpy(raw).cuda()
    d_f32 = torch_dev.zeros((frames, ci), dtype=torch_dev.float32).cuda()
    d_lo_ro, d_lim = (torch_dev.zeros((1, frames, co), dtype=torch_dev.float32).cuda() for _ in range(2))
    d_out = torch_dev.zeros((frames * co * 2,), dtype=torch_dev.uint8).cuda()
    bank.import_pcm(d_pcm.data_ptr(), pr.S24, d_f32.data_ptr(), frames, ci)
    bank.configure_remix(fold, ci, co)
    bank.remix(d_f32.data_ptr(), d_lo_ro.data_ptr(), frames)
    bank.process(d_lo_ro.data_ptr(), frames, co, fs, pos_out)
    ptr = bank.plan_gains(GainRule(-16.0, -1.0, -60.0, 60.0, 0))
    bank.configure_limiter(LimitRule(-1.0, 64, 0), co, fs)
    bank.apply_limited(d_lo_ro.data_ptr(), frames, d_lim.data_ptr(), frames, ptr, 1, flush_mask=[1])
    bank.configure_export(ExportRule(pr.S16, pr.TPDF, 2025), co)
    bank.export_pcm(d_lim.data_ptr(), d_out.data_ptr(), frames)
    torch_dev.cuda.synchronize()
    m, rec, g, lim, e = bank.fetch_remixed(0), bank.fetch(0), bank.fetch_gains()[0], bank.fetch_limited(0), bank.fetch_exported(0)
    checksum = 1469598103934665603
    for byte in d_out.cpu().numpy().tobytes():
        checksum = ((checksum ^ byte) * 1099511628211) & (2 ** 64 - 1)
    want = {"tile": str(tile_of(omx, ci, co)), "channels_in": "6", "channels_out": "2", "remixed_frames": str(int(m["frames"])),
            "remixed_over": str(int(m["samples_over"])), "remixed_peak": f"{float(m['out_sample_peak']):.6f}", "matrix": "0", "terms": "6",
            "integrated_lufs": f"{float(rec.integrated_lufs):.4f}", "gain_db": f"{float(g['gain_db']):.4f}",
            "frames_limited": str(int(lim["frames_limited"])), "min_envelope": f"{float(lim['min_envelope']):.6f}",
            "frames_out": str(int(e["frames_out"])), "samples_clipped": str(int(e["samples_clipped"])), "out_peak": str(int(e["out_peak"])),
            "format": "1", "checksum": str(checksum)}
    assert printed == want, (printed, want)
    # the device's Lo/Ro programme is the restatement's, and the LFE at full scale did not reach it
    x = (samples.astype(np.float64) / 2.0 ** 23).astype(np.float32)
    assert d_f32.cpu().numpy().tobytes() == x.tobytes()
    want_lo_ro = mr.remix(fold, x)
    assert d_lo_ro.cpu().numpy()[0].tobytes() == want_lo_ro.tobytes()
    mr.check_record(m, mr.record(want_lo_ro, fold, 0, FLOOR), "demo", BAR)
    assert int(m["frames"]) == frames and float(np.abs(x[:, 3]).max()) > 0.99 and float(m["out_sample_peak"]) < 2.0

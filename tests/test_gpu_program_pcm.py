"""Programme bank PCM formats on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.import_pcm / configure_export / export_pcm /
fetch_exported against the numpy restatement (tests/program_pcm_ref.py, pinned by tests/test_cpu_program_pcm.py).

Bars.  Every float of an import and every byte of an export equal the restatement's; every record field equal except out_peak_db,
within 1e-4 dB (the family's bar).  Not written: the integer buffer is filled with the byte 0xA5 and the f32 buffer with a sentinel
float beforehand, and every byte and float beyond frames[s] keeps it, the bytes that share a dword with a row's last sample or its
neighbour's first included (rows of 1001 frames start off a dword boundary in S16 and S24).  Cut invariance: the concatenated bytes
of any schedule of calls are those of the one-call export.  Round trip: integrated loudness within 1e-4 LU.
pr.TILE_SAMPLES is kPcTileSamples; pr.tile_frames puts a stream length one frame beside a tile's end.
No test provokes a fault: the refusals use only arguments the host rejects before any launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import program_limit_ref as lr
import program_loudness_ref as ref
import program_pcm_ref as pr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import EXPORT_RECORD_DTYPE, ExportRule, GainRule, LimitRule, ProgramLoudnessBank
from parity import bar
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL_FLOAT = np.float32(777.25)
SENTINEL_BYTE = 0xA5
FORMATS = (pr.S16, pr.S24, pr.S32)
CHANNELS = (1, 2, 3, 8)
SLACK = 16      # sentinel bytes behind the last row


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def shapes(ch):
    """(frames_capacity, frames per stream): 0, 1 and 1001 frames in rows of 1001 (a row of no frames behind a full one and in front of
    one), one frame either side of a tile's end; 5 streams x 3 tiles"""
    t = pr.tile_frames(ch)
    out = [(1001, [0, 1, 1001]), (1001, [1001, 0, 1]), (t[-1] + 1, [t[0], t[2], t[1]]), (t[-1] + 1, [t[3], 0, t[-1] + 1])]
    if ch == 8:
        out.append((1541, [1541, 1025, 1536, 0, 1537]))
    return out


def first_difference(got, want):
    at = int(np.flatnonzero(got != want)[0])
    return at, got[max(at - 4, 0):at + 8], want[max(at - 4, 0):at + 8]


def run_import(torch, bank, raws, counts, cap, ch, fmt):
    """raws[s]: the bytes of row s (cap frames).  -> f32 [n][cap][ch] as the device left it, sentinel where nothing was written"""
    n, B = len(counts), pr.BYTES[fmt]
    blob = np.frombuffer(b"".join(raws), np.uint8).copy()
    assert blob.size == n * cap * ch * B
    d_in = torch.from_numpy(np.concatenate([blob, np.zeros(SLACK, np.uint8)])).cuda()
    d_out = torch.full((n, cap, ch), float(SENTINEL_FLOAT), dtype=torch.float32).cuda()
    rc = bank.import_pcm(d_in.data_ptr(), fmt, d_out.data_ptr(), cap, ch, frames=counts, stream=stream_of(torch))
    torch.cuda.synchronize()
    assert rc == (1 if any(counts) else 0)
    assert d_in.cpu().numpy()[:blob.size].tobytes() == blob.tobytes(), "d_in changed"
    return d_out.cpu().numpy()


def run_export(torch, bank, rows, cap, ch, fmt, filler=999):
    """rows[s]: f32 [frames][ch] of stream s in this call.  Frames of d_in beyond them hold other samples.  Checks that nothing beyond a
    stream's frames was written.  -> (per stream the bytes written, the device pointer to the records)"""
    n, B = len(rows), pr.BYTES[fmt]
    counts = [len(r) for r in rows]
    host = pr.noise(filler, n * cap, ch).reshape(n, cap, ch)
    for s, r in enumerate(rows):
        host[s, :len(r)] = r
    d_in = torch.from_numpy(host).cuda()
    row_bytes = cap * ch * B
    d_out = torch.full((n * row_bytes + SLACK,), SENTINEL_BYTE, dtype=torch.uint8).cuda()
    ptr = bank.export_pcm(d_in.data_ptr(), d_out.data_ptr(), cap, frames=counts, stream=stream_of(torch))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    out = []
    for s, f in enumerate(counts):
        lo, hi = s * row_bytes + f * ch * B, (s + 1) * row_bytes
        assert (got[lo:hi] == SENTINEL_BYTE).all(), (s, f, "bytes beyond frames[s] were written", lo + int(np.flatnonzero(got[lo:hi] != SENTINEL_BYTE)[0]))
        out.append(got[s * row_bytes:lo].tobytes())
    assert (got[n * row_bytes:] == SENTINEL_BYTE).all()
    return out, ptr


def fit(schedule, xs):
    """the calls of `schedule` clipped to what every stream has left, and one more call with the rest"""
    left, out = [len(x) for x in xs], []
    for counts in schedule:
        row = [min(int(c), l) for c, l in zip(counts, left)]
        left = [l - r for l, r in zip(left, row)]
        out.append(row)
    return out + ([left] if any(left) else [])


def export_in_calls(torch, bank, xs, ch, fmt, schedule):
    taken, parts = [0] * len(xs), [[] for _ in xs]
    for counts in schedule:
        rows = [xs[s][taken[s]:taken[s] + f] for s, f in enumerate(counts)]
        got, _ = run_export(torch, bank, rows, max(max(counts), 1), ch, fmt)
        for s, f in enumerate(counts):
            parts[s].append(got[s])
            taken[s] += f
            rec = bank.fetch_exported(s)
            assert (int(rec["frames_written"]), int(rec["frames_out"])) == (f, taken[s]), (s, counts)
    assert all(taken[s] == len(x) for s, x in enumerate(xs))
    return [b"".join(p) for p in parts]


# ---------------------------------------------------------------- 1. import
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_import_equals_the_restatement(torch_dev, omx, fmt, ch):
    for cap, counts in shapes(ch):
        bank = new_bank(omx, len(counts), ch)
        raws = [pr.random_pcm(10 * cap + s, cap, ch, fmt) for s in range(len(counts))]
        got = run_import(torch_dev, bank, raws, counts, cap, ch, fmt)
        for s, f in enumerate(counts):
            want = pr.import_pcm(raws[s][:f * ch * pr.BYTES[fmt]], fmt, ch)
            assert got[s, :f].tobytes() == want.tobytes(), (fmt, ch, cap, counts, s, first_difference(got[s, :f].reshape(-1), want.reshape(-1)))
            assert (got[s, f:] == SENTINEL_FLOAT).all(), (fmt, ch, cap, counts, s, "frames at or above frames[s] were written")


# ---------------------------------------------------------------- 2. export
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("dither", (pr.NONE, pr.TPDF))
@pytest.mark.parametrize("fmt", FORMATS)
def test_export_bytes_and_records_equal_the_restatement(torch_dev, omx, fmt, dither, ch):
    """noise at +-1.2 full scale, a sine of 0.4 LSB, a stream with NaN, infinities, denormals, +-1.0 and exact halves, zeros"""
    rule = (fmt, dither, 0xC0FFEE + ch)
    clipped = nans = 0
    for k, (cap, counts) in enumerate(shapes(ch)):
        n = len(counts)
        bank = new_bank(omx, n, ch)
        bank.configure_export(ExportRule(*rule), ch)
        for s in range(n):
            idle = bank.fetch_exported(s)
            assert idle.tobytes() == np.array([(0, 0, 0, 0, 0, FLOOR, fmt, dither)], EXPORT_RECORD_DTYPE).tobytes(), idle
        xs = pr.export_case_streams(100 * ch + k, counts, ch, fmt, first_kind=k)
        got, ptr = run_export(torch_dev, bank, xs, cap, ch, fmt)
        for s, x in enumerate(xs):
            ex = pr.Exporter(rule, s, FLOOR)
            want = ex.feed(x)
            assert len(got[s]) == len(want)
            if got[s] != want:
                g, w = np.frombuffer(got[s], np.uint8), np.frombuffer(want, np.uint8)
                raise AssertionError((fmt, dither, ch, cap, counts, s, "bytes differ from the restatement", first_difference(g, w)))
            rec = bank.fetch_exported(s)
            pr.check_record(rec, ex.record(), (fmt, dither, ch, cap, counts, s))
            clipped, nans = clipped + int(rec["samples_clipped"]), nans + int(rec["samples_nan"])
        assert device_bytes(ptr, n * 48) == b"".join(bank.fetch_exported(s).tobytes() for s in range(n))
    assert clipped > 0 and nans > 0, (clipped, nans)


# ---------------------------------------------------------------- 3. cut invariance
@pytest.mark.parametrize("fmt,ch", [(pr.S16, 2), (pr.S24, 3), (pr.S24, 1), (pr.S32, 8), (pr.S16, 3)])
def test_bytes_do_not_depend_on_the_cuts(torch_dev, omx, fmt, ch):
    rule = (fmt, pr.TPDF, 31337)
    t = pr.tile_frames(ch)
    lengths = [2 * t[1] + 77, t[1] + 500, 1001]
    xs = [pr.hard(300 + s, f, ch, fmt) if s != 1 else pr.noise(300 + s, f, ch) for s, f in enumerate(lengths)]
    n = len(xs)
    bank = new_bank(omx, n, ch)
    bank.configure_export(ExportRule(*rule), ch)
    whole = export_in_calls(torch_dev, bank, xs, ch, fmt, [lengths])
    records = [bank.fetch_exported(s) for s in range(n)]
    for s, x in enumerate(xs):
        ex = pr.Exporter(rule, s, FLOOR)
        assert whole[s] == ex.feed(x), s
        pr.check_record(records[s], ex.record(), s)
    small = [[0] * n, [1] * n, [7] * n, [t[0]] * n, [t[2]] * n]
    rng = np.random.default_rng(5)
    ragged = [[int(rng.integers(0, 900)) if rng.random() < 0.7 else 0 for _ in range(n)] for _ in range(6)] + [[1, 0, 3], [0, 2, 0]]
    for name, schedule in (("0, 1, 7 and tile -+ 1 frames", small), ("ragged", ragged)):
        bank.reset_export()
        assert all(int(bank.fetch_exported(s)["frames_out"]) == 0 for s in range(n))
        parts = export_in_calls(torch_dev, bank, xs, ch, fmt, fit(schedule, xs))
        for s in range(n):
            assert parts[s] == whole[s], (fmt, ch, name, s)
            got = bank.fetch_exported(s)
            for f in pr.RECORD_FIELDS:
                if f != "frames_written":
                    assert got[f].tobytes() == records[s][f].tobytes(), (name, s, f, got[f], records[s][f])


# ---------------------------------------------------------------- 4. dither keys
def test_dither_keys(torch_dev, omx):
    fmt, ch, n, frames = pr.S16, 2, 3, 700
    x = pr.noise(40, frames, ch, 0.7)
    xs = [x, x, x]
    bank = new_bank(omx, n, ch)
    bank.configure_export(ExportRule(fmt, pr.NONE, 1), ch)
    plain = export_in_calls(torch_dev, bank, xs, ch, fmt, [[frames] * n])
    assert plain[0] == plain[1] == plain[2]
    bank.reset_export()
    bank.configure_export(ExportRule(fmt, pr.TPDF, 1), ch)
    first = export_in_calls(torch_dev, bank, xs, ch, fmt, [[frames] * n])
    assert len({first[0], first[1], first[2]}) == 3 and plain[0] not in first
    for s in range(n):
        assert first[s] == pr.export_pcm(x, (fmt, pr.TPDF, 1), s, 0)[0], s
    # a second pass continues at frame 700; a reset of stream 1 alone restarts that stream at frame 0
    bank.reset_export([0, 1, 0])
    assert [int(bank.fetch_exported(s)["frames_out"]) for s in range(n)] == [frames, 0, frames]
    assert bank.fetch_exported(0)["out_peak"] > 0 and bank.fetch_exported(1)["out_peak"] == 0
    got, _ = run_export(torch_dev, bank, xs, frames, ch, fmt)
    assert got[1] == first[1] and got[0] != first[0] and got[2] != first[2]
    assert got[0] == pr.export_pcm(x, (fmt, pr.TPDF, 1), 0, frames)[0] and got[2] == pr.export_pcm(x, (fmt, pr.TPDF, 1), 2, frames)[0]
    assert [int(bank.fetch_exported(s)["frames_out"]) for s in range(n)] == [2 * frames, frames, 2 * frames]
    # the same seed gives the same bytes in another bank; another seed does not
    for seed, same in ((1, True), (2, False)):
        other = new_bank(omx, n, ch)
        other.configure_export(ExportRule(fmt, pr.TPDF, seed), ch)
        again = export_in_calls(torch_dev, other, xs, ch, fmt, [[frames] * n])
        assert (again == first) == same and (again[0] == first[0]) == same, seed


# ---------------------------------------------------------------- 5. round trips and the measurement state
def records_of(bank):
    return [record_array(bank.fetch(s)).tobytes() for s in range(bank.n_streams)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_import_then_process_measures_what_the_host_converted_f32_measures(torch_dev, omx, fmt):
    fs, ch, n, cap = 8000.0, 2, 3, 30000      # 3.75 s, 1.5 s and 3 s: every stream completes gating blocks
    pos = capi.positions_fallback(ch)
    counts = [30000, 12345, 24001]
    B = pr.BYTES[fmt]
    raws = []
    for s in range(n):      # programmes at a moderate level: noise of 14 bits under a slow gate, in the format's top bits
        v = (np.random.default_rng(60 + s).integers(-8000, 8000, (cap, ch)) * ((np.arange(cap) // 6000) % 2 + 1)[:, None]).astype(np.int64)
        raws.append(pr.pack(v.reshape(-1) << (pr.BITS[fmt] - 16), fmt))
    direct, via = new_bank(omx, n, ch, fs), new_bank(omx, n, ch, fs)
    direct.set_peaks(True)
    via.set_peaks(True)
    host = np.zeros((n, cap, ch), np.float32)
    for s, f in enumerate(counts):
        host[s, :f] = pr.import_pcm(raws[s][:f * ch * B], fmt, ch)
    d_host = torch_dev.from_numpy(host).cuda()
    direct.process(d_host.data_ptr(), cap, ch, fs, pos, frames=counts, stream=stream_of(torch_dev))
    d_in = torch_dev.from_numpy(np.frombuffer(b"".join(raws), np.uint8).copy()).cuda()
    d_f32 = torch_dev.full((n, cap, ch), float(SENTINEL_FLOAT), dtype=torch_dev.float32).cuda()
    via.import_pcm(d_in.data_ptr(), fmt, d_f32.data_ptr(), cap, ch, frames=counts, stream=stream_of(torch_dev))
    via.process(d_f32.data_ptr(), cap, ch, fs, pos, frames=counts, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert records_of(via) == records_of(direct)
    assert [via.fetch_peaks(s).tobytes() for s in range(n)] == [direct.fetch_peaks(s).tobytes() for s in range(n)]
    assert all(np.isfinite(direct.fetch(s).integrated_lufs) and direct.fetch(s).integrated_lufs > -40.0 for s in range(n))


def test_limited_output_survives_24_bits_and_no_measurement_changes(torch_dev, omx, oracle):
    """plan to -14 LUFS, apply_limited, export as S24 with TPDF, import, measure with a second bank: the integrated loudness is within
    1e-4 LU of the f32 output's.  The CPU restatement of both says so first (the dither of a 24-bit export lies 138 dB under full
    scale, the programme's tone at -30 dBFS).  Every record of the earlier headers has the same bytes before and after the new calls"""
    fs, ch, rule = lr.ROUND_TRIP_RATE, 2, lr.ROUND_TRIP_RULE
    pos = capi.positions_fallback(2)
    xs = lr.round_trip_programmes()
    n, frames = len(xs), lr.ROUND_TRIP_FRAMES
    d = torch_dev.from_numpy(np.stack(xs)).cuda()
    bank = new_bank(omx, n, ch, fs)
    bank.set_peaks(True)
    bank.process(d.data_ptr(), frames, ch, fs, pos, stream=stream_of(torch_dev))
    ptr = bank.plan_gains(GainRule(lr.ROUND_TRIP_TARGET, lr.CEILING_DB, -60.0, 60.0, 0), stream=stream_of(torch_dev))
    bank.configure_limiter(LimitRule(*rule), ch, fs)
    d_lim = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.apply_limited(d.data_ptr(), frames, d_lim.data_ptr(), frames, ptr, n, flush_mask=[1] * n, stream=stream_of(torch_dev))
    d_plain = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.apply_gains(d.data_ptr(), d_plain.data_ptr(), frames, ch, ptr, n, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    limited = d_lim.cpu().numpy()

    def state():
        return (records_of(bank), [bank.fetch_peaks(s).tobytes() for s in range(n)], bank.fetch_gains().tobytes(),
                [bank.fetch_applied(s).tobytes() for s in range(n)], [bank.fetch_limited(s).tobytes() for s in range(n)])

    before = state()
    export_rule = (pr.S24, pr.TPDF, 7)
    kw = oracle.k_weighting_coefficients(ref.sanitize_rate(fs))
    cpu_f32 = ref.restate(limited[0], fs, pos, kw, FLOOR)
    cpu_s24 = ref.restate(pr.import_pcm(pr.export_pcm(limited[0], export_rule, 0, 0)[0], pr.S24, ch), fs, pos, kw, FLOOR)
    cpu_diff = abs(float(cpu_s24["integrated_lufs"]) - float(cpu_f32["integrated_lufs"]))
    print(f"restated: f32 {float(cpu_f32['integrated_lufs']):.6f} LUFS, through 24 bits {float(cpu_s24['integrated_lufs']):.6f} ({cpu_diff:.2e} LU)")
    assert cpu_diff <= BAR / 10 and cpu_f32["gate_margin"] >= ref.GATE_MARGIN_MIN

    bank.configure_export(ExportRule(*export_rule), ch)
    d_pcm = torch_dev.full((n * frames * ch * 3 + SLACK,), SENTINEL_BYTE, dtype=torch_dev.uint8).cuda()
    bank.export_pcm(d_lim.data_ptr(), d_pcm.data_ptr(), frames, stream=stream_of(torch_dev))
    d_back = torch_dev.zeros((n, frames, ch), dtype=torch_dev.float32).cuda()
    bank.import_pcm(d_pcm.data_ptr(), pr.S24, d_back.data_ptr(), frames, ch, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    raw = d_pcm.cpu().numpy()
    for s in range(n):
        want, _ = pr.export_pcm(limited[s], export_rule, s, 0)
        assert raw[s * len(want):(s + 1) * len(want)].tobytes() == want, s
        assert d_back.cpu().numpy()[s].tobytes() == pr.import_pcm(want, pr.S24, ch).tobytes(), s
    bank.reset_export([1, 0, 1])
    assert state() == before, "a call of program_pcm.h changed a record of an earlier header"
    first, second = new_bank(omx, n, ch, fs), new_bank(omx, n, ch, fs)
    first.process(d_lim.data_ptr(), frames, ch, fs, pos, stream=stream_of(torch_dev))
    second.process(d_back.data_ptr(), frames, ch, fs, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    a, b = first.fetch(0), second.fetch(0)
    print(f"measured: f32 {float(a.integrated_lufs):.6f} LUFS, through 24 bits {float(b.integrated_lufs):.6f}")
    bar("program pcm: |integrated through S24 - integrated of the f32| LU", abs(float(b.integrated_lufs) - float(a.integrated_lufs)), BAR, 0)


# ---------------------------------------------------------------- 6. refusals
def test_refused_calls_change_nothing(torch_dev, omx):
    fmt, ch, n, cap = pr.S24, 2, 3, 200
    B = pr.BYTES[fmt]
    x = np.stack([pr.noise(70 + s, cap, ch, 0.8) for s in range(n)])
    f32_bytes, int_bytes = x.size * 4, x.size * B
    store = torch_dev.full((f32_bytes + int_bytes + 64,), SENTINEL_BYTE, dtype=torch_dev.uint8).cuda()
    store[:f32_bytes] = torch_dev.from_numpy(x.reshape(-1).view(np.uint8).copy()).cuda()
    d_f32, d_int = store.data_ptr(), store.data_ptr() + f32_bytes
    assert d_int % 4 == 0
    bank = new_bank(omx, n, ch)
    rule = (fmt, pr.TPDF, 5)
    good = dict(d_in=d_f32, d_out=d_int, frames_capacity=cap, frames=[100, 0, 50])
    for call in (lambda: bank.export_pcm(**good), lambda: bank.fetch_exported(0), lambda: bank.reset_export()):      # before configure
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID
    for bad in ((0, 1, 5), (4, 0, 5), (fmt, 2, 5), (fmt, 1, 5, 1)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_export(ExportRule(*bad), ch)
        assert err.value.status == capi.ERR_INVALID, bad
    for channels in (0, 9):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_export(ExportRule(*rule), channels)
        assert err.value.status == capi.ERR_INVALID, channels
    with pytest.raises(capi.OmxError):
        bank.fetch_exported(0)                                          # a refused configure configured nothing
    bank.configure_export(ExportRule(*rule), ch)
    bank.configure_export(ExportRule(pr.S16, pr.NONE, 9), ch)           # again, while every position is 0
    bank.configure_export(ExportRule(*rule), ch)
    ptr = bank.export_pcm(**good)
    torch_dev.cuda.synchronize()
    everything, records = store.cpu().numpy().tobytes(), device_bytes(ptr, n * 48)
    assert [int(bank.fetch_exported(s)["frames_out"]) for s in range(n)] == [100, 0, 50]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert store.cpu().numpy().tobytes() == everything, tag
        assert device_bytes(ptr, n * 48) == records, tag

    bad_calls = {"d_out inside d_in": dict(d_out=d_f32 + 4), "d_out one dword below the end of d_in": dict(d_out=d_f32 + f32_bytes - 4),
                 "d_in inside d_out": dict(d_in=d_int + 8), "the same buffer": dict(d_out=d_f32),
                 "d_out two bytes off a dword": dict(d_out=d_int + 2), "d_out one byte off a dword": dict(d_out=d_int + 1),
                 "frames[s] > frames_capacity": dict(frames=[cap + 1, 0, 0]), "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                 "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.export_pcm(**{**good, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    raw_fn = omx.fn("program_loudness_bank_export_pcm", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p])
    counts = np.array([1, 1, 1], np.uint32)
    assert raw_fn(bank._h, C.c_void_p(d_f32), C.c_void_p(d_int), cap, counts.ctypes.data, None, None) == capi.ERR_INVALID      # null d_exported
    unchanged("null d_exported")
    with pytest.raises(capi.OmxError) as err:                           # configure while a position is not 0
        bank.configure_export(ExportRule(pr.S16, pr.NONE, 9), ch)
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_exported(n)
    assert err.value.status == capi.ERR_INVALID
    unchanged("configure while a position is not 0")
    # import: the same refusals, and nothing written
    bad_imports = {"unknown format": dict(format=0), "unknown format 4": dict(format=4), "channels 0": dict(channels=0), "channels 9": dict(channels=9),
                   "d_in two bytes off a dword": dict(d_in=d_int + 2), "d_out inside d_in": dict(d_out=d_int + 8), "d_in inside d_out": dict(d_in=d_f32 + 16),
                   "frames[s] > frames_capacity": dict(frames=[0, cap + 1, 0]), "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                   "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    good_import = dict(d_in=d_int, format=fmt, d_out=d_f32, frames_capacity=cap, channels=ch, frames=[100, 0, 50])
    for tag, change in bad_imports.items():
        with pytest.raises(capi.OmxError) as err:
            bank.import_pcm(**{**good_import, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged("import: " + tag)
    # none of the refusals moved the host's mirror: the next call continues where the streams stood
    rows = [x[0, 100:150], x[1, :10], x[2, 50:50]]
    got, _ = run_export(torch_dev, bank, rows, 60, ch, fmt)
    for s, (r, at) in enumerate(zip(rows, (100, 0, 50))):
        assert got[s] == pr.export_pcm(r, rule, s, at)[0], s
    bank.reset_export()
    bank.configure_export(ExportRule(pr.S16, pr.NONE, 9), ch)           # after a reset of every stream it is allowed again
    assert bank.fetch_exported(0)["format"] == pr.S16


# ---------------------------------------------------------------- 7. the C99 host
def demo_programme():
    state, out = 12345, np.zeros(192000, np.int16)
    for i in range(out.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        v = ((state >> 16) & 0x3FFF) - 8192
        out[i] = 3 * v if (i // 2) % 24000 < 2400 else v
    return out


def test_c99_demo_prints_the_python_routes_records(torch_dev, omx, tmp_path):
    """tests/c_abi/program_pcm_demo.c: import, process, plan_gains, apply_limited and the export as S16 with TPDF from a plain C host"""
    from test_cpu_program_pcm import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    printed = {tok[i]: tok[i + 1] for i in range(0, len(tok), 2)}
    fs, ch, frames = 48000.0, 2, 96000
    bank = new_bank(omx, 1, ch, fs)
    d_pcm = torch_dev.from_numpy(demo_programme().view(np.uint8).copy()).cuda()
    d_f32, d_lim = (torch_dev.zeros((1, frames, ch), dtype=torch_dev.float32).cuda() for _ in range(2))
    d_out = torch_dev.zeros((frames * ch * 2,), dtype=torch_dev.uint8).cuda()
    bank.import_pcm(d_pcm.data_ptr(), pr.S16, d_f32.data_ptr(), frames, ch)
    bank.process(d_f32.data_ptr(), frames, ch, fs, capi.positions_fallback(ch))
    ptr = bank.plan_gains(GainRule(-10.0, -1.0, -60.0, 60.0, 0))
    bank.configure_limiter(LimitRule(-1.0, 64, 0), ch, fs)
    bank.apply_limited(d_f32.data_ptr(), frames, d_lim.data_ptr(), frames, ptr, 1, flush_mask=[1])
    bank.configure_export(ExportRule(pr.S16, pr.TPDF, 2024), ch)
    bank.export_pcm(d_lim.data_ptr(), d_out.data_ptr(), frames)
    torch_dev.cuda.synchronize()
    rec, g, lim, e = bank.fetch(0), bank.fetch_gains()[0], bank.fetch_limited(0), bank.fetch_exported(0)
    checksum = 1469598103934665603
    for byte in d_out.cpu().numpy().tobytes():
        checksum = ((checksum ^ byte) * 1099511628211) & (2 ** 64 - 1)
    want = {"integrated_lufs": f"{float(rec.integrated_lufs):.4f}", "gain_db": f"{float(g['gain_db']):.4f}", "frames_limited": str(int(lim["frames_limited"])),
            "min_envelope": f"{float(lim['min_envelope']):.6f}", "limiter_peak": f"{float(lim['out_sample_peak']):.6f}", "frames_out": str(int(e["frames_out"])),
            "frames_written": str(int(e["frames_written"])), "samples_clipped": str(int(e["samples_clipped"])), "samples_nan": str(int(e["samples_nan"])),
            "out_peak": str(int(e["out_peak"])), "out_peak_db": f"{float(e['out_peak_db']):.4f}", "format": "1", "dither": "1", "checksum": str(checksum)}
    assert printed == want, (printed, want)
    assert int(e["frames_out"]) == frames and int(lim["frames_limited"]) > 0 and 0 < int(e["out_peak"]) < 32768

"""Programme bank limiter on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_limiter / apply_limited / fetch_limited
against the numpy restatement (tests/program_limit_ref.py, pinned by tests/test_cpu_program_limit.py, which also proves the round
trip's inputs fair: their restated output stays within 0.01 dB of the ceiling in true peak).

Bars.  Every float of d_out equal bits to the restatement; every record field equal bits except the two dB fields, within 1e-4 dB (as
the peak tests).  Cut invariance: the concatenated output of any schedule of calls has the bytes of the one-call output.  Round trip:
measured maximum true peak <= ceiling + 0.01 dB; integrated loudness within 1e-4 LU of the restatement's prediction.
Tile lengths named here: lr.LEVEL_TILE (kLmLevelTile), lr.HOLD_TILE (kLmHoldTile), lr.SMOOTH_TILE (kLmSmoothTile) and
lr.APPLY_TILE_FLOATS (kLmApplyTileFloats); lr.case_lengths puts a stream length one frame beside an end of each.
No test provokes a fault: the refusals use only arguments the host rejects before any launch."""
import numpy as np
import pytest

import program_limit_ref as lr
import program_loudness_ref as ref
import program_normalize_ref as nr
import program_peaks_ref as pk
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, LIMIT_RECORD_DTYPE, UNITY_GAIN, GainRule, LimitRule, ProgramLoudnessBank
from parity import bar
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
TRUE_PEAK_BAR_DB = 0.01


@pytest.fixture(scope="module")
def coeffs(oracle):
    return pk.coefficients(oracle)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def gains_on_device(torch, factors):
    g = np.zeros((len(factors),), GAIN_RECORD_DTYPE)
    g["gain"] = np.asarray(factors, np.float32)
    return torch.from_numpy(g.view(np.uint8).copy()).cuda(), g


def limiter_bank(omx, n, ch, fs, rule):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)
    bank.configure_limiter(LimitRule(*rule), ch, fs)
    return bank


def drive(torch, bank, xs, ch, schedule, rule, d_gains, n_gains, route=None, flush_with_last=False):
    """Feeds stream s its programme xs[s] in calls of schedule[k][s] frames, then flushes every stream (in a call of its own that brings
    no frames, or with the last call).  Rows of d_in beyond frames[s] hold other samples, d_out is filled with a sentinel and one
    frame longer than the longest emission.  -> (per stream the concatenated output, the device pointer to the records)"""
    n, LA = len(xs), lr.latency(rule)
    taken, emitted = [0] * n, [0] * n
    outs = [[] for _ in range(n)]
    calls = [(list(map(int, counts)), False) for counts in schedule]
    if flush_with_last:
        calls[-1] = (calls[-1][0], True)
    else:
        calls.append(([0] * n, True))
    ptr = 0
    for counts, flush in calls:
        cap = max(max(counts), 1)
        host = lr.noise(999, n * cap, ch).reshape(n, cap, ch)
        emit = []
        for s, f in enumerate(counts):
            host[s, :f] = xs[s][taken[s]:taken[s] + f]
            taken[s] += f
            e_new = taken[s] if flush else max(emitted[s], taken[s] - LA)
            emit.append(e_new - emitted[s])
            emitted[s] = e_new
        out_cap = max(emit) + 1
        d_in = torch.from_numpy(host).cuda()
        d_out = torch.full((n, out_cap, ch), float(SENTINEL), dtype=torch.float32).cuda()
        ptr = bank.apply_limited(d_in.data_ptr(), cap, d_out.data_ptr(), out_cap, d_gains, n_gains, frames=counts,
                                 flush_mask=[1] * n if flush else None, gain_of_stream=route, stream=stream_of(torch))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
        for s in range(n):
            assert int(bank.fetch_limited(s)["frames_written"]) == emit[s], (s, counts, flush)
            assert (got[s, emit[s]:] == SENTINEL).all(), (s, "frames at or above frames_written were written")
            outs[s].append(got[s, :emit[s]].copy())
    assert all(taken[s] == len(xs[s]) == emitted[s] for s in range(n))
    return [np.concatenate(o) for o in outs], ptr


def rules():
    return [(lr.CEILING_DB, A, R) for A in lr.ATTACKS for R in lr.HOLDS]


def same_floats(got, want):
    """equal bits, except that a NaN may stand for any NaN: infinity times an envelope of zero makes a new NaN, and IEEE 754 leaves
    the sign and the payload of a generated NaN to the implementation (the host's differs from the device's)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    both = np.isnan(got) & np.isnan(want)
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | both).all())


def fit(schedule, xs):
    """the calls of `schedule` clipped to what every stream has left, and one more call with the rest"""
    left, out = [len(x) for x in xs], []
    for counts in schedule:
        row = [min(int(c), l) for c, l in zip(counts, left)]
        left = [l - r for l, r in zip(left, row)]
        out.append(row)
    return out + ([left] if any(left) else [])


# ---------------------------------------------------------------- 1. bit equality with the restatement
@pytest.mark.parametrize("ch", lr.CHANNELS)
@pytest.mark.parametrize("fs", lr.RATES)
def test_output_and_records_equal_the_restatement(torch_dev, omx, coeffs, fs, ch):
    """five streams (noise over the ceiling, a gated tone under a negative gain, one never limited, one with NaN and infinities, zeros),
    every attack and hold, whole programmes flushed in the call that brings them"""
    streams = lr.case_streams(100 + ch, ch, fs)
    xs, factors = [x for _, x, _ in streams], [g for _, _, g in streams]
    d_gains, _ = gains_on_device(torch_dev, factors)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, 10)
    for rule in rules():
        bank.configure_limiter(LimitRule(*rule), ch, fs)
        for s in range(len(xs)):
            idle = bank.fetch_limited(s)
            assert (idle["state"], idle["frames_in"], idle["gain"], idle["gain_index"], idle["min_envelope"]) == (lr.IDLE, 0, 1.0, UNITY_GAIN, 1.0)
            assert idle["latency_frames"] == lr.latency(rule) and idle["ceiling"].tobytes() == lr.ceiling(rule).tobytes()
        outs, ptr = drive(torch_dev, bank, xs, ch, [[len(x) for x in xs]], rule, d_gains.data_ptr(), len(xs), flush_with_last=True)
        limited = 0
        for s, (name, x, g) in enumerate(streams):
            want, gf, rec = lr.restate(x, fs, coeffs, g, rule, FLOOR)
            rec["gain_index"] = s
            assert same_floats(outs[s], want), (fs, ch, rule, name, "output differs from the restatement")
            got = bank.fetch_limited(s)
            lr.check_record(got, rec, (fs, ch, rule, name))
            limited += int(got["frames_limited"])
            if name == "never limited":
                assert got["frames_limited"] == 0 and got["min_envelope"] == 1.0
                assert outs[s].tobytes() == nr.apply(x, g)[0].tobytes()
        assert limited > 0
        assert device_bytes(ptr, len(xs) * 80) == b"".join(bank.fetch_limited(s).tobytes() for s in range(len(xs)))
        bank.reset_limiter()


def test_longest_attack_and_hold(torch_dev, omx, coeffs):
    """A = 4096, R = 16384: a window longer than one hold tile takes (the minimum of shifted windows), the longest rings"""
    fs, ch, rule = 48000.0, 2, (lr.CEILING_DB, 4096, 16384)
    xs = [lr.noise(40, 6000, ch), lr.gated_tone(41, 5000, ch, fs), lr.noise(42, 4097, ch, 0.05)]
    d_gains, _ = gains_on_device(torch_dev, [lr.GAIN] * 3)
    bank = limiter_bank(omx, 3, ch, fs, rule)
    cuts = [[2000, 1, 4097], [0, 4999, 0], [4000, 0, 0]]
    outs, _ = drive(torch_dev, bank, xs, ch, cuts, rule, d_gains.data_ptr(), 3)
    for s, x in enumerate(xs):
        want, _, rec = lr.restate(x, fs, coeffs, lr.GAIN, rule, FLOOR)
        rec.update(gain_index=s, frames_written=bank.fetch_limited(s)["frames_written"])
        assert outs[s].tobytes() == want.tobytes(), s
        lr.check_record(bank.fetch_limited(s), rec, s)


# ---------------------------------------------------------------- 2. cut invariance
@pytest.mark.parametrize("fs,ch,rule", [(48000.0, 2, (lr.CEILING_DB, 16, 100)), (96000.0, 3, (lr.CEILING_DB, 240, 0)),
                                        (192000.0, 8, (lr.CEILING_DB, 1, 0)), (48000.0, 1, (lr.CEILING_DB, 240, 100))])
def test_output_does_not_depend_on_the_cuts(torch_dev, omx, fs, ch, rule):
    streams = lr.case_streams(200 + ch, ch, fs)
    xs, factors = [x for _, x, _ in streams], [g for _, _, g in streams]
    n, LA = len(xs), lr.latency(rule)
    d_gains, _ = gains_on_device(torch_dev, factors)
    bank = limiter_bank(omx, n, ch, fs, rule)
    whole, _ = drive(torch_dev, bank, xs, ch, [[len(x) for x in xs]], rule, d_gains.data_ptr(), n)
    records = [bank.fetch_limited(s) for s in range(n)]
    small = [[0] * n, [1] * n, [LA - 1] * n, [1, 0, 1, 0, 1], [0, 1, 0, 1, 0], [LA - 1, 0, 1, LA, 0]]
    per_stream = [lr.ragged_cuts(300 + s, len(x)) for s, x in enumerate(xs)]
    ragged = [[c[k] if k < len(c) else 0 for c in per_stream] for k in range(max(len(c) for c in per_stream))]
    tiles = [[t] * n for t in (lr.LEVEL_TILE - 1, 2, lr.LEVEL_TILE)]          # one frame short of a tile, one beyond it, one beyond the next
    for name, schedule in (("0, 1 and LA - 1 frames", small), ("ragged", ragged), ("around a level tile", tiles)):
        bank.reset_limiter()
        assert all(bank.fetch_limited(s)["state"] == lr.IDLE for s in range(n))
        outs, _ = drive(torch_dev, bank, xs, ch, fit(schedule, xs), rule, d_gains.data_ptr(), n)
        for s in range(n):
            assert outs[s].tobytes() == whole[s].tobytes(), (fs, ch, rule, name, s)
            got = bank.fetch_limited(s)
            for f in lr.EXACT_FIELDS + ("out_sample_peak_db", "max_reduction_db"):
                if f != "frames_written":
                    assert got[f].tobytes() == records[s][f].tobytes(), (name, s, f, got[f], records[s][f])


# ---------------------------------------------------------------- 3. a limiter that never engages is apply_gains
def test_idle_limiter_equals_apply_gains(torch_dev, omx):
    fs, ch, rule = 48000.0, 3, (lr.CEILING_DB, 16, 100)
    xs = [lr.noise(50 + s, f, ch, 0.1) for s, f in enumerate((3000, 1001, 257))]
    xs[1][[3, 500, 1000], [0, 1, 2]] = np.array([1e-40, -3e-42, -0.0], np.float32)      # denormals and -0.0 pass as they do through apply_gains
    factors = [2.0, -1.5, 0.3]
    d_gains, _ = gains_on_device(torch_dev, factors)
    bank = limiter_bank(omx, 3, ch, fs, rule)
    cuts = [[1000, 1001, 100], [2000, 0, 157]]
    outs, _ = drive(torch_dev, bank, xs, ch, cuts, rule, d_gains.data_ptr(), 3)
    cap = max(len(x) for x in xs)
    host = np.zeros((3, cap, ch), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    d_in = torch_dev.from_numpy(host).cuda()
    d_out = torch_dev.empty_like(d_in)
    bank.apply_gains(d_in.data_ptr(), d_out.data_ptr(), cap, ch, d_gains.data_ptr(), 3, frames=[len(x) for x in xs], stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    plain = d_out.cpu().numpy()
    for s, x in enumerate(xs):
        assert outs[s].tobytes() == plain[s, :len(x)].tobytes(), s
        rec, applied = bank.fetch_limited(s), bank.fetch_applied(s)
        assert (rec["frames_limited"], rec["min_envelope"], rec["state"]) == (0, 1.0, lr.FLUSHED)
        assert rec["samples_over"] == applied["samples_over"] and rec["out_sample_peak"].tobytes() == applied["out_sample_peak"].tobytes()


# ---------------------------------------------------------------- 4. round trip
def records_of(bank):
    return [record_array(bank.fetch(s)) for s in range(bank.n_streams)]


def test_round_trip_reaches_the_ceiling_and_the_predicted_loudness(torch_dev, omx, oracle, coeffs):
    """plan to -14 LUFS without the peak limit (the predicted peaks lie above -1 dBTP), apply_limited, measure d_out with a fresh bank.
    tests/test_cpu_program_limit.py measured the restated output's true peak at about 1e-6 dB over the ceiling; the measured bank
    figure may differ from that by the f32 logarithm (1e-5 dB), far inside the 0.01 dB bar.  Measurement state: every record of the
    first bank has the same bytes before and after the limiter's calls"""
    fs, ch, rule = lr.ROUND_TRIP_RATE, 2, lr.ROUND_TRIP_RULE
    pos = capi.positions_fallback(2)
    xs = lr.round_trip_programmes()
    n, frames = len(xs), lr.ROUND_TRIP_FRAMES
    d = torch_dev.from_numpy(np.stack(xs)).cuda()
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)
    bank.set_peaks(True)
    bank.process(d.data_ptr(), frames, ch, fs, pos, stream=stream_of(torch_dev))
    ptr = bank.plan_gains(GainRule(lr.ROUND_TRIP_TARGET, lr.CEILING_DB, -60.0, 60.0, 0), stream=stream_of(torch_dev))
    gains = bank.fetch_gains()
    before, peaks_before = [r.tobytes() for r in records_of(bank)], [bank.fetch_peaks(s).tobytes() for s in range(n)]
    assert all(g["limited_by"] == nr.BY_TARGET and float(g["predicted_peak_db"]) > lr.CEILING_DB for g in gains), gains
    bank.configure_limiter(LimitRule(*rule), ch, fs)
    d_out = torch_dev.full((n, frames, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    assert bank.apply_limited(d.data_ptr(), frames, d_out.data_ptr(), frames, ptr, n, flush_mask=[1] * n, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert [r.tobytes() for r in records_of(bank)] == before and [bank.fetch_peaks(s).tobytes() for s in range(n)] == peaks_before, \
        "a limiter call changed a measurement"
    assert bank.fetch_gains().tobytes() == gains.tobytes()
    fresh = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)
    fresh.set_peaks(True)
    fresh.process(d_out.data_ptr(), frames, ch, fs, pos, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    kw = oracle.k_weighting_coefficients(ref.sanitize_rate(fs))
    for s, x in enumerate(xs):
        want, _, rec = lr.restate(x, fs, coeffs, gains[s]["gain"], rule, FLOOR)
        rec["gain_index"] = s
        assert got[s].tobytes() == want.tobytes(), s
        lr.check_record(bank.fetch_limited(s), rec, s)
        assert rec["frames_limited"] > 0
        after, predicted = fresh.fetch(s), ref.restate(want, fs, pos, kw, FLOOR)
        over = float(after.max_true_peak_db) - lr.CEILING_DB
        print(f"round trip {s}: gain {float(gains[s]['gain_db']):+.2f} dB, predicted peak {float(gains[s]['predicted_peak_db']):+.2f} dBTP, measured "
              f"{float(after.max_true_peak_db):+.5f} dBTP ({over:+.2e} dB over the ceiling), {float(after.integrated_lufs):.4f} LUFS, restated "
              f"{float(predicted['integrated_lufs']):.4f}")
        assert over <= TRUE_PEAK_BAR_DB, (s, after.max_true_peak_db)
        bar("program limit: |integrated - restated| LU", abs(float(after.integrated_lufs) - float(predicted["integrated_lufs"])), BAR, s)


# ---------------------------------------------------------------- 5. routing and refusals
def test_gain_routing_and_the_latch(torch_dev, omx, coeffs):
    fs, ch, rule, n = 48000.0, 2, (lr.CEILING_DB, 16, 0), 4
    xs = [lr.noise(60 + s, 600, ch) for s in range(n)]
    d_three, three = gains_on_device(torch_dev, [0.25, 1.75, 2.5])
    route = [2, 2, UNITY_GAIN, 1]
    bank = limiter_bank(omx, n, ch, fs, rule)
    outs, _ = drive(torch_dev, bank, xs, ch, [[600] * n], rule, d_three.data_ptr(), 3, route=route)
    for s, x in enumerate(xs):
        g = 1.0 if route[s] == UNITY_GAIN else three["gain"][route[s]]
        want, _, rec = lr.restate(x, fs, coeffs, g, rule, FLOOR)
        rec.update(gain_index=route[s], frames_written=lr.latency(rule))      # the flush call brought no frames: it wrote the held ones
        assert outs[s].tobytes() == want.tobytes(), s
        lr.check_record(bank.fetch_limited(s), rec, s)
    # the gain is latched with the first frame: later calls may name another record, or none; a reset stream latches anew
    bank.reset_limiter()
    d_other, _ = gains_on_device(torch_dev, [9.0, 9.0, 9.0])
    d_in = torch_dev.from_numpy(np.concatenate([np.stack(xs), np.zeros((1, 600, ch), np.float32)])).cuda()    # (a row to spare: calls start inside row 0)
    d_out = torch_dev.full((n, 601, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    got = [[] for _ in range(n)]

    def call(first, count, d_gains, n_gains, route, flush):
        bank.apply_limited(d_in.data_ptr() + first * ch * 4, 600, d_out.data_ptr(), 601, d_gains, n_gains, frames=[count] * n,
                           flush_mask=[1] * n if flush else None, gain_of_stream=route, stream=stream_of(torch_dev))
        torch_dev.cuda.synchronize()
        out = d_out.cpu().numpy()
        for s in range(n):
            got[s].append(out[s, :int(bank.fetch_limited(s)["frames_written"])].copy())

    call(0, 0, 0, 0, [UNITY_GAIN] * n, False)                       # no frame: nothing is latched
    assert all(bank.fetch_limited(s)["state"] == lr.IDLE for s in range(n))
    call(0, 200, d_three.data_ptr(), 3, route, False)
    call(200, 300, d_other.data_ptr(), 3, [0, 1, 2, 0], False)     # other records: not read
    call(500, 100, 0, 0, [UNITY_GAIN] * n, True)
    for s in range(n):
        assert np.concatenate(got[s]).tobytes() == outs[s].tobytes(), s
        assert bank.fetch_limited(s)["gain_index"] == route[s]
    bank.reset_limiter([0, 1, 0, 0])
    assert [int(bank.fetch_limited(s)["state"]) for s in range(n)] == [lr.FLUSHED, lr.IDLE, lr.FLUSHED, lr.FLUSHED]
    bank.apply_limited(d_in.data_ptr(), 600, d_out.data_ptr(), 601, d_other.data_ptr(), 3, frames=[0, 600, 0, 0], flush_mask=[0, 1, 0, 0],
                       gain_of_stream=[0, 1, 2, 0], stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    want, _, _ = lr.restate(xs[1], fs, coeffs, 9.0, rule, FLOOR)
    assert d_out.cpu().numpy()[1, :600].tobytes() == want.tobytes() and bank.fetch_limited(1)["gain"] == 9.0


def test_refused_calls_change_nothing(torch_dev, omx):
    fs, ch, rule, n, cap = 48000.0, 2, (lr.CEILING_DB, 16, 0), 3, 200
    LA = lr.latency(rule)
    x = np.stack([lr.noise(70 + s, cap, ch) for s in range(n)])
    store = torch_dev.full((2 * x.size + 8,), float(SENTINEL), dtype=torch_dev.float32).cuda()
    store[:x.size] = torch_dev.from_numpy(x.reshape(-1)).cuda()
    d_in, d_out = store.data_ptr(), store.data_ptr() + 4 * x.size
    d_gains, _ = gains_on_device(torch_dev, [2.0, 0.5])
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)
    good = dict(d_in=d_in, frames_capacity=cap, d_out=d_out, out_capacity=cap, d_gains=d_gains.data_ptr(), n_gains=2, frames=[100, 100, 0],
                flush_mask=[0, 1, 0], gain_of_stream=[0, 1, UNITY_GAIN])
    for call in (lambda: bank.apply_limited(**good), lambda: bank.fetch_limited(0), lambda: bank.reset_limiter()):      # before configure
        with pytest.raises(capi.OmxError) as err:
            call()
        assert err.value.status == capi.ERR_INVALID
    for bad, status in (((lr.CEILING_DB, 0, 0), capi.ERR_INVALID), ((np.nan, 16, 0), capi.ERR_INVALID), ((lr.CEILING_DB, 16, 0, 1), capi.ERR_INVALID)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_limiter(LimitRule(*bad), ch, fs)
        assert err.value.status == status, bad
    for channels, rate, status in ((0, fs, capi.ERR_INVALID), (9, fs, capi.ERR_INVALID), (ch, 3000.0, capi.ERR_UNSUPPORTED)):
        with pytest.raises(capi.OmxError) as err:
            bank.configure_limiter(LimitRule(*rule), channels, rate)
        assert err.value.status == status, (channels, rate)
    with pytest.raises(capi.OmxError):
        bank.fetch_limited(0)                                           # a refused configure configured nothing
    bank.configure_limiter(LimitRule(*rule), ch, fs)
    bank.configure_limiter(LimitRule(lr.CEILING_DB, 32, 5), ch, fs)     # again, while no stream holds frames
    bank.configure_limiter(LimitRule(*rule), ch, fs)
    ptr = bank.apply_limited(**good)     # stream 0 running with 100 frames held, stream 1 flushed, stream 2 idle
    torch_dev.cuda.synchronize()
    everything = store.cpu().numpy().tobytes()
    records = device_bytes(ptr, n * 80)
    assert [int(bank.fetch_limited(s)["state"]) for s in range(n)] == [lr.RUNNING, lr.FLUSHED, lr.IDLE]
    assert [int(bank.fetch_limited(s)["frames_written"]) for s in range(n)] == [100 - LA, 100, 0]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert store.cpu().numpy().tobytes() == everything, tag
        assert device_bytes(ptr, n * 80) == records, tag

    more = {**good, "frames": [50, 0, 50], "flush_mask": None}
    bad_calls = {"frames after a flush": dict(frames=[0, 1, 0]),
                 "out_capacity too small for a running stream": dict(out_capacity=49),
                 "out_capacity too small for a flush": dict(frames=[0, 0, 0], flush_mask=[1, 0, 0], out_capacity=LA - 1),
                 "d_out inside d_in": dict(d_out=d_in + 4), "d_out one float below the end of d_in": dict(d_out=d_in + 4 * (x.size - 1)),
                 "d_in above d_out": dict(d_in=d_in + 4 * ch, d_out=d_in), "the same buffer": dict(d_out=d_in),
                 "index == n_gains": dict(gain_of_stream=[0, 1, 2]), "identity routing with fewer records than streams": dict(gain_of_stream=None),
                 "frames[s] > frames_capacity": dict(frames=[cap + 1, 0, 0]), "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 1]),
                 "out_capacity beyond 2^32 - 1": dict(out_capacity=2 ** 32),
                 "null d_gains while a stream latches a record": dict(d_gains=0, gain_of_stream=[0, 1, 1]),
                 "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.apply_limited(**{**more, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    with pytest.raises(capi.OmxError) as err:                           # configure while frames are held
        bank.configure_limiter(LimitRule(lr.CEILING_DB, 32, 5), ch, fs)
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_limited(n)
    assert err.value.status == capi.ERR_INVALID
    unchanged("configure while frames are held")
    # none of the refusals moved the host's mirror: the call they all varied is still taken, and continues where stream 0 stood
    bank.apply_limited(**more)
    torch_dev.cuda.synchronize()
    assert [int(bank.fetch_limited(s)["frames_in"]) for s in range(n)] == [150, 100, 50]
    assert [int(bank.fetch_limited(s)["frames_written"]) for s in range(n)] == [50, 0, 50 - LA]
    bank.reset_limiter()
    bank.configure_limiter(LimitRule(lr.CEILING_DB, 32, 5), ch, fs)     # after a reset of every stream it is allowed again
    assert bank.fetch_limited(0)["latency_frames"] == 55

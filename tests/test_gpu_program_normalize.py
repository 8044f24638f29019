"""Programme bank normalisation on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.plan_gains / plan_group_gains / apply_gains
against the numpy restatement (tests/program_normalize_ref.py, pinned by tests/test_cpu_program_normalize.py, which also proves the
round trip's inputs fair: every known programme keeps its gate counts and its gate margin when it is scaled).

Bars.  Plan: gain_db, predicted_*, source_*, limited_by and peak_known equal bits, `gain` within 1 f32 ulp, the restatement fed the
bank's own fetched records.  Pass: every float of d_out equal bits to x * f32(fetched gain); samples_over, out_sample_peak (bits) and
frames exact; out_sample_peak_db within 1e-4 dB.  Round trip: 1e-4 LU / dB (the project's loudness bar), gate counts exact.
No test provokes a fault: the refusals use only arguments the host rejects before any launch."""
import ctypes as C

import numpy as np
import pytest

import program_groups_ref as gr
import program_normalize_ref as nr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (GAIN_RECORD_DTYPE, TO_END, UNITY_GAIN, GainRule,
                                             ProgramLoudnessBank)
from parity import bar
from test_gpu_program_loudness import BAR, FLOOR, device_rows, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(777.25)
COUNT_FIELDS = ("gating_above_absolute", "gating_above_relative", "short_term_above_absolute", "short_term_above_relative")
POS2 = capi.positions_fallback(2)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def known_bank(torch, omx, d, longest, peaks=True, storage="segments"):
    """a bank that has taken the five known programmes (device array d), whole, in one call"""
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=gr.KNOWN_RATE), 5, 2, 30, storage=storage)
    if peaks:
        bank.set_peaks(True)
    bank.process(d if isinstance(d, int) else d.data_ptr(), longest, 2, gr.KNOWN_RATE, POS2, stream=stream_of(torch))
    torch.cuda.synchronize()
    return bank


@pytest.fixture(scope="module")
def known(torch_dev, omx):
    """the known programmes on the device and a bank with peaks on that has measured them, made once"""
    xs = gr.known_programmes()
    d, longest = device_rows(torch_dev, xs, 2)
    assert all(len(x) == longest for x in xs)
    return d, longest, known_bank(torch_dev, omx, d, longest)


def records_of(bank):
    return [record_array(bank.fetch(s)) for s in range(bank.n_streams)]


def gains_on_device(torch, factors):
    """caller-made gain records: only `gain` is read by the pass"""
    g = np.zeros((len(factors),), GAIN_RECORD_DTYPE)
    g["gain"] = np.asarray(factors, np.float32)
    g["gain_db"] = np.float32(np.nan)
    return torch.from_numpy(g.view(np.uint8).copy()).cuda(), g


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_applied(bank, s, x, factor, index, tag):
    """the apply record of stream s against the restatement of x (the frames it brought) * factor"""
    got = bank.fetch_applied(s)
    want_out, over, peak = nr.apply(x, factor)
    assert int(got["frames"]) == len(x) and int(got["samples_over"]) == over, (tag, s, got, over)
    assert got["out_sample_peak"].tobytes() == np.float32(peak).tobytes(), (tag, s, got["out_sample_peak"], peak)
    assert got["gain"].tobytes() == np.float32(factor).tobytes() and int(got["gain_index"]) == index, (tag, s, got)
    want_db = nr.peak_db(peak, FLOOR)
    if np.isinf(want_db):
        assert np.isinf(got["out_sample_peak_db"]) and got["out_sample_peak_db"] > 0, (tag, s, got)
    else:
        print(tag, s, "out_sample_peak_db", got["out_sample_peak_db"], "restated", want_db)
        assert abs(float(got["out_sample_peak_db"]) - want_db) <= 1e-4, (tag, s, got["out_sample_peak_db"], want_db)
    return want_out


# ---------------------------------------------------------------- 1. plan against the restatement
EXPECTED_BY = {nr.RULE_TARGET: [nr.BY_TARGET] * 5, nr.RULE_CEILING: [nr.BY_PEAK] * 5,
               nr.RULE_CLAMPS: [nr.BY_MIN_GAIN, nr.BY_PEAK, nr.BY_MAX_GAIN, nr.BY_MIN_GAIN, nr.BY_MAX_GAIN]}
EXPECTED_BY_WITHOUT_PEAKS = {nr.RULE_TARGET: [nr.BY_TARGET] * 5, nr.RULE_CEILING: [nr.BY_TARGET] * 5,
                             nr.RULE_CLAMPS: [nr.BY_TARGET, nr.BY_MAX_GAIN, nr.BY_MAX_GAIN, nr.BY_MIN_GAIN, nr.BY_MAX_GAIN]}


@pytest.mark.parametrize("peaks,storage", [(True, "segments"), (False, "segments"), (True, "histogram")])
def test_plan_gains_against_the_restatement(torch_dev, omx, known, peaks, storage):
    d, longest, shared = known
    bank = shared if (peaks, storage) == (True, "segments") else known_bank(torch_dev, omx, d, longest, peaks, storage)
    before = records_of(bank)
    peak_before = bank.fetch_peaks(0).tobytes() if peaks else None
    scratch = d.clone()
    for rule in (nr.RULE_TARGET, nr.RULE_CEILING, nr.RULE_CLAMPS):
        ptr = bank.plan_gains(GainRule(*rule), stream=stream_of(torch_dev))
        got = bank.fetch_gains()
        assert len(got) == 5 and device_bytes(ptr, 5 * 32) == got.tobytes()
        for s in range(5):
            src = before[s]
            nr.check_record(got[s], nr.gain(rule, src["integrated_lufs"], src["gating_above_relative"], src["max_true_peak_db"], FLOOR),
                            (peaks, storage, rule, s))
            assert got[s]["peak_known"] == (1 if peaks else 0)
            if not peaks:
                assert src["max_true_peak_db"] == np.float32(FLOOR) and got[s]["predicted_peak_db"] == np.float32(FLOOR)
        assert [int(b) for b in got["limited_by"]] == (EXPECTED_BY if peaks else EXPECTED_BY_WITHOUT_PEAKS)[rule], (rule, got["limited_by"])
        assert bank.fetch_gains(1, 3).tobytes() == got[1:4].tobytes() and len(bank.fetch_gains(5, 0)) == 0
        assert [r.tobytes() for r in records_of(bank)] == [r.tobytes() for r in before], "plan_gains changed a measurement"
        print(storage, "peaks" if peaks else "no peaks", rule, got["gain_db"], got["limited_by"])
    # ... and apply_gains changes none either; the plan's records outlive it
    planned = bank.fetch_gains().tobytes()
    bank.apply_gains(scratch.data_ptr(), scratch.data_ptr(), longest, 2, ptr, 5, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert [r.tobytes() for r in records_of(bank)] == [r.tobytes() for r in before], "apply_gains changed a measurement"
    assert bank.fetch_gains().tobytes() == planned and device_bytes(ptr, 5 * 32) == planned
    if peaks:
        assert bank.fetch_peaks(0).tobytes() == peak_before


# ---------------------------------------------------------------- 2. album plan
def test_plan_group_gains_against_the_restatement(torch_dev, omx, known):
    _, _, bank = known
    names = list(gr.KNOWN_GROUPS)          # "-23 and -29" and "-23, -29 and -50" overlap: they share two members
    members = gr.KNOWN_MEMBERS + [(3, 50, 100), (1, 0, TO_END)]
    groups = [gr.KNOWN_GROUPS[n] for n in names] + [(5, 0), (5, 2), (0, 7)]      # an empty group, one with a PART of stream 3, all
    streams = records_of(bank)
    for rule in (nr.RULE_TARGET, nr.RULE_CEILING, nr.RULE_CLAMPS):
        ptr = bank.plan_group_gains(GainRule(*rule), members, groups, stream=stream_of(torch_dev))
        got = bank.fetch_gains()
        assert len(got) == len(groups) and device_bytes(ptr, len(groups) * 32) == got.tobytes()
        measured = bank.fetch_groups(members, groups)
        for k, (first, count) in enumerate(groups):
            peaks = [streams[s]["max_true_peak_db"] for s, _, _ in members[first:first + count]]
            peak = np.float32(max(peaks)) if peaks else np.float32(FLOOR)
            assert got[k]["source_lufs"].tobytes() == measured[k]["integrated_lufs"].tobytes(), (rule, k)
            assert got[k]["source_peak_db"].tobytes() == peak.tobytes(), (rule, k, got[k]["source_peak_db"], peak)
            nr.check_record(got[k], nr.gain(rule, measured[k]["integrated_lufs"], measured[k]["gating_above_relative"], peak, FLOOR), (rule, k))
        empty = got[len(names)]
        assert (empty["limited_by"], empty["gain_db"], empty["gain"], empty["peak_known"]) == (nr.BY_NO_MEASUREMENT, 0.0, 1.0, 0)
        assert empty["source_peak_db"] == np.float32(FLOOR) and empty["source_lufs"] == np.float32(FLOOR)
        part = got[len(names) + 1]         # the part's peak is its stream's whole-programme figure: conservative
        assert part["source_peak_db"] == max(streams[3]["max_true_peak_db"], streams[1]["max_true_peak_db"]) and part["peak_known"] == 1
        print(rule, got["gain_db"], got["limited_by"])
    bank.plan_group_gains(GainRule(*nr.RULE_TARGET), members, groups)
    album = bank.fetch_gains(names.index("-23 and -29"), 1)[0]
    assert album["limited_by"] == nr.BY_TARGET and abs(float(album["gain_db"]) - (-23.0 - gr.KNOWN_ALBUM_LUFS)) <= 0.1, album
    assert [r.tobytes() for r in records_of(bank)] == [r.tobytes() for r in streams], "plan_group_gains changed a measurement"
    # no group: nothing is planned, the earlier plan stays
    assert bank.plan_group_gains(GainRule(*nr.RULE_CEILING), members, []) == 0
    assert bank.fetch_gains(names.index("-23 and -29"), 1)[0].tobytes() == album.tobytes()


# ---------------------------------------------------------------- 3. the pass is exact
def apply_case(torch, omx, xs, capacity, ch, factors, in_place, tag, in_offset=0, out_offset=0):
    """xs[s]: the frames stream s brings (f32 [frames][ch]); rows beyond them hold other seeded samples.  *_offset: floats by which the
    buffer is moved off its 16-byte boundary"""
    n = len(xs)
    host = np.stack([nr.noise(1000 + s, capacity, ch) for s in range(n)])
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    flat = host.reshape(-1)
    d_in_store = torch.zeros(flat.size + 4, dtype=torch.float32).cuda()
    d_in_store[in_offset:in_offset + flat.size] = torch.from_numpy(flat).cuda()
    in_ptr = d_in_store.data_ptr() + 4 * in_offset
    assert d_in_store.data_ptr() % 16 == 0
    if in_place:
        d_out_store, out_ptr, out_offset = d_in_store, in_ptr, in_offset
    else:
        d_out_store = torch.full((flat.size + 4,), float(SENTINEL), dtype=torch.float32).cuda()
        out_ptr = d_out_store.data_ptr() + 4 * out_offset
        assert d_out_store.data_ptr() % 16 == 0
    d_gains, _ = gains_on_device(torch, factors)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
    status_ptr = bank.apply_gains(in_ptr, out_ptr, capacity, ch, d_gains.data_ptr(), len(factors), frames=[len(x) for x in xs],
                                  stream=stream_of(torch))
    torch.cuda.synchronize()
    assert status_ptr
    got_all = d_out_store.cpu().numpy()
    got = got_all[out_offset:out_offset + flat.size].reshape(n, capacity, ch)
    for s, x in enumerate(xs):
        want = check_applied(bank, s, x, factors[s], s, tag)
        assert same_bits(got[s, :len(x)], want), (tag, s, "scaled frames differ")
        rest = got[s, len(x):]
        if in_place:
            assert same_bits(rest, host[s, len(x):]), (tag, s, "frames at or above frames[s] were written")
        else:
            assert (rest == SENTINEL).all(), (tag, s, "frames at or above frames[s] were written")
    if not in_place:
        assert same_bits(d_in_store.cpu().numpy()[in_offset:in_offset + flat.size], flat), (tag, "d_in changed")
        outside = np.concatenate([got_all[:out_offset], got_all[out_offset + flat.size:]])
        assert (outside == SENTINEL).all(), (tag, "floats outside d_out were written")
    assert device_bytes(status_ptr, n * 32) == b"".join(bank.fetch_applied(s).tobytes() for s in range(n))
    return bank


def ragged_streams(ch, seed):
    """every frame count of nr.APPLY_FRAMES twice: once with planted NaN, infinities, denormals and -0.0, once finite (so that peaks
    and counts are checked on finite rows too)"""
    xs = []
    for i, frames in enumerate(nr.APPLY_FRAMES):
        x = nr.noise(seed + i, frames, ch)
        xs += [nr.planted(x, seed + i), x]
    return xs


FACTORS = [0.5, 1.25, 2.0, 0.1, 1.0, 3.0, 1.1111112, 0.9, 1.5]


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("ch", nr.APPLY_CHANNELS)
def test_apply_is_exact_on_ragged_rows(torch_dev, omx, ch, in_place):
    """frames_capacity 1001: the rows of 3 and 5 channels start off a 16-byte boundary (heads of 1, 2 and 3 floats)"""
    xs = ragged_streams(ch, 10 * ch)
    apply_case(torch_dev, omx, xs, nr.APPLY_CAPACITY, ch, (FACTORS * 2)[:len(xs)][::-1] + [], in_place, ("ragged", ch, in_place))


@pytest.mark.parametrize("in_place", [False, True])
def test_apply_is_exact_on_a_row_of_many_tiles(torch_dev, omx, in_place):
    """70 001 frames x 2 channels: 35 tiles, the last one partial, two floats behind the last whole vector; the second row starts 8 bytes
    off a 16-byte boundary"""
    xs = [nr.planted(nr.noise(70, nr.LONG_FRAMES, nr.LONG_CHANNELS), 70), nr.noise(71, nr.LONG_FRAMES, nr.LONG_CHANNELS),
          nr.noise(72, 4097, nr.LONG_CHANNELS)]
    apply_case(torch_dev, omx, xs, nr.LONG_FRAMES, nr.LONG_CHANNELS, [1.3, 1.2, 0.7], in_place, ("long", in_place))


OFFSET_CASES = [(ch, a_in, a_out) for ch in (2, 3, 8) for a_in in range(4) for a_out in range(4)]      # (2 channels keep their earlier ids)


@pytest.mark.parametrize("ch,in_offset,out_offset", OFFSET_CASES,
                         ids=[f"{a_in}-{a_out}" if ch == 2 else f"{a_in}-{a_out}-{ch}ch" for ch, a_in, a_out in OFFSET_CASES])
def test_apply_is_exact_when_loads_and_stores_are_aligned_differently(torch_dev, omx, ch, in_offset, out_offset):
    """d_in one float off a 16-byte boundary against an aligned d_out (the dword-load form), and every other pair of offsets; at 8
    channels a row leaves its boundary through the offset alone"""
    xs = [nr.planted(nr.noise(80 + s, f, ch), 80 + s) for s, f in enumerate((1000, 999, 517, 3, 0, 2100))]
    apply_case(torch_dev, omx, xs, 2100, ch, [1.7, 0.3, 1.0, 2.5, 4.0, 1.05], False, ("offsets", ch, in_offset, out_offset), in_offset, out_offset)


# ---------------------------------------------------------------- 4. gain routing
def test_gain_routing(torch_dev, omx):
    ch, cap, n = 2, 300, 6
    xs = [nr.planted(nr.noise(90 + s, cap - 7 * s, ch), 90 + s) for s in range(n)]
    host = np.zeros((n, cap, ch), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    d_in = torch_dev.from_numpy(host).cuda()
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), n, ch, 10)
    frames = [len(x) for x in xs]

    def run(d_gains, n_gains, route):
        d_out = torch_dev.full((n, cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
        bank.apply_gains(d_in.data_ptr(), d_out.data_ptr(), cap, ch, d_gains, n_gains, frames=frames, gain_of_stream=route, stream=stream_of(torch_dev))
        torch_dev.cuda.synchronize()
        return d_out.cpu().numpy()

    d_three, three = gains_on_device(torch_dev, [0.25, 1.75, 1.2])
    route = [2, 2, 0, UNITY_GAIN, 1, 2]                      # several streams share one record; one stream at unity
    out = run(d_three.data_ptr(), 3, route)
    for s, x in enumerate(xs):
        factor = 1.0 if route[s] == UNITY_GAIN else three["gain"][route[s]]
        assert same_bits(out[s, :len(x)], check_applied(bank, s, x, factor, route[s], "routed")), s
    assert out[3, :frames[3]].tobytes() == host[3, :frames[3]].tobytes()       # unity: the input's bytes, NaN and -0.0 included
    out = run(None, 0, [UNITY_GAIN] * n)                       # all unity needs no records at all
    for s, x in enumerate(xs):
        assert out[s, :len(x)].tobytes() == x.tobytes() and (out[s, len(x):] == SENTINEL).all(), s
        check_applied(bank, s, x, 1.0, UNITY_GAIN, "unity")
    d_six, six = gains_on_device(torch_dev, [1.0, 0.5, 2.0, 0.75, 1.5, 0.1])
    out = run(d_six.data_ptr(), 6, None)                       # NULL: stream s uses record s
    for s, x in enumerate(xs):
        assert same_bits(out[s, :len(x)], check_applied(bank, s, x, six["gain"][s], s, "identity")), s
    out_more = run(d_six.data_ptr(), 6, list(range(n)))
    assert out_more.tobytes() == out.tobytes()
    # frames None: every stream brings frames_capacity frames
    d_out = torch_dev.full((n, cap, ch), float(SENTINEL), dtype=torch_dev.float32).cuda()
    bank.apply_gains(d_in.data_ptr(), d_out.data_ptr(), cap, ch, d_six.data_ptr(), 6, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    for s in range(n):
        assert same_bits(d_out.cpu().numpy()[s], check_applied(bank, s, host[s], six["gain"][s], s, "whole rows")), s
    # a call without frames writes the records fresh and nothing else
    assert bank.api.fn("program_loudness_bank_apply_gains", C.c_int,
                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                        C.POINTER(C.c_void_p)])(bank._h, None, None, 0, None, ch, C.c_void_p(d_six.data_ptr()), 6, None, None, C.byref(C.c_void_p())) == 0
    rec = bank.fetch_applied(2)
    assert (rec["frames"], rec["samples_over"], rec["out_sample_peak"], rec["gain"], rec["gain_index"]) == (0, 0, 0.0, 2.0, 2)
    assert rec["out_sample_peak_db"] == np.float32(FLOOR)


# ---------------------------------------------------------------- 5. round trip
def test_round_trip_lands_on_the_target_and_on_the_predicted_peak(torch_dev, omx, known):
    """plan, apply, measure d_out with a fresh bank.  The true peak is a maximum of 12-term f32 sums of scaled samples: scaling every
    sample by one f32 factor moves each term by at most half an ulp and the sum by a few ulps, far inside 1e-4 dB (1.2e-5 relative);
    the measured distance is printed"""
    d, longest, bank = known
    source = records_of(bank)
    d_out = torch_dev.empty_like(d)
    worst = {}
    for rule in (nr.RULE_TARGET, nr.RULE_CEILING):
        ptr = bank.plan_gains(GainRule(*rule), stream=stream_of(torch_dev))
        bank.apply_gains(d.data_ptr(), d_out.data_ptr(), longest, 2, ptr, 5, stream=stream_of(torch_dev))
        gains = bank.fetch_gains()
        after = records_of(known_bank(torch_dev, omx, d_out, longest))
        for s in range(5):
            g, a = gains[s], after[s]
            if g["limited_by"] == nr.BY_TARGET:
                worst["target"] = max(worst.get("target", 0.0), bar("program normalize: |integrated - target| LU", abs(float(a["integrated_lufs"]) - rule[0]), BAR, (rule, s)))
                worst["lufs"] = max(worst.get("lufs", 0.0), bar("program normalize: |integrated - predicted| LU", abs(float(a["integrated_lufs"]) - float(g["predicted_lufs"])), BAR, (rule, s)))
            else:
                assert g["limited_by"] == nr.BY_PEAK
                worst["lufs"] = max(worst.get("lufs", 0.0), bar("program normalize: |integrated - predicted| LU", abs(float(a["integrated_lufs"]) - float(g["predicted_lufs"])), BAR, (rule, s)))
                worst["peak"] = max(worst.get("peak", 0.0), bar("program normalize: |true peak - predicted| dB", abs(float(a["max_true_peak_db"]) - float(g["predicted_peak_db"])), BAR, (rule, s)))
                assert abs(float(a["max_true_peak_db"]) - rule[1]) <= BAR, (rule, s, a["max_true_peak_db"])
            for f in COUNT_FIELDS:
                assert a[f] == source[s][f], (rule, s, f)
        assert {int(b) for b in gains["limited_by"]} == ({nr.BY_TARGET} if rule == nr.RULE_TARGET else {nr.BY_PEAK})
    # the album: both members by the album gain, the rest at unity; the re-measured group sits at the target
    members, groups = gr.KNOWN_MEMBERS[:2], [(0, 2)]
    ptr = bank.plan_group_gains(GainRule(*nr.RULE_TARGET), members, groups, stream=stream_of(torch_dev))
    album = bank.fetch_gains()[0]
    bank.apply_gains(d.data_ptr(), d_out.data_ptr(), longest, 2, ptr, 1, gain_of_stream=[0, 0, UNITY_GAIN, UNITY_GAIN, UNITY_GAIN], stream=stream_of(torch_dev))
    fresh = known_bank(torch_dev, omx, d_out, longest)
    again, was = fresh.fetch_groups(members, groups)[0], bank.fetch_groups(members, groups)[0]
    worst["album"] = bar("program normalize: |album - target| LU", abs(float(again["integrated_lufs"]) + 23.0), BAR, album)
    bar("program normalize: |album - predicted| LU", abs(float(again["integrated_lufs"]) - float(album["predicted_lufs"])), BAR, album)
    for f in COUNT_FIELDS:
        assert again[f] == was[f], f
    assert record_array(fresh.fetch(2)).tobytes() == source[2].tobytes()         # a stream at unity measures as before, bit for bit
    print("round trip, measured distances (LU / dB):", {k: f"{v:.2e}" for k, v in worst.items()})


# ---------------------------------------------------------------- 6. refusals
def test_refused_calls_change_nothing(torch_dev, omx, known):
    ch, cap, n = 2, 64, 4
    x = np.stack([nr.noise(300 + s, cap, ch) for s in range(n)])
    store = torch_dev.zeros(2 * x.size + 8, dtype=torch_dev.float32).cuda()     # room for every overlapping pair below
    store[:x.size] = torch_dev.from_numpy(x.reshape(-1)).cuda()
    d_in, d_out = store.data_ptr(), store.data_ptr() + 4 * x.size
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=8000.0), n, ch, 10)
    with pytest.raises(capi.OmxError) as err:                                  # before any plan / apply
        bank.fetch_gains(0, 1)
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_applied(0)
    assert err.value.status == capi.ERR_INVALID
    bank.process(d_in, cap, ch, 8000.0, POS2, stream=stream_of(torch_dev))
    gains_ptr = bank.plan_gains(GainRule(*nr.RULE_TARGET), stream=stream_of(torch_dev))
    d_mine, _ = gains_on_device(torch_dev, [0.5, 2.0])
    applied_ptr = bank.apply_gains(d_in, d_out, cap, ch, d_mine.data_ptr(), 2, gain_of_stream=[0, 1, 1, UNITY_GAIN], stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    everything = store.cpu().numpy().tobytes()
    gains, applied, records = device_bytes(gains_ptr, n * 32), device_bytes(applied_ptr, n * 32), [r.tobytes() for r in records_of(bank)]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert store.cpu().numpy().tobytes() == everything, tag
        assert device_bytes(gains_ptr, n * 32) == gains and device_bytes(applied_ptr, n * 32) == applied, tag
        assert [r.tobytes() for r in records_of(bank)] == records, tag

    good = dict(d_in=d_in, d_out=d_out, frames_capacity=cap, channels=ch, d_gains=d_mine.data_ptr(), n_gains=2, frames=None,
                gain_of_stream=[0, 1, 1, UNITY_GAIN])
    bad_calls = {"partial overlap, d_out one float above d_in": dict(d_out=d_in + 4),
                 "partial overlap, d_out one float below the end of d_in": dict(d_out=d_in + 4 * (x.size - 1)),
                 "partial overlap, d_in above d_out": dict(d_in=d_in + 4 * ch, d_out=d_in),
                 "index == n_gains": dict(gain_of_stream=[0, 1, 2, UNITY_GAIN]),
                 "index far beyond n_gains": dict(gain_of_stream=[0, 1, 1, UNITY_GAIN - 1]),
                 "identity routing with fewer records than streams": dict(gain_of_stream=None),
                 "channels 0": dict(channels=0), "channels 9": dict(channels=9),
                 "frames[s] > frames_capacity": dict(frames=[cap, cap + 1, 0, 0]),
                 "frames_capacity beyond 2^32 - 1": dict(frames_capacity=2 ** 32, frames=[0, 0, 0, 1]),
                 "null d_gains with frames to scale": dict(d_gains=0),
                 "null d_in": dict(d_in=0), "null d_out": dict(d_out=0)}
    for tag, change in bad_calls.items():
        with pytest.raises(capi.OmxError) as err:
            bank.apply_gains(**{**good, **change})
        assert err.value.status == capi.ERR_INVALID, (tag, err.value.status)
        unchanged(tag)
    # touching buffers are no overlap: d_out right behind d_in is what `good` is
    for bad in [(np.nan, -1.0, -60.0, 60.0, 0), (-23.0, np.inf, -60.0, 60.0, nr.LIMIT_PEAK), (-23.0, -1.0, 1.0, 0.0, 0), (-23.0, -1.0, -60.0, 60.0, 4)]:
        for call in (lambda r: bank.plan_gains(r), lambda r: bank.plan_group_gains(r, [(0, 0, TO_END)], [(0, 1)]),
                     lambda r: bank.plan_group_gains(r, [], [])):
            with pytest.raises(capi.OmxError) as err:
                call(GainRule(*bad))
            assert err.value.status == capi.ERR_INVALID, bad
        unchanged(bad)
    for members, groups in ([(n, 0, TO_END)], [(0, 1)]), ([(0, 0, TO_END)], [(0, 2)]), ([(0, 1, TO_END)], [(0, 1)]):   # as measure_groups refuses
        with pytest.raises(capi.OmxError) as err:
            bank.plan_group_gains(GainRule(*nr.RULE_TARGET), members, groups)
        assert err.value.status == capi.ERR_INVALID, (members, groups)
        unchanged((members, groups))
    for first, count in ((0, n + 1), (n + 1, 0), (n, 1), (2 ** 64 - 1, 2)):
        with pytest.raises(capi.OmxError) as err:
            bank.fetch_gains(first, count)
        assert err.value.status == capi.ERR_INVALID, (first, count)
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_applied(n)
    assert err.value.status == capi.ERR_INVALID
    unchanged("fetches out of range")
    # a bounded bank keeps no segments: a member that is a part of a stream is unsupported, a whole one is planned
    d, longest, _ = known
    bounded = known_bank(torch_dev, omx, d, longest, True, "histogram")
    bounded.plan_gains(GainRule(*nr.RULE_TARGET))
    planned = bounded.fetch_gains().tobytes()
    for members in ([(0, 0, 199)], [(1, 0, TO_END), (0, 1, TO_END)]):
        with pytest.raises(capi.OmxError) as err:
            bounded.plan_group_gains(GainRule(*nr.RULE_TARGET), members, [(0, len(members))])
        assert err.value.status == capi.ERR_UNSUPPORTED, members
        assert bounded.fetch_gains().tobytes() == planned
    bounded.plan_group_gains(GainRule(*nr.RULE_TARGET), gr.KNOWN_MEMBERS[:2], [(0, 2)])
    album = bounded.fetch_gains()
    assert len(album) == 1 and album[0]["limited_by"] == nr.BY_TARGET and abs(float(album[0]["gain_db"]) - (-23.0 - gr.KNOWN_ALBUM_LUFS)) <= 0.1

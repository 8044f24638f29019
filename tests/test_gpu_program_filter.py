"""Programme bank filter stage on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.configure_filter / reset_filter / filter /
fetch_filtered against the numpy restatement (tests/program_filter_ref.py, pinned by tests/test_cpu_program_filter.py).

Bars.  Reference order: the output equals the restatement's on bytes, however the programme is cut into calls, and so does every field
of the record but out_sample_peak_db, which holds the family's 1e-4 dB (the device's logf is not numpy's).
Time-parallel form: per stream max |tp - ref| <= 2^-23 x max(peak in, peak out), one f32 ulp at the stream's loudest sample, the cost
of a single rounding flip there; derived, not tuned (test_cpu_program_filter.py holds the model of the schedule to a quarter of it
before the rounding).  No float of d_out beyond a stream's frames changes.
Shapes.  With C = filter_plan().chunk_frames the streams are 0, 1, C - 1, C, C + 1 and 4 C + 17 frames long: a work item, its seams,
four items and a ragged tile; rows of odd channel counts start at 4-byte offsets.  No test provokes a fault: the refusals use only
arguments the host rejects before any launch."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import program_filter_ref as fr
from openmeters_amd.capi import LoudnessConfig, OmxError
from openmeters_amd.program_loudness import (FILTER_BYPASS, FILTER_RECORD_DTYPE, INSPECT_DC, CProgramLoudnessRecord, CProgramPeakRecord,
                                             GainRule, InspectRule, ProgramLoudnessBank, filter_plan, inspect_summarize)
from test_cpu_program_filter import build_demo, hard_filters, hard_inputs, resonator_768k
from test_gpu_program_loudness import torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes

pytestmark = pytest.mark.gpu
FLOOR = LoudnessConfig().floor_db
SIZE = FILTER_RECORD_DTYPE.itemsize
POISON = np.float32(-777.25)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=48000.0):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, 10)


def chunk_of(omx, ch, fs=48000.0):
    return int(filter_plan(omx, ch, fs)["chunk_frames"])


def noise(seed, frames, ch, peak=1.0):
    return np.random.default_rng(seed).uniform(-peak, peak, (frames, ch)).astype(np.float32)


def rows_of(xs, ch, fill):
    cap = max(max(len(x) for x in xs), 1)
    host = np.full((len(xs), cap, ch), fill, np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    return host, cap


def run_call(torch, bank, xs, ch, in_place=False):
    """xs[s]: f32 [frames][ch] of stream s in this call.  -> the outputs, per stream; checks that nothing beyond a stream's frames was
    written and that d_in is unchanged (out of place)"""
    host, cap = rows_of(xs, ch, 0.375)
    counts = [len(x) for x in xs]
    d_in = torch.from_numpy(host).cuda()
    if in_place:
        d_out = d_in
        before = host
    else:
        before = np.full(host.shape, POISON, np.float32)
        d_out = torch.from_numpy(before).cuda()
    bank.filter(d_in.data_ptr(), d_out.data_ptr(), cap, frames=counts, stream=stream_of(torch))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for s, f in enumerate(counts):
        assert got[s, f:].tobytes() == before[s, f:].tobytes(), ("written beyond the stream's frames", s, f)
    if not in_place:
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    return [got[s, :f].copy() for s, f in enumerate(counts)]


def restate(filters, foc, xs, ch, states=None):
    """the restatement per stream -> (outputs, states)"""
    outs, sts = [], []
    for s, x in enumerate(xs):
        coef, count, bypass = fr.lane_table(filters, None if foc is None else [foc[s]], 1, ch)
        o, st = fr.run(x, coef, count, bypass, None if states is None else states[s])
        outs.append(o)
        sts.append(st)
    return outs, sts


EXACT_FIELDS = tuple(f for f in FILTER_RECORD_DTYPE.names if f != "out_sample_peak_db")


def check_record(got, want, tag):
    """every field equal, the dB figure within 1e-4 dB (the family's bar: the device's logf is not numpy's)"""
    for f in EXACT_FIELDS:
        assert got[f] == want[f], (tag, f, got, want)
    g, w = float(got["out_sample_peak_db"]), float(want["out_sample_peak_db"])
    assert g == w or abs(g - w) <= 1e-4, (tag, got, want)


def check_records(bank, outs, totals, form, tag):
    for s, o in enumerate(outs):
        check_record(bank.fetch_filtered(s), fr.record(o, totals[s], form, FLOOR), (tag, s))


def filter_table_for(fs):
    """two sections, one section with b2 = a2 = 0, one full section"""
    return [fr.design(fr.HIGHPASS, fs, 20.0, order=4), fr.design(fr.DC_BLOCK, fs, 5.0), fr.design(fr.LOW_SHELF, fs, 200.0, gain_db=6.0)]


def per_channel(n, ch):
    """filter_of_channel [n][ch]: the table's filters in turn, one channel of every stream on bypass"""
    foc = [[(s + c) % 3 for c in range(ch)] for s in range(n)]
    for s in range(n):
        foc[s][(s + 1) % ch] = FILTER_BYPASS
    return foc


def same_but_for_nan_bits(got, want):
    """equal on bytes, where a NaN that the arithmetic produced counts as any NaN (its sign and payload are the hardware's)"""
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and got[~nan].tobytes() == want[~nan].tobytes()


def bar_of(x, ref):
    return 2.0 ** -23 * max(float(np.abs(x).max()) if x.size else 0.0, float(np.abs(ref).max()) if ref.size else 0.0)


# ---------------------------------------------------------------- 1. reference order at every length, channel count and rate
@pytest.mark.parametrize("ch,fs", [(1, 48000.0), (2, 44100.0), (3, 192000.0), (6, 48000.0), (8, 44100.0)])
def test_reference_order_equals_the_restatement_at_every_length(torch_dev, omx, ch, fs):
    c = chunk_of(omx, ch, fs)
    lengths = [0, 1, c - 1, c, c + 1, 4 * c + 17]
    n = len(lengths)
    filters = filter_table_for(fs)
    xs = [noise(10 * ch + s, f, ch, 1.2) for s, f in enumerate(lengths)]
    for foc in (None, per_channel(n, ch)):
        want, _ = restate(filters, foc, xs, ch)
        for in_place in (False, True):
            bank = new_bank(omx, n, ch, fs)
            bank.configure_filter(filters, ch, fs, foc)
            bank.set_filter_form(1)
            for s in range(n):  # before the first call
                assert bank.fetch_filtered(s).tobytes() == fr.record(np.zeros((0, ch), np.float32), 0, 0, FLOOR).tobytes()
            got = run_call(torch_dev, bank, xs, ch, in_place)
            assert bank.last_filter_form() == 1
            for s in range(n):
                assert got[s].tobytes() == want[s].tobytes(), (ch, fs, foc is not None, in_place, s, np.abs(got[s] - want[s]).max())
            check_records(bank, want, lengths, 1, (ch, fs))
    assert sum(int(fr.record(o, 0, 1, FLOOR)["samples_over"]) for o in want) > 0, "the input does not exercise samples_over"


# ---------------------------------------------------------------- 2. the same programme cut into calls
def cuts_of(total, steps):
    out, at, i = [], 0, 0
    while at < total:
        k = min(steps[i % len(steps)], total - at)
        out.append(k)
        at += k
        i += 1
    return out


@pytest.mark.parametrize("ch", [2, 3])
def test_reference_order_does_not_depend_on_the_cuts(torch_dev, omx, ch):
    fs = 48000.0
    tile = int(filter_plan(omx, ch, fs)["tile_frames"])
    total, n = 4 * tile + 37, 3
    filters, foc = filter_table_for(fs), per_channel(n, ch)
    xs = [noise(77 + s, total - 11 * s, ch, 1.1) for s in range(n)]  # ragged: the shorter streams run out earlier
    want, _ = restate(filters, foc, xs, ch)
    host, cap = rows_of(xs, ch, 0.0)
    schedules = {"primes": cuts_of(total, [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]),
                 "tile edges": cuts_of(total, [tile - 1, tile + 1, tile, 2 * tile - 1, 1, 2 * tile + 1]),
                 "one frame at a time": [1] * total}
    for name, cuts in schedules.items():
        bank = new_bank(omx, n, ch, fs)
        bank.configure_filter(filters, ch, fs, foc)
        bank.set_filter_form(1)
        d = torch_dev.from_numpy(host).cuda()  # in place, every call at its offset into the rows
        at = 0
        for k in cuts:
            counts = [max(min(k, len(x) - at), 0) for x in xs]
            bank.filter(d.data_ptr() + at * ch * 4, d.data_ptr() + at * ch * 4, cap, frames=counts, stream=stream_of(torch_dev))
            at += k
        torch_dev.cuda.synchronize()
        got = d.cpu().numpy()
        for s, x in enumerate(xs):
            assert got[s, :len(x)].tobytes() == want[s].tobytes(), (name, ch, s)
        last = [max(min(cuts[-1], len(x) - (total - cuts[-1])), 0) for x in xs]
        for s, x in enumerate(xs):
            rec = bank.fetch_filtered(s)
            assert (int(rec["frames"]), int(rec["frames_total"])) == (last[s], len(x)), (name, s, rec)


def test_reset_of_one_stream_leaves_the_others(torch_dev, omx):
    ch, fs, n, frames = 2, 48000.0, 3, 700
    filters = filter_table_for(fs)
    xs = [noise(300 + s, frames, ch) for s in range(n)]
    bank = new_bank(omx, n, ch, fs)
    bank.configure_filter(filters, ch, fs)
    bank.set_filter_form(1)
    first, states = restate(filters, None, xs, ch)
    got = run_call(torch_dev, bank, xs, ch)
    assert all(got[s].tobytes() == first[s].tobytes() for s in range(n))
    before = [bank.fetch_filtered(s).tobytes() for s in range(n)]
    bank.reset_filter([0, 1, 0])
    assert [bank.fetch_filtered(s).tobytes() for s in (0, 2)] == [before[0], before[2]]
    assert bank.fetch_filtered(1).tobytes() == fr.record(np.zeros((0, ch), np.float32), 0, 0, FLOOR).tobytes()
    states[1] = None
    second, _ = restate(filters, None, xs, ch, states)
    got = run_call(torch_dev, bank, xs, ch)
    for s in range(n):
        assert got[s].tobytes() == second[s].tobytes(), s
    assert second[1].tobytes() == first[1].tobytes() and second[0].tobytes() != first[0].tobytes()
    check_records(bank, second, [2 * frames, frames, 2 * frames], 1, "after the reset")


# ---------------------------------------------------------------- 3. the time-parallel form against reference order
def check_time_parallel(got, want, xs, tag, figures):
    for s, x in enumerate(xs):
        if not len(x):
            continue
        finite = np.isfinite(want[s])
        assert (np.isfinite(got[s]) == finite).all(), (tag, s)
        err = float(np.abs(got[s].astype(np.float64) - want[s])[finite].max()) if finite.any() else 0.0
        bar = bar_of(x[np.isfinite(x)], want[s][finite])
        figures.append(err / bar if bar else 0.0)
        print(f"{tag} stream {s}: max |tp - ref| = {err:.3e} = {figures[-1]:.3f} of the bar {bar:.3e}")
        assert err <= bar, (tag, s, err, bar)


@pytest.mark.parametrize("ch,fs", [(1, 48000.0), (2, 44100.0), (3, 192000.0), (6, 48000.0), (8, 44100.0)])
def test_time_parallel_holds_the_bar_on_the_ragged_shapes(torch_dev, omx, ch, fs):
    c = chunk_of(omx, ch, fs)
    lengths = [0, 1, c - 1, c, c + 1, 4 * c + 17]
    n = len(lengths)
    filters = filter_table_for(fs)
    xs = [noise(10 * ch + s, f, ch, 1.2) for s, f in enumerate(lengths)]
    figures = []
    for foc in (None, per_channel(n, ch)):  # one filter in every wavefront; several, and lanes on bypass
        want, _ = restate(filters, foc, xs, ch)
        for in_place in (False, True):
            bank = new_bank(omx, n, ch, fs)
            bank.configure_filter(filters, ch, fs, foc)
            bank.set_filter_form(2)
            got = run_call(torch_dev, bank, xs, ch, in_place)
            assert bank.last_filter_form() == 2
            check_time_parallel(got, want, xs, (ch, fs, foc is not None, in_place), figures)
            if foc is not None:  # a lane on bypass copies its bits in this form too
                for s, x in enumerate(xs):
                    b = (s + 1) % ch
                    assert got[s][:, b].tobytes() == x[:, b].tobytes()
            for s in range(n):
                rec = bank.fetch_filtered(s)
                assert (int(rec["frames"]), int(rec["frames_total"]), int(rec["form"])) == (lengths[s], lengths[s], 2 if lengths[s] else 0)
                assert int(rec["samples_nonfinite"]) == 0
    print("largest figure:", max(figures))


@pytest.mark.parametrize("fs", [48000.0, 192000.0])
def test_time_parallel_holds_the_bar_on_the_hard_inputs(torch_dev, omx, fs):
    """DC 0.5, a 5 Hz sine at 0.5, noise at -6 dBFS and at -66 dBFS, one stream each (the second channel carries the negated
    signal), through the 20 Hz fourth-order high-pass and through DC_BLOCK at 5 Hz; in one call and cut into calls"""
    ch = 2
    c = chunk_of(omx, ch, fs)
    total = 6 * c + 17
    hard = hard_inputs(fs, total)
    xs = [np.stack([hard[:, i], -hard[:, i]], 1) for i in range(hard.shape[1])]
    n = len(xs)
    figures = []
    for name, sections in hard_filters(fs).items():
        want, _ = restate([sections], None, xs, ch)
        bank = new_bank(omx, n, ch, fs)
        bank.configure_filter([sections], ch, fs)
        bank.set_filter_form(1)
        ref = run_call(torch_dev, bank, xs, ch)
        for s in range(n):
            assert ref[s].tobytes() == want[s].tobytes(), (name, fs, s)
        bank.reset_filter()
        bank.set_filter_form(2)
        got = run_call(torch_dev, bank, xs, ch)
        assert bank.last_filter_form() == 2
        check_time_parallel(got, want, xs, (name, fs, "one call"), figures)
        bank.reset_filter()
        parts, at = [[] for _ in range(n)], 0
        for k in (2 * c + 5, c - 1, 3 * c + 13):  # the last call ends with the programme
            outs = run_call(torch_dev, bank, [x[at:at + k] for x in xs], ch, in_place=True)
            for s in range(n):
                parts[s].append(outs[s])
            at += k
        assert at == total
        check_time_parallel([np.concatenate(p) for p in parts], want, xs, (name, fs, "three calls"), figures)
    print("largest figure:", max(figures))


def test_table_with_an_ill_conditioned_filter_runs_in_reference_order(torch_dev, omx):
    ch, fs, n = 2, 768000.0, 2
    c = chunk_of(omx, ch, fs)
    filters = [fr.design(fr.HIGHPASS, fs, 20.0, order=4), resonator_768k()]
    assert fr.time_parallel_ok(filters[0]) and not fr.time_parallel_ok(filters[1])
    foc = [[0, 1], [1, 0]]
    xs = [noise(900 + s, 4 * c + 3, ch, 1e-6) for s in range(n)]
    want, _ = restate(filters, foc, xs, ch)
    bank = new_bank(omx, n, ch, fs)
    bank.configure_filter(filters, ch, fs, foc)
    for form in (2, 0):
        bank.reset_filter()
        bank.set_filter_form(form)
        got = run_call(torch_dev, bank, xs, ch)
        assert bank.last_filter_form() == 1
        for s in range(n):
            assert got[s].tobytes() == want[s].tobytes(), (form, s)
        check_records(bank, want, [len(x) for x in xs], 1, form)
    # the same rate without the resonator: the table may run in the time-parallel form
    bank = new_bank(omx, n, ch, fs)
    bank.configure_filter(filters[:1], ch, fs)
    bank.set_filter_form(2)
    run_call(torch_dev, bank, xs, ch)
    assert bank.last_filter_form() == 2


def test_form_by_call_shape(torch_dev, omx):
    ch, fs = 2, 48000.0
    c = chunk_of(omx, ch, fs)
    bank = new_bank(omx, 2, ch, fs)
    bank.configure_filter(filter_table_for(fs), ch, fs)
    assert bank.last_filter_form() == 0
    run_call(torch_dev, bank, [noise(1, 4 * c - 1, ch), noise(2, 5, ch)], ch)
    assert bank.last_filter_form() == 1
    run_call(torch_dev, bank, [noise(3, 5, ch), noise(4, 4 * c, ch)], ch)
    assert bank.last_filter_form() == 2
    with pytest.raises(OmxError):
        bank.set_filter_form(3)


# ---------------------------------------------------------------- 4. samples that are not finite, bypass bits
@pytest.mark.parametrize("form", [1, 2])
def test_nan_poisons_its_channel_from_its_frame_on(torch_dev, omx, form):
    ch, fs, n = 3, 48000.0, 2
    c = chunk_of(omx, ch, fs)
    total, k = 4 * c + 9, 2 * c + 100
    filters = [fr.design(fr.HIGHPASS, fs, 20.0, order=4)]
    foc = [[0, 0, FILTER_BYPASS], [0, FILTER_BYPASS, 0]]
    xs = [noise(40 + s, total, ch, 1.3) for s in range(n)]
    xs[0][k, 0] = np.nan
    payloads = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32).view(np.float32)
    xs[0][5:5 + len(payloads), 2] = payloads  # quiet and signalling NaNs with payloads, -0.0f, the infinities and a denormal on bypass
    xs[1][k + 1:k + 1 + len(payloads), 1] = payloads
    want, _ = restate(filters, foc, xs, ch)
    assert np.isnan(want[0][k:, 0]).all() and np.isfinite(want[0][:k, 0]).all()
    bank = new_bank(omx, n, ch, fs)
    bank.configure_filter(filters, ch, fs, foc)
    bank.set_filter_form(form)
    got = run_call(torch_dev, bank, xs, ch)
    assert bank.last_filter_form() == form
    assert got[0][:, 2].tobytes() == xs[0][:, 2].tobytes() and got[1][:, 1].tobytes() == xs[1][:, 1].tobytes()
    assert np.isnan(got[0][k:, 0]).all()
    if form == 1:
        for s in range(n):
            assert same_but_for_nan_bits(got[s], want[s]), s
        check_records(bank, want, [total] * n, 1, "nan")
    else:
        for s in range(n):
            for cc in range(ch):
                if foc[s][cc] == FILTER_BYPASS:
                    continue
                stop = k if (s, cc) == (0, 0) else total
                err = np.abs(got[s][:stop, cc].astype(np.float64) - want[s][:stop, cc]).max()
                assert err <= bar_of(xs[s][:stop, cc], want[s][:stop, cc]), (s, cc, err)
            rec, ref_rec = bank.fetch_filtered(s), fr.record(want[s], total, 2, FLOOR)
            check_record(rec, ref_rec, ("nan, form 2", s))
            assert int(rec["samples_nonfinite"]) > 0 and int(rec["samples_over"]) > 0
    # the poisoned channel stays poisoned in the next call, until its stream is reset
    again = run_call(torch_dev, bank, [x[:40] for x in xs], ch)
    assert np.isnan(again[0][:, 0]).all() and np.isfinite(again[1][:, 0]).all()
    bank.reset_filter([1, 0])
    again = run_call(torch_dev, bank, [x[:40] for x in xs], ch)
    assert np.isfinite(again[0][:, 0]).all()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(torch_dev, omx):
    ch, fs, n, frames = 2, 48000.0, 2, 300
    bank = new_bank(omx, n, ch, fs)
    host = noise(5, n * frames, ch).reshape(n, frames, ch)
    d_in = torch_dev.from_numpy(host).cuda()
    d_out = torch_dev.from_numpy(np.full(host.shape, POISON, np.float32)).cuda()
    st = stream_of(torch_dev)

    def refused(status, call, *args, **kw):
        with pytest.raises(OmxError) as e:
            call(*args, **kw)
        assert e.value.status == status and "program loudness filter" in str(e.value), e.value

    # before configure
    refused(-3, bank.filter, d_in.data_ptr(), d_out.data_ptr(), frames, stream=st)
    refused(-3, bank.reset_filter)
    refused(-3, bank.fetch_filtered, 0)
    # configure
    good = filter_table_for(fs)
    refused(-3, bank.configure_filter, good, 0, fs)
    refused(-3, bank.configure_filter, good, 9, fs)
    refused(-3, bank.configure_filter, good, ch, 0.0)
    refused(-3, bank.configure_filter, good, ch, math.nan)
    refused(-3, bank.configure_filter, [], ch, fs)
    refused(-3, bank.configure_filter, [good[0]] * 257, ch, fs)
    refused(-3, bank.configure_filter, good, ch, fs, [[0, 3], [0, 0]])          # an index beyond the table
    refused(-3, bank.configure_filter, [[(1.0, math.nan, 0.0, 0.0, 0.0)]], ch, fs)
    refused(-3, bank.configure_filter, [[(1.0, 0.0, 0.0, 0.0, math.inf)]], ch, fs)
    refused(-2, bank.configure_filter, [good[0], [(1.0, 0.0, 0.0, 0.0, 1.0)]], ch, fs)  # on the unit circle
    refused(-2, bank.configure_filter, [[(1.0, 0.0, 0.0, -2.5, 1.2)]], ch, fs)
    refused(-3, bank.filter, d_in.data_ptr(), d_out.data_ptr(), frames, stream=st)  # still not configured
    bank.configure_filter(good, ch, fs, [[0, 1], [2, FILTER_BYPASS]])
    bank.set_filter_form(1)
    ptr = bank.filter(d_in.data_ptr(), d_out.data_ptr(), frames, frames=[frames, 7], stream=st)
    torch_dev.cuda.synchronize()
    records, out_before = device_bytes(ptr, n * SIZE), d_out.cpu().numpy().tobytes()
    assert records == b"".join(bank.fetch_filtered(s).tobytes() for s in range(n))
    # a stream holds state
    refused(-3, bank.configure_filter, good, ch, fs)
    # the calls
    refused(-3, bank.filter, d_in.data_ptr(), d_in.data_ptr() + 4, frames, stream=st)                  # partial overlap
    refused(-3, bank.filter, d_in.data_ptr(), d_in.data_ptr() + n * frames * ch * 4 - 4, frames, stream=st)
    refused(-3, bank.filter, d_in.data_ptr(), d_out.data_ptr(), frames, frames=[frames + 1, 0], stream=st)
    refused(-3, bank.filter, d_in.data_ptr(), d_out.data_ptr(), 2 ** 32, frames=[0, 0], stream=st)
    refused(-3, bank.filter, 0, d_out.data_ptr(), frames, stream=st)
    refused(-3, bank.filter, d_in.data_ptr(), 0, frames, stream=st)
    refused(-3, bank.fetch_filtered, n)
    call = omx.fn("program_loudness_bank_filter", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    assert call(bank._h, C.c_void_p(d_in.data_ptr()), frames, None, C.c_void_p(d_out.data_ptr()), None, None) == -3  # null d_filtered
    torch_dev.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == out_before and device_bytes(ptr, n * SIZE) == records
    # the state is as it was too: the next call continues the programme
    _, states = restate(good, [[0, 1], [2, FILTER_BYPASS]], [host[0], host[1, :7]], ch)
    want, _ = restate(good, [[0, 1], [2, FILTER_BYPASS]], [host[0], host[1, :7]], ch, states)
    got = run_call(torch_dev, bank, [host[0], host[1, :7]], ch)
    assert all(got[s].tobytes() == want[s].tobytes() for s in range(n))
    # after a reset of every stream the table may change
    bank.reset_filter()
    bank.configure_filter(good[:1], ch, fs)


# ---------------------------------------------------------------- 6. the chain: inspect -> filter -> inspect
def test_dc_block_clears_the_offset_inspect_flags_and_touches_no_other_record(torch_dev, omx):
    ch, fs, n, frames = 2, 48000.0, 2, 48000
    t = np.arange(frames) / fs
    tone = (0.25 * np.sin(2.0 * np.pi * 1000.0 * t)).astype(np.float32)
    host = np.stack([np.stack([tone + np.float32(0.01), tone - np.float32(0.01)], 1)] * n)
    d_in = torch_dev.from_numpy(host).cuda()
    d_out = torch_dev.zeros_like(d_in)
    st = stream_of(torch_dev)
    bank = new_bank(omx, n, ch, fs)
    bank.set_peaks(True)
    bank.process(d_in.data_ptr(), frames, ch, fs, [1, 2, 0, 0, 0, 0, 0, 0], stream=st)
    rule = InspectRule()
    bank.configure_inspect(rule, ch)
    bank.inspect(d_in.data_ptr(), frames, stream=st)
    for s in range(n):
        assert int(inspect_summarize(omx, rule, bank.fetch_inspected(s))["verdict"]) & INSPECT_DC
    bank.plan_gains(GainRule(), stream=st)

    def other_records():
        torch_dev.cuda.synchronize()
        return (device_bytes(bank.results(st), n * C.sizeof(CProgramLoudnessRecord)), device_bytes(bank.peaks(st), n * C.sizeof(CProgramPeakRecord)),
                bank.fetch_gains().tobytes(), b"".join(bank.fetch_inspected(s).tobytes() for s in range(n)))

    before = other_records()
    bank.configure_filter([fr.design(fr.DC_BLOCK, fs, 5.0)], ch, fs)
    for form in (1, 2):
        bank.reset_filter()
        bank.set_filter_form(form)
        bank.filter(d_in.data_ptr(), d_out.data_ptr(), frames, stream=st)
        assert other_records() == before, form
        bank.reset_inspect()
        behind = frames // 2  # 0.5 s = 15 time constants of the 5 Hz blocker
        bank.inspect(d_out.data_ptr() + behind * ch * 4, frames, frames=[frames - behind] * n, stream=st)
        for s in range(n):
            summary = inspect_summarize(omx, rule, bank.fetch_inspected(s))
            assert not int(summary["verdict"]) & INSPECT_DC, (form, s, summary["dc_offset"])
            assert np.abs(summary["dc_offset"][:ch]).max() < 1e-4
        bank.reset_inspect()
        bank.inspect(d_in.data_ptr(), frames, stream=st)  # (the inspector's records as they were)


# ---------------------------------------------------------------- 7. the C99 demo
def test_c99_demo_takes_the_offset_out(torch_dev, omx, tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], words[1::2]))
    fs, frames, first = 48000.0, 96000, 50001
    t = np.arange(frames) / fs
    v = (0.25 + 0.25 * np.sin(2.0 * np.pi * 1000.0 * t)).astype(np.float32)
    want, _ = restate([fr.design(fr.HIGHPASS, fs, 20.0, order=4)], None, [np.stack([v, -v], 1)], 2)
    rec = fr.record(want[0][first:], frames, 2, FLOOR)
    assert (int(out["frames"]), int(out["frames_total"]), int(out["samples_over"]), int(out["samples_nonfinite"])) == (frames - first, frames, 0, 0)
    assert int(out["form"]) == int(out["last_form"]) and int(out["form"]) in (1, 2)
    assert abs(float(out["peak"]) - float(rec["out_sample_peak"])) <= 1e-6 and abs(float(out["peak_db"]) - float(rec["out_sample_peak_db"])) <= 1e-4
    assert abs(float(out["offset_left"])) < 1e-4
    assert abs(float(out["offset_left"]) - float(want[0][frames - 4800:, 0].astype(np.float64).mean())) <= 1e-6

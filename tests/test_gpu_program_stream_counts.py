"""Programme bank stages over the STREAM axis on the GPU (`-m gpu`): stream counts past one wavefront group, past one block of the
begin / finish / plan kernels and past one slab of 65535 streams, where the stage files (test_gpu_program_filter.py and its siblings)
stay within a handful of streams.  Every stream's samples come from one seeded [n][frames][ch] array, so no two streams share data and
a wrong stream index shows.  tests/test_cpu_program_stream_counts.py proves on the restatements alone that the comparisons below reject
swapped, skipped and shifted streams.

Bars: the stage files' own.  Output floats equal the restatement on bytes (NaN as NaN); every record field equal except the dB figure,
within 1e-4 dB; the filter's time-parallel form within 2^-23 x max(peak in, peak out) per stream (bar_of), and there the record is
held to the floats the device wrote (the record is a function of the output, and the output may differ from the restatement's by the
bar).  Outputs are pre-filled with a sentinel: nothing at or beyond a stream's frames changes, d_in keeps its bytes out of place.
The records of a call are read in one device_bytes(ptr, n * SIZE); fetch_* is called on the seam streams only and must give the same
bytes.  No test provokes a fault: every call uses arguments the host accepts and buffers sized for n x capacity."""
import functools

import numpy as np
import pytest

import program_filter_ref as fr
import program_limit_ref as lr
import program_normalize_ref as nr
import program_pcm_ref as pr
import program_peaks_ref as pk
import program_remix_ref as mr
import program_resample_ref as rr
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (APPLY_RECORD_DTYPE, EXPORT_RECORD_DTYPE, FILTER_BYPASS, FILTER_RECORD_DTYPE, LIMIT_RECORD_DTYPE,
                                             REMIX_RECORD_DTYPE, RESAMPLE_RECORD_DTYPE, ExportRule, GainRule, LimitRule, ProgramLoudnessBank,
                                             ResampleRule, filter_plan)
from test_cpu_program_resample import lib_plan
from test_gpu_program_filter import (POISON, check_record, check_time_parallel, filter_table_for, per_channel, rows_of,
                                     same_but_for_nan_bits)
from test_gpu_program_limit import drive, same_floats
from test_gpu_program_limit import gains_on_device as limit_gains_on_device
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_normalize import check_applied, gains_on_device
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
FS = 48000.0
SENTINEL = np.float32(777.25)       # the slab stages' and the limiter's; the filter cases use the filter file's POISON
SENTINEL_BYTE = 0xA5
SLAB = 65535                        # streams of one launch of the slab stages
N_SLAB = SLAB + 64 + 1
SLAB_CAP = 3
SLAB_IDLE = (7, 64, SLAB)
SLAB_SEAMS = (0, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, N_SLAB - 1)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, n, ch=2, fs=FS, seconds=10):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), n, ch, seconds)


def data_of(seed, n, frames, ch, peak=1.0):
    """the one seeded array of a case: f32 [n][frames][ch]"""
    return np.random.default_rng(seed).uniform(-peak, peak, (n, frames, ch)).astype(np.float32)


# ================================================================ the filter: inputs and expectations (numpy only)
def filter_shape(omx, ch):
    """(G streams per wavefront, chunk_frames, tile_frames) of filter_plan"""
    info = filter_plan(omx, ch, FS)
    return int(info["streams_per_wavefront"]), int(info["chunk_frames"]), int(info["tile_frames"])


def group_lengths(G, C, t, group_1_has_frames):
    """case 1: group 0 ragged, group 1 idle (or ragged too), the one stream of group 2 the call's longest"""
    cycle = [1, t - 1, t, t + 1, C - 1, C + 1, 0]
    ragged = [cycle[i % len(cycle)] for i in range(G)]
    return ragged + (ragged if group_1_has_frames else [0] * G) + [2 * C + 5]


def bypass_table(n, ch, G):
    """filter_of_channel [n][ch]: every lane of group 1 on bypass, one channel of every other stream on bypass, the table's three
    filters in turn on the rest.  A mono stream has one lane only, so there every third stream is the one on bypass."""
    foc = per_channel(n, ch) if ch > 1 else [[FILTER_BYPASS if s % 3 == 1 else s % 3] for s in range(n)]
    for s in range(G, 2 * G):
        foc[s] = [FILTER_BYPASS] * ch
    return foc


def streams_of(data, lengths):
    return [data[s, :f].copy() for s, f in enumerate(lengths)]


def restate_many(filters, foc, xs, ch, states=None):
    """test_gpu_program_filter.restate for many streams: fr.run is vectorised over lanes, so the streams of one length run together,
    once per distinct length.  -> (outputs per stream, states f64 [n][4][ch])"""
    n = len(xs)
    outs, sts = [None] * n, np.zeros((n, 4, ch))
    by_length = {}
    for s, x in enumerate(xs):
        by_length.setdefault(len(x), []).append(s)
    for ss in by_length.values():
        coef, count, bypass = fr.lane_table(filters, None if foc is None else [foc[s] for s in ss], len(ss), ch)
        start = None if states is None else np.concatenate([states[s] for s in ss], axis=1)
        o, st = fr.run(np.concatenate([xs[s] for s in ss], axis=1), coef, count, bypass, start)
        for k, s in enumerate(ss):
            outs[s], sts[s] = np.ascontiguousarray(o[:, k * ch:(k + 1) * ch]), st[:, k * ch:(k + 1) * ch]
    return outs, sts


def image_of(wants, before):
    """what a faultless device leaves of `before` [n][cap][ch]: stream s's output in its first frames, the rest untouched"""
    out = before.copy()
    for s, w in enumerate(wants):
        out[s, :len(w)] = w
    return out


def check_filter_untouched(got, before, counts, tag):
    for s, f in enumerate(counts):
        assert got[s, f:].tobytes() == before[s, f:].tobytes(), (tag, "written at or beyond the stream's frames", s, f)


def check_filter_image(got, before, wants, tag):
    """got [n][cap][ch] as the device left it: the restatement's bytes (NaN as NaN) in a stream's frames, `before` behind them"""
    check_filter_untouched(got, before, [len(w) for w in wants], tag)
    for s, w in enumerate(wants):
        assert same_but_for_nan_bits(got[s, :len(w)], w), (tag, "output differs from the restatement", s, len(w))


def check_filter_records(records, outs, totals, form, tag):
    """records: FILTER_RECORD_DTYPE [n]; outs[s]: the floats of stream s's call that the record describes"""
    assert len(records) == len(outs)
    for s, o in enumerate(outs):
        check_record(records[s], fr.record(o, totals[s], form, FLOOR), (tag, s))


FILTERS_4 = [fr.design(fr.HIGHPASS, FS, 20.0, order=4), fr.design(fr.DC_BLOCK, FS, 5.0)]
FOC_4 = [[0, 1], [0, 1]]


def case_4_inputs(C):
    """two stereo streams of 65 C + 3 and 64 C frames, noise at 0.5.  In stream 0 the only samples over full scale (channel 0, through
    the high-pass) and the only sample that is not finite (a NaN on channel 1, through DC_BLOCK: its lane stays NaN from there to the
    stream's end, three frames into item 65) lie in item 64, the last full one."""
    data = data_of(4004, 2, 65 * C + 3, 2, 0.5)
    x0, x1 = data[0].copy(), data[1, :64 * C].copy()
    x0[64 * C + 100:64 * C + 103, 0] = 1.5
    x0[65 * C - 8, 1] = np.nan
    return [x0, x1]


@functools.lru_cache(maxsize=None)
def case_4(C):
    """-> (inputs, the restatement's outputs, its values before they are rounded to f32).  One run of fr.run over the four lanes: a
    frame's output depends on no later frame, so the shorter stream is the head of its zero-padded run."""
    xs = case_4_inputs(C)
    padded = np.concatenate([xs[0], np.concatenate([xs[1], np.zeros((len(xs[0]) - len(xs[1]), 2), np.float32)])], axis=1)
    coef, count, bypass = fr.lane_table(FILTERS_4, FOC_4, 2, 2)
    unrounded = np.zeros(padded.shape)
    out, _ = fr.run(padded, coef, count, bypass, unrounded=unrounded)
    n1 = len(xs[1])
    return xs, [np.ascontiguousarray(out[:, :2]), np.ascontiguousarray(out[:n1, 2:])], [unrounded[:, :2], unrounded[:n1, 2:]]


def record_of_the_first_items(out, items, C, total, form):
    """what a fold that stops after `items` work items would leave: the tallies of the head, the frame counts of the whole"""
    r = fr.record(out[:items * C], total, form, FLOOR)
    r["frames"] = len(out)
    return r


# ================================================================ the slab stages: inputs and expectations (numpy only)
def slab_counts(n=N_SLAB):
    counts = (1 + np.arange(n) % 3).astype(np.uint32)
    counts[list(SLAB_IDLE)] = 0
    return counts


def level_db(peak, floor=FLOOR):
    """power_to_db(peak * peak) in f32, over an array"""
    with np.errstate(all="ignore"):
        p = np.asarray(peak, np.float32) * np.asarray(peak, np.float32)
        db = np.log(np.where(p > 0, p, np.float32(1.0)), dtype=np.float32) * np.float32(4.3429448)
    return np.where(p > 0, np.maximum(db, np.float32(floor)), np.float32(floor)).astype(np.float32)


def tallies(want, counts):
    """(samples over full scale, peak with fmaxf semantics) per stream of want [n][cap] within counts[s] frames"""
    live = np.arange(want.shape[1])[None, :] < counts[:, None]
    with np.errstate(all="ignore"):
        mag = np.where(live & ~np.isnan(want), np.abs(want), np.float32(0.0)).astype(np.float32)
    return (live & (mag > np.float32(1.0))).sum(axis=1), mag.max(axis=1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def check_slab_image(got, want, counts, sentinel, tag):
    """got, want: [n][cap] of one 2- or 4-byte type.  A stream's frames equal the expectation on bits; what lies behind them holds the
    sentinel"""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    live = np.arange(want.shape[1])[None, :] < np.asarray(counts)[:, None]
    bad = live & (bits(got) != bits(want))
    assert not bad.any(), (tag, "output differs from the expectation, first at (stream, frame)", np.argwhere(bad)[:4].tolist())
    wrote = ~live & (bits(got) != bits(np.full((), sentinel, got.dtype)))
    assert not wrote.any(), (tag, "written at or beyond a stream's frames, first at (stream, frame)", np.argwhere(wrote)[:4].tolist())


def check_record_array(got, want, db_fields, tag, bar=BAR):
    """got, want: arrays of one record dtype.  Every field equal on bits except db_fields, which hold `bar` dB"""
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.shape, want.shape)
    for f in got.dtype.names:
        g, w = got[f], want[f]
        if f in db_fields:
            with np.errstate(invalid="ignore"):
                bad = ~((g == w) | (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= bar))
        else:
            bad = np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1) != np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1)
            bad = bad.any(axis=1)
        assert not bad.any(), (tag, f, "differs, first at streams", np.flatnonzero(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


REMIX_MATRIX = np.array([[0.75, -1.5]], np.float32)


def remix_inputs():
    return data_of(6001, N_SLAB, SLAB_CAP, 2)


def remix_expectation(x, counts):
    """-> (want f32 [n][cap], records REMIX_RECORD_DTYPE [n]) of the 2 to 1 remix of x [n][cap][2] under REMIX_MATRIX, all streams at once"""
    want = mr.remix(REMIX_MATRIX, x.reshape(-1, 2)).reshape(len(x), -1)
    over, peak = tallies(want, counts)
    rec = np.zeros(len(x), REMIX_RECORD_DTYPE)
    rec["frames"], rec["samples_over"], rec["out_sample_peak"], rec["out_sample_peak_db"] = counts, over, peak, level_db(peak)
    rec["matrix_index"], rec["terms"] = 0, mr.terms(REMIX_MATRIX)
    return want, rec


# ================================================================ 1. the filter: wavefront groups
def filter_call(torch, bank, xs, ch, in_place):
    """test_gpu_program_filter.run_call, returning what the comparisons need -> (the device's rows [n][cap][ch], the rows beforehand,
    the records of the call in one read)"""
    host, cap = rows_of(xs, ch, 0.375)
    d_in = torch.from_numpy(host).cuda()
    before = host if in_place else np.full(host.shape, POISON, np.float32)
    d_out = d_in if in_place else torch.from_numpy(before).cuda()
    ptr = bank.filter(d_in.data_ptr(), d_out.data_ptr(), cap, frames=[len(x) for x in xs], stream=stream_of(torch))
    torch.cuda.synchronize()
    bank.records_ptr = ptr      # (the bank's one record array: a reset writes into it too)
    if not in_place:
        assert d_in.cpu().numpy().tobytes() == host.tobytes(), "d_in changed"
    records =np.frombuffer(device_bytes(ptr, len(xs) * FILTER_RECORD_DTYPE.itemsize), FILTER_RECORD_DTYPE)
    return d_out.cpu().numpy(), before, records


def check_seams(bank, records, seams):
    for s in seams:
        assert bank.fetch_filtered(s).tobytes() == records[s].tobytes(), ("fetch_filtered differs from the device's record", s)


def frames_of(rows, counts):
    return [rows[s, :f] for s, f in enumerate(counts)]


@pytest.mark.parametrize("ch", [1, 2, 3, 4, 5, 7, 8])
def test_filter_over_three_wavefront_groups(torch_dev, omx, ch):
    G, C, t = filter_shape(omx, ch)
    n = 2 * G + 1
    filters = filter_table_for(FS)
    data, more = data_of(1000 + ch, n, 2 * C + 5, ch, 1.2), data_of(1100 + ch, n, t + 3, ch, 1.2)
    seams = (0, G - 1, G, G + 1, 2 * G - 1, 2 * G)
    figures = []
    for foc in (None, bypass_table(n, ch, G)):
        lengths = group_lengths(G, C, t, foc is not None)
        xs, xs2 = streams_of(data, lengths), streams_of(more, [t + 3] * n)
        want, states = restate_many(filters, foc, xs, ch)
        want2, _ = restate_many(filters, foc, xs2, ch, states)
        totals = [f + t + 3 for f in lengths]
        for form in (1, 2):
            for in_place in (False, True):
                tag = (ch, "bypass table" if foc else "filter 0", form, in_place)
                bank = new_bank(omx, n, ch)
                bank.configure_filter(filters, ch, FS, foc)
                bank.set_filter_form(form)
                got, before, records = filter_call(torch_dev, bank, xs, ch, in_place)
                assert bank.last_filter_form() == form
                check_seams(bank, records, seams)
                got2, before2, records2 = filter_call(torch_dev, bank, xs2, ch, in_place)
                check_seams(bank, records2, seams)
                if form == 1:
                    check_filter_image(got, before, want, tag)
                    check_filter_image(got2, before2, want2, tag + ("second call",))
                    check_filter_records(records, want, lengths, 1, tag)
                    check_filter_records(records2, want2, totals, 1, tag + ("second call",))
                else:
                    check_filter_untouched(got, before, lengths, tag)
                    check_filter_untouched(got2, before2, [t + 3] * n, tag)
                    first, second = frames_of(got, lengths), frames_of(got2, [t + 3] * n)
                    both = [np.concatenate([a, b]) for a, b in zip(first, second)]
                    check_time_parallel(both, [np.concatenate([a, b]) for a, b in zip(want, want2)],
                                        [np.concatenate([a, b]) for a, b in zip(xs, xs2)], tag, figures)
                    check_filter_records(records, first, lengths, 2, tag)
                    check_filter_records(records2, second, totals, 2, tag + ("second call",))
                if foc is not None:      # a lane on bypass keeps its bits in both forms
                    for s in range(n):
                        for c in (c for c in range(ch) if foc[s][c] == FILTER_BYPASS):
                            assert got[s, :lengths[s], c].tobytes() == xs[s][:, c].tobytes(), (tag, s, c)
                            assert got2[s, :t + 3, c].tobytes() == xs2[s][:, c].tobytes(), (tag, s, c)
    print("largest figure:", max(figures))


# ================================================================ 2. the filter: exact fits
@pytest.mark.parametrize("fit", [-1, 0, 1])
def test_filter_streams_that_fill_a_wavefront_exactly(torch_dev, omx, fit):
    ch = 2
    G, _, t = filter_shape(omx, ch)
    n = G + fit
    filters = filter_table_for(FS)
    xs = streams_of(data_of(2000 + fit, n, t + 1, ch, 1.2), [t + 1] * n)
    want, _ = restate_many(filters, None, xs, ch)
    bank = new_bank(omx, n, ch)
    bank.configure_filter(filters, ch, FS)
    bank.set_filter_form(1)
    got, before, records = filter_call(torch_dev, bank, xs, ch, False)
    assert bank.last_filter_form() == 1
    check_filter_image(got, before, want, ("exact fit", n))
    check_filter_records(records, want, [t + 1] * n, 1, ("exact fit", n))
    check_seams(bank, records, (0, n - 2, n - 1))


# ================================================================ 3. the filter: reset over many streams
def test_filter_reset_of_every_third_stream(torch_dev, omx):
    ch = 3
    G, _, t = filter_shape(omx, ch)
    n, frames = 2 * G + 1, t + 8
    filters = filter_table_for(FS)
    xs, xs2 = streams_of(data_of(3000, n, frames, ch, 1.2), [frames] * n), streams_of(data_of(3001, n, frames, ch, 1.2), [frames] * n)
    bank = new_bank(omx, n, ch)
    bank.configure_filter(filters, ch, FS)
    bank.set_filter_form(1)
    want, states = restate_many(filters, None, xs, ch)
    got, before, records = filter_call(torch_dev, bank, xs, ch, False)
    check_filter_image(got, before, want, "before the reset")
    check_filter_records(records, want, [frames] * n, 1, "before the reset")
    marked = [1 if s % 3 == 0 else 0 for s in range(n)]
    bank.reset_filter(marked)
    torch_dev.cuda.synchronize()
    fresh = fr.record(np.zeros((0, ch), np.float32), 0, 0, FLOOR)
    after = np.frombuffer(device_bytes(bank.records_ptr, n * FILTER_RECORD_DTYPE.itemsize), FILTER_RECORD_DTYPE)
    for s in range(n):
        assert after[s].tobytes() == (fresh if marked[s] else records[s]).tobytes(), ("reset" if marked[s] else "not reset", s, after[s])
    check_seams(bank, after, (0, 1, G - 1, G, G + 1, 2 * G))
    for s in range(n):
        if marked[s]:
            states[s] = 0.0
    want2, _ = restate_many(filters, None, xs2, ch, states)
    got2, before2, records2 = filter_call(torch_dev, bank, xs2, ch, False)
    check_filter_image(got2, before2, want2, "after the reset")
    check_filter_records(records2, want2, [frames if marked[s] else 2 * frames for s in range(n)], 1, "after the reset")
    from_zero, _ = restate_many(filters, None, xs2, ch)
    assert all((want2[s].tobytes() == from_zero[s].tobytes()) == bool(marked[s]) for s in range(n)), "the carried state does not show"


# ================================================================ 4. the filter: more than 64 work items
def assert_case_4_placement(xs, want, C):
    """on the restatement: stream 0's samples over full scale, its input that is not finite and its output peak lie in item 64, so a
    record folded from items 0 .. 63 is wrong in all three fields"""
    lo, hi = 64 * C, 65 * C
    assert len(xs[0]) == 65 * C + 3 and len(xs[1]) == 64 * C
    with np.errstate(invalid="ignore"):
        over = np.argwhere(np.abs(want[0]) > np.float32(1.0))
    assert len(over) and lo <= over[:, 0].min() and over[:, 0].max() < hi
    bad = np.argwhere(~np.isfinite(xs[0]))
    assert len(bad) == 1 and lo <= bad[0, 0] < hi and FOC_4[0][bad[0, 1]] != FILTER_BYPASS
    assert lo <= int(np.argmax(np.nanmax(np.abs(want[0]), axis=1))) < hi      # (channel 0 stays finite: no frame is all NaN)
    assert np.isfinite(xs[1]).all() and np.isfinite(want[1]).all()
    whole, head = fr.record(want[0], len(xs[0]), 2, FLOOR), record_of_the_first_items(want[0], 64, C, len(xs[0]), 2)
    for f in ("samples_over", "samples_nonfinite", "out_sample_peak"):
        assert whole[f] != head[f], (f, whole[f], head[f])
    assert int(head["samples_over"]) == 0 and int(head["samples_nonfinite"]) == 0


def test_filter_with_more_work_items_than_a_wavefront_has_lanes(torch_dev, omx):
    ch = 2
    _, C, _ = filter_shape(omx, ch)
    xs, want, _ = case_4(C)
    assert_case_4_placement(xs, want, C)
    lengths = [len(x) for x in xs]
    bank = new_bank(omx, 2, ch)
    bank.configure_filter(FILTERS_4, ch, FS, FOC_4)
    bank.set_filter_form(2)
    got, before, records = filter_call(torch_dev, bank, xs, ch, False)
    assert bank.last_filter_form() == 2
    check_filter_untouched(got, before, lengths, "65 items")
    outs, figures = frames_of(got, lengths), []
    check_time_parallel(outs, want, xs, "65 items", figures)
    print("largest figure:", max(figures))
    check_filter_records(records, outs, lengths, 2, "65 items, form 2")
    for s in range(2):      # the counts do not hang on a rounding: the restatement's own
        ref = fr.record(want[s], lengths[s], 2, FLOOR)
        assert (int(records[s]["samples_over"]), int(records[s]["samples_nonfinite"])) == (int(ref["samples_over"]), int(ref["samples_nonfinite"]))
    check_seams(bank, records, (0, 1))
    bank.reset_filter()
    bank.set_filter_form(1)
    got, before, records = filter_call(torch_dev, bank, xs, ch, False)
    assert bank.last_filter_form() == 1
    check_filter_image(got, before, want, "65 items, form 1")
    check_filter_records(records, want, lengths, 1, "65 items, form 1")


# ================================================================ 5. the filter: form chosen by stream count
def test_filter_form_by_stream_count(torch_dev, omx):
    ch = 8
    G, C, _ = filter_shape(omx, ch)
    shift = (64 // G).bit_length() - 1
    # program_filter.cpp: waves = (n_streams << slot_shift) / 64 + 1; time-parallel by shape only while waves * 4 < 2048
    many = next(n for n in range(1, 1 << 20) if ((n << shift) // 64 + 1) * 4 >= 2048)
    assert (((many - 1) << shift) // 64 + 1) * 4 < 2048 and 4000 < many < 4200, many
    for n, form in ((many, 1), (2, 2)):
        bank = new_bank(omx, n, ch)
        bank.configure_filter(filter_table_for(FS), ch, FS)
        bank.set_filter_form(0)
        d = torch_dev.zeros((n, 4 * C, ch), dtype=torch_dev.float32, device="cuda")
        ptr = bank.filter(d.data_ptr(), d.data_ptr(), 4 * C, stream=stream_of(torch_dev))
        torch_dev.cuda.synchronize()
        assert bank.last_filter_form() == form, (n, bank.last_filter_form())
        assert not bool(d.any()), "zeros in, something else out"
        records = np.frombuffer(device_bytes(ptr, n * FILTER_RECORD_DTYPE.itemsize), FILTER_RECORD_DTYPE)
        want = np.repeat(fr.record(np.zeros((4 * C, ch), np.float32), 4 * C, form, FLOOR).reshape(1), n)
        check_record_array(records, want, ("out_sample_peak_db",), ("form by stream count", n))
        del d


# ================================================================ 6. the slab stages
def slab_rows(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def test_remix_over_more_streams_than_one_launch_holds(torch_dev, omx):
    counts, x = slab_counts(), remix_inputs()
    want, want_rec = remix_expectation(x, counts)
    bank = new_bank(omx, N_SLAB, 2)
    bank.configure_remix(REMIX_MATRIX, 2, 1)
    d_in = slab_rows(torch_dev, x)
    d_out = torch_dev.full((N_SLAB, SLAB_CAP, 1), float(SENTINEL), dtype=torch_dev.float32, device="cuda")
    ptr = bank.remix(d_in.data_ptr(), d_out.data_ptr(), SLAB_CAP, frames=counts, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == x.tobytes(), "d_in changed"
    got = d_out.cpu().numpy().reshape(N_SLAB, SLAB_CAP)
    check_slab_image(got, want, counts, SENTINEL, "remix")
    rec = np.frombuffer(device_bytes(ptr, N_SLAB * REMIX_RECORD_DTYPE.itemsize), REMIX_RECORD_DTYPE)
    check_record_array(rec, want_rec, ("out_sample_peak_db",), "remix")
    assert want_rec["samples_over"].sum() > 0
    for s in SLAB_SEAMS:
        f = int(counts[s])
        assert bank.fetch_remixed(s).tobytes() == rec[s].tobytes()
        own = mr.remix(REMIX_MATRIX, x[s, :f])
        assert got[s, :f].tobytes() == own.tobytes(), ("remix, the stage's restatement", s)
        mr.check_record(rec[s], mr.record(own, REMIX_MATRIX, 0, FLOOR), ("remix", s), BAR)


def test_apply_gains_over_more_streams_than_one_launch_holds(torch_dev, omx):
    counts = slab_counts()
    x = data_of(6002, N_SLAB, SLAB_CAP, 1)
    factors = (np.float32(0.5) + np.arange(N_SLAB, dtype=np.float32) * np.float32(2.0 ** -15)).astype(np.float32)      # every stream its own
    assert len(np.unique(factors)) == N_SLAB
    want = (x[:, :, 0] * factors[:, None]).astype(np.float32)
    over, peak = tallies(want, counts)
    want_rec = np.zeros(N_SLAB, APPLY_RECORD_DTYPE)
    want_rec["frames"], want_rec["samples_over"], want_rec["gain"], want_rec["out_sample_peak"] = counts, over, factors, peak
    want_rec["out_sample_peak_db"], want_rec["gain_index"] = level_db(peak), np.arange(N_SLAB)
    d_gains, _ = gains_on_device(torch_dev, factors)
    bank = new_bank(omx, N_SLAB, 1)
    d_in = slab_rows(torch_dev, x)
    d_out = torch_dev.full((N_SLAB, SLAB_CAP, 1), float(SENTINEL), dtype=torch_dev.float32, device="cuda")
    ptr = bank.apply_gains(d_in.data_ptr(), d_out.data_ptr(), SLAB_CAP, 1, d_gains.data_ptr(), N_SLAB, frames=counts, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == x.tobytes(), "d_in changed"
    got = d_out.cpu().numpy().reshape(N_SLAB, SLAB_CAP)
    check_slab_image(got, want, counts, SENTINEL, "apply_gains")
    rec = np.frombuffer(device_bytes(ptr, N_SLAB * APPLY_RECORD_DTYPE.itemsize), APPLY_RECORD_DTYPE)
    check_record_array(rec, want_rec, ("out_sample_peak_db",), "apply_gains")
    assert over.sum() > 0
    for s in SLAB_SEAMS:
        f = int(counts[s])
        assert bank.fetch_applied(s).tobytes() == rec[s].tobytes()
        own = check_applied(bank, s, x[s, :f], factors[s], s, "apply_gains, the stage's restatement")
        assert got[s, :f].tobytes() == own[:, 0].tobytes(), s


def test_import_pcm_over_more_streams_than_one_launch_holds(torch_dev, omx):
    counts = slab_counts()
    pcm = np.random.default_rng(6003).integers(-2 ** 15, 2 ** 15, (N_SLAB, SLAB_CAP), dtype=np.int64).astype("<i2")
    want = (pcm.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)
    raw = np.concatenate([pcm.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])
    bank = new_bank(omx, N_SLAB, 1)
    d_in = slab_rows(torch_dev, raw)
    d_out = torch_dev.full((N_SLAB, SLAB_CAP, 1), float(SENTINEL), dtype=torch_dev.float32, device="cuda")
    assert bank.import_pcm(d_in.data_ptr(), pr.S16, d_out.data_ptr(), SLAB_CAP, 1, frames=counts, stream=stream_of(torch_dev)) == 1
    torch_dev.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == raw.tobytes(), "d_in changed"
    got = d_out.cpu().numpy().reshape(N_SLAB, SLAB_CAP)
    check_slab_image(got, want, counts, SENTINEL, "import_pcm")
    for s in SLAB_SEAMS:
        f = int(counts[s])
        assert got[s, :f].tobytes() == pr.import_pcm(pcm[s, :f].tobytes(), pr.S16, 1).tobytes(), ("import_pcm, the stage's restatement", s)


def export_dither(seed, n, frames):
    """pr.dither for channel 0 of frames 0 .. frames - 1 of the streams 0 .. n - 1 at once: f64 [n][frames], in LSB"""
    with np.errstate(over="ignore"):
        key = pr.mix(np.uint64(seed) + pr.GOLDEN * (np.arange(n, dtype=np.uint64) + np.uint64(1)))
        at = np.arange(frames, dtype=np.uint64) * np.uint64(8)
        h = pr.mix((key[:, None] + pr.GOLDEN * at[None, :]).reshape(-1)).reshape(n, frames)
    a = (h & np.uint64(0xFFFFFF)).astype(np.int64)
    b = ((h >> np.uint64(24)) & np.uint64(0xFFFFFF)).astype(np.int64)
    return (a - b).astype(np.float64) * 2.0 ** -24


def test_export_pcm_over_more_streams_than_one_launch_holds(torch_dev, omx):
    counts = slab_counts()
    rule = (pr.S16, pr.TPDF, 0xC0FFEE)
    x = data_of(6004, N_SLAB, SLAB_CAP, 1, 1.2)
    d = export_dither(rule[2], N_SLAB, SLAB_CAP)
    for s in (0, SLAB, N_SLAB - 1):      # the vectorised dither is the restatement's
        assert d[s].tobytes() == pr.dither(rule[2], s, np.arange(SLAB_CAP), 0).tobytes()
    y, clipped, nan, _ = pr.quantise(x[:, :, 0], d, pr.S16)
    live = np.arange(SLAB_CAP)[None, :] < counts[:, None]
    want_rec = np.zeros(N_SLAB, EXPORT_RECORD_DTYPE)
    want_rec["frames_out"] = want_rec["frames_written"] = counts
    want_rec["samples_clipped"], want_rec["samples_nan"] = (clipped & live).sum(axis=1), (nan & live).sum(axis=1)
    want_rec["out_peak"] = np.where(live, np.abs(y), 0).max(axis=1)
    want_rec["out_peak_db"] = level_db((want_rec["out_peak"].astype(np.float64) / 2.0 ** 15).astype(np.float32))
    want_rec["format"], want_rec["dither"] = rule[0], rule[1]
    bank = new_bank(omx, N_SLAB, 1)
    bank.configure_export(ExportRule(*rule), 1)
    d_in = slab_rows(torch_dev, x)
    d_out = torch_dev.full((N_SLAB * SLAB_CAP * 2 + 16,), SENTINEL_BYTE, dtype=torch_dev.uint8, device="cuda")
    ptr = bank.export_pcm(d_in.data_ptr(), d_out.data_ptr(), SLAB_CAP, frames=counts, stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == x.tobytes(), "d_in changed"
    out = d_out.cpu().numpy()
    assert (out[N_SLAB * SLAB_CAP * 2:] == SENTINEL_BYTE).all()
    got = out[:N_SLAB * SLAB_CAP * 2].view("<i2").reshape(N_SLAB, SLAB_CAP)
    check_slab_image(got, y.astype("<i2"), counts, np.uint16(0xA5A5).view(np.int16), "export_pcm")
    rec = np.frombuffer(device_bytes(ptr, N_SLAB * EXPORT_RECORD_DTYPE.itemsize), EXPORT_RECORD_DTYPE)
    check_record_array(rec, want_rec, ("out_peak_db",), "export_pcm")
    assert want_rec["samples_clipped"].sum() > 0
    for s in SLAB_SEAMS:
        f = int(counts[s])
        assert bank.fetch_exported(s).tobytes() == rec[s].tobytes()
        ex = pr.Exporter(rule, s, FLOOR)
        assert got[s, :f].tobytes() == ex.feed(x[s, :f]), ("export_pcm, the stage's restatement", s)
        pr.check_record(rec[s], ex.record(), ("export_pcm", s))


def test_resample_over_more_streams_than_one_launch_holds(torch_dev, omx):
    """24 kHz to 48 kHz, every stream flushed in the call that brings its frames: 2 f frames out of f in"""
    counts = slab_counts()
    rates = (24000, 48000)
    pl = lib_plan(omx, *rates)
    assert (pl["L"], pl["M"]) == (2, 1)
    out_cap = 2 * SLAB_CAP
    x = data_of(6005, N_SLAB, SLAB_CAP, 1, 1.4)
    want = np.zeros((N_SLAB, out_cap), np.float32)
    for f in (1, 2, 3):      # rr.resample treats channels alike: the streams of one length go through it as channels
        ss = np.flatnonzero(counts == f)
        want[ss, :2 * f] = rr.resample(pl, x[ss, :f, 0].T).T
    emitted = 2 * counts
    over, peak = tallies(want, emitted)
    want_rec = np.zeros(N_SLAB, RESAMPLE_RECORD_DTYPE)
    want_rec["frames_in"], want_rec["frames_out"], want_rec["frames_written"], want_rec["samples_over"] = counts, emitted, emitted, over
    want_rec["out_sample_peak"], want_rec["out_sample_peak_db"] = peak, level_db(peak)
    want_rec["state"] = np.where(counts > 0, rr.FLUSHED, rr.IDLE)
    want_rec["L"], want_rec["M"], want_rec["taps"], want_rec["latency_frames"] = pl["L"], pl["M"], pl["T"], pl["H"]
    bank = new_bank(omx, N_SLAB, 1)
    bank.configure_resampler(ResampleRule(*rates), 1)
    d_in = slab_rows(torch_dev, x)
    d_out = torch_dev.full((N_SLAB, out_cap, 1), float(SENTINEL), dtype=torch_dev.float32, device="cuda")
    ptr = bank.resample(d_in.data_ptr(), SLAB_CAP, d_out.data_ptr(), out_cap, frames=counts, flush_mask=(counts > 0).astype(np.uint8),
                        stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == x.tobytes(), "d_in changed"
    got = d_out.cpu().numpy().reshape(N_SLAB, out_cap)
    check_slab_image(got, want, emitted, SENTINEL, "resample")
    rec = np.frombuffer(device_bytes(ptr, N_SLAB * RESAMPLE_RECORD_DTYPE.itemsize), RESAMPLE_RECORD_DTYPE)
    check_record_array(rec, want_rec, ("out_sample_peak_db",), "resample")
    assert over.sum() > 0
    for s in SLAB_SEAMS:
        f = int(counts[s])
        assert bank.fetch_resampled(s).tobytes() == rec[s].tobytes()
        own = rr.Resampler(pl, 1, FLOOR)
        assert got[s, :2 * f].tobytes() == own.feed(x[s, :f], flush=f > 0).tobytes(), ("resample, the stage's restatement", s)
        rr.check_record(rec[s], own.record(), ("resample", s), BAR)


# ================================================================ 7. the stages on a linear grid
N_GRID = 129


def test_limiter_over_three_blocks_of_streams(torch_dev, omx, oracle):
    """ragged lengths of 0, 1 and one frame either side of the look-ahead and of the level, hold and apply tiles; one call, then the
    flush in a call of its own; every stream under its own gain"""
    ch, rule = 2, (lr.CEILING_DB, 16, 100)
    coeffs = pk.coefficients(oracle)
    LA, apply_frames = lr.latency(rule), lr.APPLY_TILE_FLOATS // ch
    cycle = [0, 1, LA - 1, LA, LA + 1, lr.LEVEL_TILE - 1, lr.LEVEL_TILE, lr.LEVEL_TILE + 1, apply_frames - 1, lr.HOLD_TILE + 1]
    lengths = [cycle[s % len(cycle)] for s in range(N_GRID)]
    data = data_of(7001, N_GRID, max(lengths), ch, 0.9)
    xs = streams_of(data, lengths)
    factors = (np.float32(1.25) + np.arange(N_GRID, dtype=np.float32) / np.float32(128.0)).astype(np.float32)
    d_gains, _ = limit_gains_on_device(torch_dev, factors)
    bank = new_bank(omx, N_GRID, ch)
    bank.configure_limiter(LimitRule(*rule), ch, FS)
    outs, ptr = drive(torch_dev, bank, xs, ch, [lengths], rule, d_gains.data_ptr(), N_GRID)
    rec = np.frombuffer(device_bytes(ptr, N_GRID * LIMIT_RECORD_DTYPE.itemsize), LIMIT_RECORD_DTYPE)
    limited = 0
    for s, x in enumerate(xs):
        lim = lr.Limiter(rule, FS, coeffs, ch, FLOOR)
        first, _ = lim.feed(x, gain=factors[s], gain_index=s)
        rest, _ = lim.feed(np.zeros((0, ch), np.float32), flush=True)
        assert same_floats(outs[s], np.concatenate([first, rest])), ("limiter", s, len(x), "output differs from the restatement")
        lr.check_record(rec[s], lim.record(), ("limiter", s, len(x)))
        limited += int(rec[s]["frames_limited"])
    assert limited > 0
    for s in (0, 63, 64, 65, 127, 128):
        assert bank.fetch_limited(s).tobytes() == rec[s].tobytes()


def test_plan_gains_over_three_blocks_of_streams(torch_dev, omx):
    """half a second of a 1 kHz tone at 8 kHz per stream, 129 levels from -40 to -8 dBFS; the bar of test_gpu_program_normalize.py:
    the restatement fed the bank's own fetched records, every field equal bits, `gain` within 1 f32 ulp"""
    ch, fs, frames = 2, 8000.0, 4000
    level = -40.0 + 0.25 * np.arange(N_GRID)
    tone = np.sin(2.0 * np.pi * 1000.0 * np.arange(frames) / fs)
    host = (10.0 ** (level[:, None, None] / 20.0) * tone[None, :, None] * np.array([1.0, -1.0])[None, None, :]).astype(np.float32)
    d = torch_dev.from_numpy(host).cuda()
    bank = new_bank(omx, N_GRID, ch, fs)
    bank.set_peaks(True)
    bank.process(d.data_ptr(), frames, ch, fs, capi.positions_fallback(ch), stream=stream_of(torch_dev))
    torch_dev.cuda.synchronize()
    sources = [record_array(bank.fetch(s)) for s in range(N_GRID)]
    for rule in (nr.RULE_TARGET, nr.RULE_CEILING):
        ptr = bank.plan_gains(GainRule(*rule), stream=stream_of(torch_dev))
        got = bank.fetch_gains()
        assert len(got) == N_GRID and device_bytes(ptr, N_GRID * 32) == got.tobytes()
        for s, src in enumerate(sources):
            nr.check_record(got[s], nr.gain(rule, src["integrated_lufs"], src["gating_above_relative"], src["max_true_peak_db"], FLOOR), (rule, s))
        assert (np.diff(got["gain_db"]) < 0).all(), "129 levels, and the gains do not fall from stream to stream"
        assert (got["limited_by"] == (nr.BY_TARGET if rule is nr.RULE_TARGET else nr.BY_PEAK)).all() and (got["peak_known"] == 1).all()

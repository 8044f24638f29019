"""The expectations of tests/test_gpu_program_stream_counts.py without a device.

a. The model of the filter's time-parallel schedule (program_filter_ref.run_time_parallel) on that file's input of 65 work items: before
   its output is rounded to f32 it stays within a quarter of the form's bar 2^-23 x max(peak in, peak out), as
   test_cpu_program_filter.py asserts for its own lengths; so the bar holds on the device for a reason, not by luck.
b. The comparisons discriminate.  The restatement's outputs and records of the GPU file's inputs, put where a faultless device would
   put them, pass the GPU file's own comparison helpers; with two streams swapped, a wavefront group left at the sentinel, the streams
   from 65535 on shifted by one, or a record folded from the first 64 work items only, the same helpers reject them."""
import numpy as np
import pytest

import program_filter_ref as fr
from test_gpu_program_filter import POISON, bar_of, filter_table_for, restate, rows_of
from test_gpu_program_loudness import FLOOR
from test_gpu_program_stream_counts import (FILTERS_4, FOC_4, N_SLAB, SENTINEL, SLAB, assert_case_4_placement, bypass_table, case_4,
                                            check_filter_image, check_filter_records, check_record_array, check_slab_image, data_of,
                                            filter_shape, group_lengths, image_of, record_of_the_first_items, remix_expectation, remix_inputs,
                                            restate_many, slab_counts, streams_of)

FS = 48000.0


# ---------------------------------------------------------------- a. the model at 65 work items
def test_model_of_the_time_parallel_schedule_holds_a_quarter_of_the_bar_at_65_items(omx):
    _, C, _ = filter_shape(omx, 2)
    assert C == fr.CHUNK_FRAMES
    xs, want, unrounded = case_4(C)
    assert_case_4_placement(xs, want, C)
    frames = [len(x) for x in xs]
    pad = np.zeros((frames[0] - frames[1], 2), np.float32)
    largest = 0.0
    for c, sections in enumerate(FILTERS_4):      # FOC_4: channel c of both streams runs filter c
        assert fr.time_parallel_ok(sections), (c, fr.predicted_start_error(sections))
        x = np.stack([xs[0][:, c], np.concatenate([xs[1], pad])[:, c]], axis=1)
        u_tp = np.zeros(x.shape)
        tp, _ = fr.run_time_parallel(x, sections, unrounded=u_tp)
        for s in range(2):      # (the shorter stream is the head of its zero-padded run: its items start from the same states)
            f = frames[s]
            ref, u_ref, got, u_got, xin = want[s][:, c], unrounded[s][:, c], tp[:f, s], u_tp[:f, s], x[:f, s]
            finite = np.isfinite(ref)
            assert (np.isfinite(got) == finite).all() and (np.isfinite(u_got) == np.isfinite(u_ref)).all() and finite.any()
            bar = bar_of(xin[np.isfinite(xin)], ref[finite])
            before = float(np.abs(u_got - u_ref)[np.isfinite(u_ref)].max())
            after = float(np.abs(got.astype(np.float64) - ref)[finite].max())
            largest = max(largest, before / bar)
            print(f"filter {c} stream {s}: model before rounding {before / bar:.3e} of the bar, after {after / bar:.3e}")
            assert before <= bar / 4.0 and after <= bar, (c, s, before, after, bar)
    print("largest figure before rounding:", largest)


# ---------------------------------------------------------------- b. the comparisons reject what a wrong stream index would leave
def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def records_of(outs, totals, form):
    return np.concatenate([fr.record(o, f, form, FLOOR).reshape(1) for o, f in zip(outs, totals)])


@pytest.mark.parametrize("ch", [3, 5])
def test_filter_comparisons_reject_swapped_and_skipped_streams(omx, ch):
    G, C, t = filter_shape(omx, ch)
    n = 2 * G + 1
    filters = filter_table_for(FS)
    data = data_of(1000 + ch, n, 2 * C + 5, ch, 1.2)
    for foc in (None, bypass_table(n, ch, G)):
        lengths = group_lengths(G, C, t, foc is not None)
        xs = streams_of(data, lengths)
        want, states = restate_many(filters, foc, xs, ch)
        for s in (0, G - 1, G + 4, 2 * G):      # the streams of one length run together: the same bytes as one at a time
            one, st = restate(filters, None if foc is None else [foc[s]], [xs[s]], ch)
            assert one[0].tobytes() == want[s].tobytes() and np.asarray(st[0]).tobytes() == states[s].tobytes(), s
        host, _ = rows_of(xs, ch, 0.375)
        for before in (np.full(host.shape, POISON, np.float32), host):      # out of place, in place
            good = image_of(want, before)
            records = records_of(want, lengths, 1)
            check_filter_image(good, before, want, "as it should be")
            check_filter_records(records, want, lengths, 1, "as it should be")
            # two streams of different groups swapped: of different lengths, and (where group 1 has frames) of the same length
            pairs = [(1, 2 * G)] + ([(4, G + 4), (5, G + 5)] if foc is not None else [(4, G + 4)])
            for a, b in pairs:
                bad, bad_records = good.copy(), records.copy()
                bad[[a, b]], bad_records[[a, b]] = good[[b, a]], records[[b, a]]
                rejected(check_filter_image, bad, before, want, "swapped")
                rejected(check_filter_records, bad_records, want, lengths, 1, "swapped")
            # one group's rows left as they were
            for group in (0, 1, 2):
                if group == 1 and foc is None:
                    continue      # (idle there: nothing to leave out)
                bad, bad_records = good.copy(), records.copy()
                bad[group * G:(group + 1) * G] = before[group * G:(group + 1) * G]
                bad_records[group * G:(group + 1) * G] = fr.record(np.zeros((0, ch), np.float32), 0, 0, FLOOR)
                rejected(check_filter_records, bad_records, want, lengths, 1, "a group skipped")
                if not (before is host and foc is not None and group == 1):      # (in place and all on bypass: the input's rows either way)
                    rejected(check_filter_image, bad, before, want, "a group skipped")


def test_filter_record_of_the_first_64_items_is_rejected(omx):
    _, C, _ = filter_shape(omx, 2)
    xs, want, _ = case_4(C)
    lengths = [len(x) for x in xs]
    for form in (1, 2):
        good = records_of(want, lengths, form)
        check_filter_records(good, want, lengths, form, "as it should be")
        bad = good.copy()
        bad[0] = record_of_the_first_items(want[0], 64, C, lengths[0], form)
        assert all(bad[0][f] != good[0][f] for f in ("samples_over", "samples_nonfinite", "out_sample_peak"))
        rejected(check_filter_records, bad, want, lengths, form, "folded from 64 items")
        for f in ("samples_over", "samples_nonfinite", "out_sample_peak"):      # each field alone is enough
            one = good.copy()
            one[0][f] = bad[0][f]
            rejected(check_filter_records, one, want, lengths, form, f)
    assert FOC_4 == [[0, 1], [0, 1]]


def test_slab_comparisons_reject_shifted_and_skipped_streams():
    counts, x = slab_counts(), remix_inputs()
    want, records = remix_expectation(x, counts)
    live = np.arange(want.shape[1])[None, :] < counts[:, None]
    good = np.where(live, want, SENTINEL).astype(np.float32)
    check_slab_image(good, want, counts, SENTINEL, "as it should be")
    check_record_array(records, records.copy(), ("out_sample_peak_db",), "as it should be")
    # the streams at and behind 65535 shifted by one stream
    bad, bad_records = good.copy(), records.copy()
    bad[SLAB:], bad_records[SLAB:] = good[SLAB - 1:-1], records[SLAB - 1:-1]
    rejected(check_slab_image, bad, want, counts, SENTINEL, "shifted")
    rejected(check_record_array, bad_records, records, ("out_sample_peak_db",), "shifted")
    # the second slab written over the first (a dropped base): the streams behind 65535 stay at the sentinel
    bad, bad_records = good.copy(), records.copy()
    bad[:N_SLAB - SLAB], bad[SLAB:] = good[SLAB:], SENTINEL
    bad_records[:N_SLAB - SLAB], bad_records[SLAB:] = records[SLAB:], 0
    rejected(check_slab_image, bad, want, counts, SENTINEL, "base dropped")
    rejected(check_record_array, bad_records, records, ("out_sample_peak_db",), "base dropped")
    # one stream alone
    for s in (SLAB - 1, SLAB + 1, N_SLAB - 1):
        bad = good.copy()
        bad[s] = good[s - 3]      # (the same count of frames, another stream's floats)
        rejected(check_slab_image, bad, want, counts, SENTINEL, s)
    # the dB figure holds its bar and no more
    near, far = records.copy(), records.copy()
    near["out_sample_peak_db"][5] += np.float32(5e-5)
    far["out_sample_peak_db"][5] += np.float32(1e-3)
    check_record_array(near, records, ("out_sample_peak_db",), "within the bar")
    rejected(check_record_array, far, records, ("out_sample_peak_db",), "beyond the bar")

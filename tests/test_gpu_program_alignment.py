"""Programme bank stages fed buffers at every 4-byte alignment on the GPU (`-m gpu`).  The stage files pass pointers that the allocator
made, 256-byte aligned, so a row base leaves a 16-byte boundary only through stream * capacity * channels; a host that cuts calls out
of a ring buffer hands the bank any float boundary.  Here every f32 pointer of every stage sits 0, 1, 2 and 3 floats behind a 16-byte
boundary (the integer PCM buffers 0, 4, 8 and 12 bytes), input against output in all 16 pairs, at channel counts where only the base
offset moves a row (4 and 8) as well.  tests/test_cpu_program_alignment.py builds the cases (case_of), proves the coverage conditions on
them and proves that check_image rejects a missing, a stray and a shifted float.

Bars: the stage files' own, none new.  Output floats equal the stage's restatement on bytes (a NaN where it has a NaN, for the stages
whose files say so); every record field equal except the dB figures, within the family's 1e-4 dB (BAR); the filter's time-parallel form
within bar_of per stream, its records held to the floats the device wrote.  The records of a pair have the bytes of the records of pair
(0, 0): no field of any stage's record depends on an address.  Nothing else is written: every output store holds a sentinel beforehand,
8 floats longer than the rows, and the floats in front of d_out, behind the last row and in a row at or beyond the stream's frames
keep it; out of place the input store keeps all its bytes, pad floats included.
A carrying stage takes every stream in two calls cut at t + 1 frames, the second at other offsets, then the flush in a call of its
own at a third pair: the concatenated output is the restatement's one-call output.
No test provokes a fault: every call uses pointers and sizes the host accepts, and every store lies inside an allocation."""
import numpy as np
import pytest

import program_convolve_ref as cr
import program_edit_ref as er
import program_filter_ref as fr
import program_limit_ref as lr
import program_mix_ref as xr
import program_pcm_ref as pr
import program_remix_ref as mr
import program_resample_ref as rr
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (APPLY_RECORD_DTYPE, CONVOLVE_RECORD_DTYPE, DYNAMICS_RECORD_DTYPE, EDIT_RECORD_DTYPE, EXPORT_RECORD_DTYPE,
                                             FILTER_RECORD_DTYPE, INSPECT_RECORD_DTYPE, LIMIT_RECORD_DTYPE, MIX_RECORD_DTYPE, REMIX_RECORD_DTYPE,
                                             RESAMPLE_RECORD_DTYPE, DynamicsCurve, EditClip, ExportRule, InspectRule, LimitRule, MixSend,
                                             ProgramLoudnessBank, ResampleRule)
from test_cpu_program_alignment import (CHANNELS, FS, LIMIT_RULE, N, OFFSETS, PAIRS, SENTINEL, SENTINEL_BYTE, case_of, check_image, input_fill,
                                        pair_of_call, placed, rows_of, rows_of_image, store_image)
from test_gpu_program_dynamics import check_record as check_dynamics_record
from test_gpu_program_dynamics import same_floats as same_dynamics_floats
from test_gpu_program_filter import check_record as check_filter_record
from test_gpu_program_filter import check_time_parallel
from test_gpu_program_limit import gains_on_device as limit_gains_on_device
from test_gpu_program_limit import same_floats as same_limit_floats
from test_gpu_program_loudness import BAR, FLOOR, torch_dev  # noqa: F401
from test_gpu_program_loudness import check_record as check_loudness_record
from test_gpu_program_normalize import apply_case
from test_gpu_program_peaks import check_peaks
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def new_bank(omx, ch, fs=FS, seconds=10):
    return ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), N, ch, seconds)


def run_calls(torch, case, a_in, a_out, launch, tag, nan_as_nan=True, in_place=False, exact=True, after=None):
    """The calls of a case with d_in a_in floats (or 4 a_in bytes) and d_out a_out floats (4 a_out bytes) behind a 16-byte boundary;
    call k of a carrying stage at pair_of_call(k).  launch(k, call, ai, ao, in_ptr, out_ptr) enqueues the stage's call and returns the
    records' device pointer (and, if it likes, a function to run once the call has finished).  Checks every call's output store with
    check_image and that d_in kept its bytes.  exact False (the filter's time-parallel form): only what must NOT be written is checked
    here.  -> (the last call's records pointer, per stream the device's output of every call)"""
    in_integer, out_integer = case["in_unit"] == 1, case["out_unit"] == 1
    out_rows = case.get("out_row_bytes", case["out_cap"] * case["co"])
    parts, ptr = [[] for _ in range(N)], 0
    for k, call in enumerate(case["calls"]):
        ai, ao = pair_of_call(k, a_in, a_out)
        host = case["blob"] if in_integer else rows_of(call["rows"], case["cap"], case["ci"], 40 + k)
        fill = input_fill(host)
        in_at = 4 * ai if in_integer else ai
        in_image = store_image(host, in_at, fill)
        d_in, in_ptr = placed(torch, host, in_at, fill)
        if in_place:
            assert case["cap"] == case["out_cap"] and case["ci"] == case["co"]
            d_out, out_ptr, ao, out_at, before = d_in, in_ptr, ai, in_at, in_image
        else:
            blank = np.full(N * out_rows, SENTINEL_BYTE, np.uint8) if out_integer else np.full(N * out_rows, SENTINEL, np.float32)
            out_at = 4 * ao if out_integer else ao
            before = store_image(blank, out_at, blank[0])
            d_out, out_ptr = placed(torch, blank, out_at, blank[0])
        done = launch(k, call, ai, ao, in_ptr, out_ptr)
        torch.cuda.synchronize()
        ptr, finish = done if isinstance(done, tuple) else (done, None)
        got = d_out.cpu().numpy()
        if not in_place:
            assert d_in.cpu().numpy().tobytes() == in_image.tobytes(), (tag, k, "the input store changed")
        per_frame = out_rows // case["out_cap"]
        rows = rows_of_image(got, out_at, out_rows, [e * per_frame for e in call["emits"]])
        check_image(got, before, call["wants"] if exact else rows, out_at, out_rows, tag + ("call", k, "at", ai, ao), nan_as_nan)
        for s in range(N):
            parts[s].append(rows[s])
        if finish:
            finish()
        if after:
            after(k, call, rows, ptr)
    return ptr, parts


def whole(parts, ch):
    return [np.concatenate(p).reshape(-1, ch) for p in parts]


def same_records(seen, ptr, size, tag, count=N):
    """the records of this pair have the bytes of the first pair's: no field depends on an address"""
    raw = device_bytes(ptr, count * size)
    seen.setdefault("first", (raw, tag))
    assert raw == seen["first"][0], (tag, "the records differ from those at", seen["first"][1])
    return raw


def last_written(case):
    return case["calls"][-1]["emits"]


# ================================================================ resample
@pytest.mark.parametrize("ch", CHANNELS["resample"])
def test_resample_at_every_alignment(torch_dev, omx, ch):
    """44100 to 48000 and 48000 to 44100.  The output store's form (v4f, v2f, dword) hangs on the base a.out and on channels % 4 / % 2:
    at 4 and 8 channels the dword and v2f stores are reached only here (base 1 or 3, and 2 floats off).  Staging peels
    ps_to_aligned(src) floats in front and up to 3 behind: d_in moves as well"""
    for case in case_of("resample", ch, omx):
        bank = new_bank(omx, ch)
        bank.configure_resampler(ResampleRule(*case["rates"]), ch)
        seen = {}
        for a_in, a_out in PAIRS:
            tag = ("resample", case["rates"], ch, a_in, a_out)
            bank.reset_resampler()

            def launch(k, call, ai, ao, in_ptr, out_ptr):
                return bank.resample(in_ptr, case["cap"], out_ptr, case["out_cap"], frames=[len(r) for r in call["rows"]],
                                     flush_mask=[1] * N if call["flush"] else None, stream=stream_of(torch_dev))

            ptr, parts = run_calls(torch_dev, case, a_in, a_out, launch, tag, nan_as_nan=False)
            for s, got in enumerate(whole(parts, ch)):
                assert got.tobytes() == case["wants"][s].tobytes(), (tag, s)
                rr.check_record(bank.fetch_resampled(s), dict(case["records"][s], frames_written=last_written(case)[s]), (tag, s), BAR)
            same_records(seen, ptr, RESAMPLE_RECORD_DTYPE.itemsize, tag)


# ================================================================ convolve
@pytest.mark.parametrize("ch", CHANNELS["convolve"])
def test_convolve_at_every_alignment(torch_dev, omx, ch):
    """a FIR of tap_block + 1 taps with delay (T - 1) / 2.  Staging peels the head and the tail of the input span; the output peels on
    dst"""
    case = case_of("convolve", ch, omx)[0]
    seen = {}
    for a_in, a_out in PAIRS:
        tag = ("convolve", ch, a_in, a_out)
        bank = new_bank(omx, ch)
        bank.configure_convolve([case["taps"]], ch, None, case["delay"])

        def launch(k, call, ai, ao, in_ptr, out_ptr):
            return bank.convolve(in_ptr, case["cap"], out_ptr, case["out_cap"], frames=[len(r) for r in call["rows"]],
                                 flush_mask=[1] * N if call["flush"] else None, stream=stream_of(torch_dev))

        ptr, parts = run_calls(torch_dev, case, a_in, a_out, launch, tag)
        for s, got in enumerate(whole(parts, ch)):
            cr.same_floats(got, case["wants"][s], (tag, s))
            cr.check_record(bank.fetch_convolved(s), dict(case["records"][s], frames_written=last_written(case)[s]), (tag, s), BAR)
        same_records(seen, ptr, CONVOLVE_RECORD_DTYPE.itemsize, tag)


# ================================================================ dynamics
@pytest.mark.parametrize("ch", CHANNELS["dynamics"])
def test_dynamics_at_every_alignment(torch_dev, omx, ch):
    """every tile of the apply pass peels ps_to_aligned(out) floats and stores v4f behind them.  The 16 pairs without a key and without a
    trace, then once more with d_key (a_in + 1) % 4 and d_gain_db (a_out + 2) % 4 floats behind a boundary: the trace is the
    restatement's on bytes, and the key keeps its bytes"""
    for case in case_of("dynamics", ch, omx):
        curve, keyed = case["curve"], case["keys"] is not None
        seen = {}
        for a_in, a_out in PAIRS:
            tag = ("dynamics", ch, "keyed" if keyed else "plain", a_in, a_out)
            bank = new_bank(omx, ch)
            bank.configure_dynamics([DynamicsCurve(curve.T.astype(np.int32), curve.mask, curve.A, curve.H, curve.d)], ch)

            def launch(k, call, ai, ao, in_ptr, out_ptr):
                counts = [len(r) for r in call["rows"]]
                flush = [1] * N if call["flush"] else None
                if not keyed:
                    return bank.dynamics(in_ptr, case["cap"], out_ptr, case["out_cap"], frames=counts, flush_mask=flush, stream=stream_of(torch_dev))
                key_at, trace_at = (ai + 1) % 4, (ao + 2) % 4
                key_host = rows_of(call["keys"], case["cap"], ch, 60 + k)
                key_image = store_image(key_host, key_at, input_fill(key_host, 6))
                d_key, key_ptr = placed(torch_dev, key_host, key_at, input_fill(key_host, 6))
                blank = np.full(N * case["out_cap"], SENTINEL, np.float32)
                d_tr, tr_ptr = placed(torch_dev, blank, trace_at, SENTINEL)
                ptr = bank.dynamics(in_ptr, case["cap"], out_ptr, case["out_cap"], frames=counts, flush_mask=flush, d_key=key_ptr, d_gain_db=tr_ptr,
                                    stream=stream_of(torch_dev))

                def finish():
                    assert d_key.cpu().numpy().tobytes() == key_image.tobytes(), (tag, k, "the key store changed")
                    check_image(d_tr.cpu().numpy(), store_image(blank, trace_at, SENTINEL), call["traces"], trace_at, case["out_cap"],
                                tag + ("trace of call", k, "at", trace_at), nan_as_nan=False)
                return ptr, finish

            ptr, parts = run_calls(torch_dev, case, a_in, a_out, launch, tag)
            for s, got in enumerate(whole(parts, ch)):
                same_dynamics_floats(got, case["wants"][s], (tag, s), exact=case["E"][s] == 0)
                check_dynamics_record(bank.fetch_dynamics(s), dict(case["records"][s], frames_written=last_written(case)[s]), (tag, s))
            same_records(seen, ptr, DYNAMICS_RECORD_DTYPE.itemsize, tag)


# ================================================================ limiter
@pytest.mark.parametrize("ch", CHANNELS["limiter"])
def test_limiter_at_every_alignment(torch_dev, omx, ch):
    """apply_limited: tile 0 of the apply pass peels the head (threads 0 .. 2) and the tail (threads 4 .. 6); every stream under its own
    gain, over the ceiling in places (the case asserts that frames are limited)"""
    case = case_of("limiter", ch, omx)[0]
    d_gains, _ = limit_gains_on_device(torch_dev, case["factors"])
    bank = new_bank(omx, ch)
    bank.configure_limiter(LimitRule(*LIMIT_RULE), ch, FS)
    seen = {}
    for a_in, a_out in PAIRS:
        tag = ("limiter", ch, a_in, a_out)
        bank.reset_limiter()

        def launch(k, call, ai, ao, in_ptr, out_ptr):
            return bank.apply_limited(in_ptr, case["cap"], out_ptr, case["out_cap"], d_gains.data_ptr(), N, frames=[len(r) for r in call["rows"]],
                                      flush_mask=[1] * N if call["flush"] else None, stream=stream_of(torch_dev))

        ptr, parts = run_calls(torch_dev, case, a_in, a_out, launch, tag)
        for s, got in enumerate(whole(parts, ch)):
            assert same_limit_floats(got, case["wants"][s]), (tag, s, "output differs from the restatement")
            lr.check_record(bank.fetch_limited(s), dict(case["records"][s], frames_written=last_written(case)[s]), (tag, s))
        same_records(seen, ptr, LIMIT_RECORD_DTYPE.itemsize, tag)


# ================================================================ remix
@pytest.mark.parametrize("ch", CHANNELS["remix"])
def test_remix_at_every_alignment(torch_dev, omx, ch):
    """`ch` channels in: 6 to 2 (down), 1 to 2 (up), 4 to 4 (square: rows of both sides move with the base alone).  The input peels and
    shifts its LDS staging, the output peels and shifts by y_shift"""
    case = case_of("remix", ch, omx)[0]
    bank = new_bank(omx, ch)
    bank.configure_remix(case["matrix"], case["ci"], case["co"])
    seen = {}
    for a_in, a_out in PAIRS:
        tag = ("remix", case["ci"], case["co"], a_in, a_out)

        def launch(k, call, ai, ao, in_ptr, out_ptr):
            return bank.remix(in_ptr, out_ptr, case["cap"], frames=[len(r) for r in call["rows"]], stream=stream_of(torch_dev))

        ptr, _ = run_calls(torch_dev, case, a_in, a_out, launch, tag, nan_as_nan=False)
        for s in range(N):
            mr.check_record(bank.fetch_remixed(s), case["records"][s], (tag, s), BAR)
        same_records(seen, ptr, REMIX_RECORD_DTYPE.itemsize, tag)


# ================================================================ inspect
@pytest.mark.parametrize("ch", CHANNELS["inspect"])
def test_inspect_at_every_alignment(torch_dev, omx, ch):
    """no output buffer: d_in at the four offsets (the input peel and the shift of the LDS staging); the records are the restatement's
    on bytes, and d_in keeps its bytes"""
    case = case_of("inspect", ch, omx)[0]
    host = rows_of(case["xs"], case["cap"], ch, 40)
    want = b"".join(r.tobytes() for r in case["records"])
    for a_in in OFFSETS:
        bank = new_bank(omx, ch)
        bank.configure_inspect(InspectRule(**case["rule"]), ch, case["pairs"])
        image = store_image(host, a_in, input_fill(host))
        d_in, in_ptr = placed(torch_dev, host, a_in, input_fill(host))
        ptr = bank.inspect(in_ptr, case["cap"], frames=[len(x) for x in case["xs"]], stream=stream_of(torch_dev))
        torch_dev.cuda.synchronize()
        assert d_in.cpu().numpy().tobytes() == image.tobytes(), (ch, a_in, "the input store changed")
        got = device_bytes(ptr, N * INSPECT_RECORD_DTYPE.itemsize)
        for s in range(N):
            rec = bank.fetch_inspected(s)
            assert rec.tobytes() == case["records"][s].tobytes(), (ch, a_in, s, "record differs from the restatement", rec, case["records"][s])
        assert got == want, (ch, a_in)


# ================================================================ filter
@pytest.mark.parametrize("ch", CHANNELS["filter"])
def test_filter_at_every_alignment(torch_dev, omx, ch):
    """both forms, the 16 pairs out of place and the four offsets in place.  The tile leaves as whole rows through float4 stores where
    d_out is 16-byte aligned and the row's float index a multiple of 4, through dword stores elsewhere.  Reference order: the
    restatement on bytes (a NaN where it has a NaN), the record of every call from the restatement.  Time-parallel: check_time_parallel
    (bar_of) on the two calls together, the record of every call held to the floats the device wrote"""
    case = case_of("filter", ch, omx)[0]
    figures = []
    for form in (1, 2):
        seen = {}
        for a_in, a_out, in_place in [(a, b, False) for a, b in PAIRS] + [(a, a, True) for a in OFFSETS]:
            tag = ("filter", ch, "form", form, "in place" if in_place else "out of place", a_in, a_out)
            bank = new_bank(omx, ch)
            bank.configure_filter(case["filters"], ch, FS, case["foc"])
            bank.set_filter_form(form)
            totals = [0] * N

            def launch(k, call, ai, ao, in_ptr, out_ptr):
                return bank.filter(in_ptr, out_ptr, case["cap"], frames=[len(r) for r in call["rows"]], stream=stream_of(torch_dev))

            def after(k, call, rows, ptr):
                assert bank.last_filter_form() == form
                records = np.frombuffer(device_bytes(ptr, N * FILTER_RECORD_DTYPE.itemsize), FILTER_RECORD_DTYPE)
                for s in range(N):
                    totals[s] += call["emits"][s]
                    out = call["wants"][s] if form == 1 else rows[s].reshape(-1, ch)
                    check_filter_record(records[s], fr.record(out, totals[s], form, FLOOR), (tag, "call", k, s))
                    assert bank.fetch_filtered(s).tobytes() == records[s].tobytes()

            ptr, parts = run_calls(torch_dev, case, a_in, a_out, launch, tag, in_place=in_place, exact=form == 1, after=after)
            if form == 2:
                check_time_parallel(whole(parts, ch), case["wants"], case["xs"], tag, figures)
                if case["foc"] is not None:      # a lane on bypass keeps its bits in this form too
                    for s, got in enumerate(whole(parts, ch)):
                        b = (s + 1) % ch
                        assert got[:, b].tobytes() == case["xs"][s][:, b].tobytes(), (tag, s, b)
            same_records(seen, ptr, FILTER_RECORD_DTYPE.itemsize, tag)
    print("largest figure:", max(figures))


# ================================================================ edit
@pytest.mark.parametrize("ch", CHANNELS["edit"])
def test_edit_at_every_alignment(torch_dev, omx, ch):
    """the clip table of test_cpu_program_alignment.edit_clips: a copy of the hard values on bits, a crossfade whose sources lie four
    frames apart (both on the output's 16-byte phase at some pairs: WIDE) and one whose sources lie an odd number of frames apart (at
    odd channel counts never both: source A on a boundary and source B off it, not WIDE), zero fill in front and behind"""
    case = case_of("edit", ch, omx)[0]
    bank = new_bank(omx, ch)
    bank.configure_edit(ch, N)
    clips = [EditClip(**c.__dict__) for c in case["clips"]]
    seen = {}
    for a_in, a_out in PAIRS:
        tag = ("edit", ch, a_in, a_out)

        def launch(k, call, ai, ao, in_ptr, out_ptr):
            return bank.edit(in_ptr, case["cap"], clips, out_ptr, case["out_cap"], case["out_frames"], frames_in=[len(x) for x in case["xs"]],
                             stream=stream_of(torch_dev))

        ptr, _ = run_calls(torch_dev, case, a_in, a_out, launch, tag, nan_as_nan=False)
        for o in range(N):
            er.check_record(bank.fetch_edited(o), case["records"][o], (tag, o))
        same_records(seen, ptr, EDIT_RECORD_DTYPE.itemsize, tag)


# ================================================================ mix
@pytest.mark.parametrize("ch", CHANNELS["mix"])
def test_mix_at_every_alignment(torch_dev, omx, ch):
    """the send table of test_cpu_program_alignment.mix_sends: bus 2 has frames and no send, so its whole window is the v4f zero fill
    behind its peel; bus 4 sums layers behind two silent frames"""
    case = case_of("mix", ch, omx)[0]
    bank = new_bank(omx, ch)
    bank.configure_mix(ch, N)
    sends = [MixSend(**s.__dict__) for s in case["sends"]]
    seen = {}
    for a_in, a_out in PAIRS:
        tag = ("mix", ch, a_in, a_out)

        def launch(k, call, ai, ao, in_ptr, out_ptr):
            return bank.mix(in_ptr, case["cap"], sends, out_ptr, case["out_cap"], case["out_frames"], frames_in=[len(x) for x in case["xs"]],
                            stream=stream_of(torch_dev))

        ptr, _ = run_calls(torch_dev, case, a_in, a_out, launch, tag)
        for o in range(N):
            xr.check_record(bank.fetch_mixed(o), case["records"][o], (tag, o))
        same_records(seen, ptr, MIX_RECORD_DTYPE.itemsize, tag)


# ================================================================ PCM
@pytest.mark.parametrize("ch", CHANNELS["import_pcm"])
def test_import_pcm_at_every_alignment(torch_dev, omx, ch):
    """S16, S24 and S32: the integer d_in 0, 4, 8 and 12 bytes behind a 16-byte boundary (the head bytes up to the aligned body of the
    integer row, and the byte-align shift) against the f32 d_out at 0 .. 3 floats"""
    for case in case_of("import_pcm", ch, omx):
        bank = new_bank(omx, ch)
        for a_in, a_out in PAIRS:
            tag = ("import_pcm", case["fmt"], ch, 4 * a_in, a_out)

            def launch(k, call, ai, ao, in_ptr, out_ptr):
                assert bank.import_pcm(in_ptr, case["fmt"], out_ptr, case["cap"], ch, frames=case["counts"], stream=stream_of(torch_dev)) == 1
                return 0

            run_calls(torch_dev, case, a_in, a_out, launch, tag, nan_as_nan=False)


@pytest.mark.parametrize("ch", CHANNELS["export_pcm"])
def test_export_pcm_at_every_alignment(torch_dev, omx, ch):
    """the reverse: the f32 d_in at 0 .. 3 floats against the integer d_out at 0, 4, 8 and 12 bytes; TPDF dither under the rule of
    test_gpu_program_pcm.py, so the bytes are program_pcm_ref's"""
    for case in case_of("export_pcm", ch, omx):
        bank = new_bank(omx, ch)
        bank.configure_export(ExportRule(*case["rule"]), ch)
        seen = {}
        for a_in, a_out in PAIRS:
            tag = ("export_pcm", case["fmt"], ch, a_in, 4 * a_out)
            bank.reset_export()

            def launch(k, call, ai, ao, in_ptr, out_ptr):
                return bank.export_pcm(in_ptr, out_ptr, case["cap"], frames=[len(r) for r in call["rows"]], stream=stream_of(torch_dev))

            ptr, _ = run_calls(torch_dev, case, a_in, a_out, launch, tag, nan_as_nan=False)
            for s in range(N):
                pr.check_record(bank.fetch_exported(s), case["records"][s], (tag, s))
            same_records(seen, ptr, EXPORT_RECORD_DTYPE.itemsize, tag)


# ================================================================ apply_gains
@pytest.mark.parametrize("ch", CHANNELS["apply_gains"])
def test_apply_gains_at_every_alignment(torch_dev, omx, ch):
    """in place at the four offsets, through the normalize file's apply_case and on its assertions (the 16 pairs out of place are that
    file's test_apply_is_exact_when_loads_and_stores_are_aligned_differently): the WIDE and the dword forms with one pointer"""
    case = case_of("apply_gains", ch, omx)[0]
    first = None
    for a in OFFSETS:
        bank = apply_case(torch_dev, omx, case["xs"], case["cap"], ch, case["factors"], True, ("in place", ch, a), in_offset=a)
        records = b"".join(bank.fetch_applied(s).tobytes() for s in range(N))
        assert len(records) == N * APPLY_RECORD_DTYPE.itemsize
        first = first or records
        assert records == first, (ch, a, "the records differ from those at offset 0")


# ================================================================ process
@pytest.mark.parametrize("ch", CHANNELS["process"])
def test_process_at_every_alignment(torch_dev, omx, ch):
    """measurement with set_peaks and set_peak_timeline on, d_in at the four offsets.  program_loudness_kernels.hip and
    program_peaks_kernels.hip load d_in by single floats and choose no path by an address (no ps_to_aligned, no vector load of d_in), so
    one channel count suffices: 3, whose odd rows reach every residue on their own.  The loudness record, the peak record and the peak
    rows at every offset have the bytes of the run at offset 0, and that run meets the restatements on the loudness file's bars.  The
    programmes are finite: a NaN would poison the loudness"""
    case = case_of("process", ch, omx)[0]
    fs, lengths = case["fs"], [len(x) for x in case["xs"]]
    host = rows_of(case["xs"], case["cap"], ch, 40)
    first = None
    for a_in in OFFSETS:
        bank = new_bank(omx, ch, fs, 20)
        bank.set_peaks(True)
        bank.set_peak_timeline(True)
        image = store_image(host, a_in, input_fill(host))
        d_in, in_ptr = placed(torch_dev, host, a_in, input_fill(host))
        bank.process(in_ptr, case["cap"], ch, fs, case["positions"], frames=lengths, stream=stream_of(torch_dev))
        torch_dev.cuda.synchronize()
        assert d_in.cpu().numpy().tobytes() == image.tobytes(), (a_in, "the input store changed")
        got = [(record_array(bank.fetch(s)).tobytes(), bank.fetch_peaks(s).tobytes(), bank.fetch_peak_rows(s).tobytes()) for s in range(N)]
        if first is None:
            first = got
            for s in range(N):
                check_loudness_record(bank.fetch(s), case["records"][s], ("process", s))
                check_peaks(bank.fetch_peaks(s), case["peaks"][s], ("process", s))
                assert int(bank.fetch(s).frames) == lengths[s]
            assert len(bank.fetch_peak_rows(4)) == 80
        for s in range(N):
            assert got[s] == first[s], (a_in, s, "the records differ from those at offset 0")

"""The text of the programme bank's refusals (`-m gpu`): the stage tests check the status of a refused call, this one the message
omx_last_error holds behind it.

One bank of 2 streams, one device buffer of 512 floats, no signal processing: every call below is refused on the host before
anything is launched, so nothing here can fault or hang a device.  Each stage is configured first where it has a configure call, so
that the refusal comes from the call's own checks and not from "not configured".  The expected strings are the literal tables below,
read out of the sources as they stood before the stages' call checks moved into program_stage.hpp; the status is ERR_INVALID
throughout."""
import numpy as np
import pytest

from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import PCM_S16, UNITY_GAIN, ExportRule, InspectRule, LimitRule, ProgramLoudnessBank, ResampleRule
from test_gpu_program_loudness import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

N, CH, CAP = 2, 2, 16  # streams, channels, frames per row: a buffer of N * CAP * CH = 64 floats

# call -> (frames[0] = CAP + 1, frames_capacity = 2^32, d_out one float into d_in)
CALLS = {
    "process": ("program loudness process: frames[s] > frames_capacity",
                "program loudness process: frames_capacity beyond 2^32 - 1",
                None),
    "apply_gains": ("program loudness apply_gains: frames[s] > frames_capacity",
                    "program loudness apply_gains: frames_capacity beyond 2^32 - 1",
                    "program loudness apply_gains: d_in and d_out overlap without being the same buffer"),
    "apply_limited": ("program loudness apply_limited: frames[s] > frames_capacity",
                      "program loudness apply_limited: frames_capacity or out_capacity beyond 2^32 - 1",
                      "program loudness apply_limited: d_in and d_out overlap"),
    "import_pcm": ("program loudness import_pcm: frames[s] > frames_capacity",
                   "program loudness import_pcm: frames_capacity beyond 2^32 - 1",
                   "program loudness import_pcm: d_in and d_out overlap"),
    "export_pcm": ("program loudness export_pcm: frames[s] > frames_capacity",
                   "program loudness export_pcm: frames_capacity beyond 2^32 - 1",
                   "program loudness export_pcm: d_in and d_out overlap"),
    "resample": ("program loudness resample: frames[s] > frames_capacity",
                 "program loudness resample: frames_capacity or out_capacity beyond 2^32 - 1",
                 "program loudness resample: d_in and d_out overlap"),
    "remix": ("program loudness remix: frames[s] > frames_capacity",
              "program loudness remix: frames_capacity beyond 2^32 - 1",
              "program loudness remix: d_in and d_out overlap"),
    "inspect": ("program loudness inspect: frames[s] > frames_capacity",
                "program loudness inspect: frames_capacity beyond 2^32 - 1",
                None),
}
# fetch call -> stream index N of a bank of N streams
FETCHES = {
    "fetch": "program loudness fetch: stream index out of range",
    "fetch_segments": "program loudness fetch_segments: range outside the stored segments",
    "fetch_peaks": "program loudness fetch_peaks: stream index out of range",
    "fetch_timeline": "program loudness fetch_timeline: stream index out of range",
    "fetch_intervals": "program loudness measure_intervals: stream index out of range or interval outside the stored segments",
    "fetch_groups": "program loudness measure_groups: stream index out of range or member outside the stored segments",
    "fetch_applied": "program loudness fetch_applied: no apply_gains call yet, or stream index out of range",
    "fetch_limited": "program loudness fetch_limited: the limiter is not configured, or stream index out of range",
    "fetch_exported": "program loudness fetch_exported: the export is not configured, or stream index out of range",
    "fetch_resampled": "program loudness fetch_resampled: the resampler is not configured, or stream index out of range",
    "fetch_remixed": "program loudness fetch_remixed: the remix is not configured, or stream index out of range",
    "fetch_inspected": "program loudness fetch_inspected: the inspector is not configured, or stream index out of range",
    "fetch_histogram": "program loudness fetch_histogram: stream index out of range",
}
# one further refusal of each of these
OTHERS = {
    "timeline": "program loudness timeline: stride 0",
    "measure_groups": "program loudness measure_groups: group range outside the member table",
    "fetch_gains": "program loudness fetch_gains: no plan yet (plan_gains / plan_group_gains)",
    "fetch_peaks": "program loudness fetch_peaks: peaks are off (omx_program_loudness_bank_set_peaks)",
    "fetch_histogram": "program loudness fetch_histogram: the bank stores segments, not histograms",
}


def refused(call, message):
    with pytest.raises(capi.OmxError) as err:
        call()
    assert err.value.status == capi.ERR_INVALID, (message, err.value.status)
    assert str(err.value) == f"omx status {capi.ERR_INVALID}: {message}"


@pytest.fixture(scope="module")
def rig(torch_dev, omx):  # noqa: F811
    store = torch_dev.zeros((512,), dtype=torch_dev.float32).cuda()
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), N, CH, 10)
    bank.configure_limiter(LimitRule(), CH, 48000.0)
    bank.configure_export(ExportRule(), CH)
    bank.configure_resampler(ResampleRule(), CH)
    bank.configure_remix(np.eye(CH, dtype=np.float32), CH, CH)
    bank.configure_inspect(InspectRule(), CH)
    torch_dev.cuda.synchronize()
    d_in = store.data_ptr()
    yield bank, d_in, d_in + 1024  # d_out: 256 floats further on
    bank.close()


def stage_calls(bank, d_in):
    """call -> f(d_out, frames_capacity, frames); no stream names a gain record, and the limiter and the resampler may emit CAP frames"""
    positions = capi.positions_fallback(CH)
    unity = [UNITY_GAIN] * N
    return {
        "process": lambda d_out, cap, fr: bank.process(d_in, cap, CH, 48000.0, positions, frames=fr),
        "apply_gains": lambda d_out, cap, fr: bank.apply_gains(d_in, d_out, cap, CH, 0, 0, frames=fr, gain_of_stream=unity),
        "apply_limited": lambda d_out, cap, fr: bank.apply_limited(d_in, cap, d_out, CAP, 0, 0, frames=fr, gain_of_stream=unity),
        "import_pcm": lambda d_out, cap, fr: bank.import_pcm(d_in, PCM_S16, d_out, cap, CH, frames=fr),
        "export_pcm": lambda d_out, cap, fr: bank.export_pcm(d_in, d_out, cap, frames=fr),
        "resample": lambda d_out, cap, fr: bank.resample(d_in, cap, d_out, CAP, frames=fr),
        "remix": lambda d_out, cap, fr: bank.remix(d_in, d_out, cap, frames=fr),
        "inspect": lambda d_out, cap, fr: bank.inspect(d_in, cap, frames=fr),
    }


@pytest.mark.parametrize("who", list(CALLS))
def test_frame_counts_capacities_and_overlaps(rig, who):
    bank, d_in, d_out = rig
    call = stage_calls(bank, d_in)[who]
    too_many, too_long, overlap = CALLS[who]
    refused(lambda: call(d_out, CAP, [CAP + 1, 0]), too_many)
    refused(lambda: call(d_out, 2 ** 32, [0, 0]), too_long)
    if overlap:
        refused(lambda: call(d_in + 4, CAP, [CAP, CAP]), overlap)


def test_stream_index_out_of_range(rig, omx):
    bank = rig[0]
    bank.set_peaks(True)
    fetches = {
        "fetch": lambda: bank.fetch(N),
        "fetch_segments": lambda: bank.fetch_segments(N, 0, 0),
        "fetch_peaks": lambda: bank.fetch_peaks(N),
        "fetch_timeline": lambda: bank.fetch_timeline(N, 0, 1, 1),
        "fetch_intervals": lambda: bank.fetch_intervals([(N, 0, 0)]),
        "fetch_groups": lambda: bank.fetch_groups([(N, 0, 0)], [(0, 1)]),
        "fetch_applied": lambda: bank.fetch_applied(N),
        "fetch_limited": lambda: bank.fetch_limited(N),
        "fetch_exported": lambda: bank.fetch_exported(N),
        "fetch_resampled": lambda: bank.fetch_resampled(N),
        "fetch_remixed": lambda: bank.fetch_remixed(N),
        "fetch_inspected": lambda: bank.fetch_inspected(N),
    }
    for who, call in fetches.items():
        refused(call, FETCHES[who])
    bank.set_peaks(False)
    bounded = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=48000.0), N, CH, storage="histogram")
    refused(lambda: bounded.fetch_histogram(N), FETCHES["fetch_histogram"])
    bounded.close()
    assert set(fetches) | {"fetch_histogram"} == set(FETCHES)


def test_one_refusal_of_each_other_call(rig):
    bank, d_in, _ = rig
    others = {
        "timeline": lambda: bank.timeline(d_in, first=0, stride=0, count=1),
        "measure_groups": lambda: bank.measure_groups([(0, 0, 0)], [(1, 1)]),
        "fetch_gains": lambda: bank.fetch_gains(0, 1),
        "fetch_peaks": lambda: bank.fetch_peaks(0),  # (peaks are off: a new bank, and test_stream_index_out_of_range switches them off again)
        "fetch_histogram": lambda: bank.fetch_histogram(0),
    }
    assert set(others) == set(OTHERS)
    for who, call in others.items():
        refused(call, OTHERS[who])

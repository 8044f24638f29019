"""Programme loudness bank: both forms of the segment pass on the two shapes that decide the form threshold, the existing loudness
bank's chunk-parallel call on the same buffer in the same run, and the result pass at 10 min and 4 h of stored segments.
HIP events after a warm-up, one process; prints one line per measurement."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import openmeters_amd  # noqa: E402
from openmeters_amd import banks, capi  # noqa: E402
from openmeters_amd.program_loudness import ProgramLoudnessBank  # noqa: E402

api = openmeters_amd.api()
FS = 48000.0
stream = torch.cuda.current_stream().cuda_stream


def timed(run, warm, reps):
    """median and spread of `reps` event-timed calls after `warm` untimed ones"""
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def segment_pass(S, C, frames, warm, reps, with_meter):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    pcm = torch.randn((S, frames, C), device="cuda", generator=gen) * 0.1
    pos = capi.SURROUND if C == 8 else capi.positions_fallback(C)
    gb = S * frames * C * 4 / 1e9
    out = {}
    runs = []
    for form, name in ((1, "reference-order"), (2, "time-parallel"), (0, "by shape")):
        # capacity: every call appends frames / 4800 segments; a full bank would stop taking samples
        bank = ProgramLoudnessBank(api, capi.LoudnessConfig(), S, C, int((warm + 2 * reps + 4) * frames / FS) + 60)
        bank.set_option(capi.OPT_KERNEL_FORM, form)
        runs.append((name, bank, lambda bank=bank: bank.process(pcm.data_ptr(), frames, C, FS, pos, stream=stream)))
    if with_meter:
        meter = banks.LoudnessBank(api, capi.LoudnessConfig(), S, C)
        meter.set_option(capi.OPT_KERNEL_FORM, 2)
        runs.append(("loudness bank, chunk-parallel (existing)", meter, lambda: meter.process_device(pcm.data_ptr(), 256, frames // 256, C, FS, pos, stream)))
    for rnd in range(2):  # alternate the arms: two rounds each
        for name, bank, run in runs:
            med, lo, hi = timed(run, warm if rnd == 0 else 2, reps)
            out.setdefault(name, []).append(med)
            form = bank.last_form() if hasattr(bank, "last_form") else 0
            print(f"{S} x {C} ch x {frames} frames, {name} (form {form}), round {rnd}: {med:.3f} ms/call (min {lo:.3f}, max {hi:.3f}), "
                  f"{gb / med * 1e3:.0f} GB/s of PCM", flush=True)
    return out


def result_pass(S, seconds):
    segs = int(seconds * 10)
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(), S, 2, seconds)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    # fill the storage through the public interface: a few long calls of noise with a level step every 5 s
    call = 48000 * 600
    pos = capi.positions_fallback(2)
    left = seconds * 48000
    while left > 0:
        n = min(call, left)
        steps = 10.0 ** (torch.empty((S, n // 240000 + 1, 1), device="cuda").uniform_(-70.0, -10.0, generator=gen) / 20.0)
        pcm = torch.randn((S, n, 2), device="cuda", generator=gen) * steps.repeat_interleave(240000, dim=1)[:, :n]
        bank.process(pcm.data_ptr(), n, 2, FS, pos, stream=stream)
        torch.cuda.synchronize()
        left -= n
    med, lo, hi = timed(lambda: bank.results(stream), 3, 10)
    r = bank.fetch(0)
    print(f"result pass, {S} streams x {segs} segments ({seconds / 60:.0f} min): {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); stream 0: I {r.integrated_lufs:.3f} "
          f"LUFS, LRA {r.loudness_range_lu:.3f} LU, {r.gating_above_relative}/{r.gating_blocks} gating blocks above both gates", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["bank", "long", "results"]
    if "bank" in what:
        segment_pass(1024, 8, 16384, 10, 20, True)
    if "long" in what:
        segment_pass(64, 2, 60 * 48000, 3, 6, False)
    if "results" in what:
        result_pass(64, 600)
        result_pass(8, 4 * 3600)

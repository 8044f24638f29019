"""Programme loudness bank, filter stage (include/omx/program_filter.h): what `filter` costs beside two yardsticks on the same
buffers in the same run.

  apply_gains out of place : reads N and writes N bytes of f32, the memory floor of one read and one write
  process pinned to form 2 : the K-weighting recurrence of the same shape (two biquads in f64, time-parallel) without the store;
                             every stream is reset in the call, so the bank never fills

Arms: the filter in reference order (form 1) and in the time-parallel form (form 2), out of place and in place, with a one-section
filter (DC_BLOCK at 5 Hz) and a two-section one (20 Hz fourth-order high-pass).  Shapes: 1024 streams x 16 384 frames at 2 and at 8
channels, 64 streams x 60 s at 48 kHz and 2 channels.  The in-place arms work on a copy of the input that they filter again and again.
HIP events around `inner` back-to-back calls after a warm-up, one process.  The arms of a shape ALTERNATE (a b c a b c ...), and per arm
the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those two
is the spread of the run, and an arm is slower than another only beyond it.  Reference order on the long shape leaves the card to two
wavefronts and takes a third of a second per call: those arms run one call per repetition.
The lines go to --out (default profiles/program_filter.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_filter.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import (FILTER_DC_BLOCK, FILTER_HIGHPASS, GAIN_RECORD_DTYPE, FilterSpec, ProgramLoudnessBank, filter_design)

LINES = []
FLOOR = "apply_gains out of place"
PROCESS = "process, form 2"


def say(line):
    print(line, flush=True)
    LINES.append(line)


def alternated(arms, inner_of, warm, reps):
    """arms: name -> callable.  Every repetition runs each arm in turn, inner_of[name] calls between its own pair of events; ms per call"""
    for _ in range(warm):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(reps):
        for name, run in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner_of[name]):
                run()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / inner_of[name])
    out = {}
    for name, v in ms.items():
        s = sorted(v)
        out[name] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "reps": reps, "median_even": float(np.median(v[0::2])),
                     "median_odd": float(np.median(v[1::2])) if reps > 1 else s[0]}
    return out


def shape(key, title, api, S, ch, cap, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    fs = 48000.0
    n = S * cap * ch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    f32_in = torch.empty((n,), device="cuda").uniform_(-0.5, 0.5, generator=gen)
    f32_out = torch.zeros((n,), device="cuda")
    work = f32_in.clone()
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.7)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    positions = capi.positions_fallback(ch)
    everyone = np.ones((S,), np.uint8)
    meter = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, max(int(cap / fs) + 2, 2))
    meter.set_option(capi.OPT_KERNEL_FORM, 2)
    designs = {"one section": filter_design(api, FilterSpec(FILTER_DC_BLOCK, 0, 5.0), fs),
               "two sections": filter_design(api, FilterSpec(FILTER_HIGHPASS, 4, 20.0), fs)}
    banks = {}
    arms = {FLOOR: lambda: meter.apply_gains(f32_in.data_ptr(), f32_out.data_ptr(), cap, ch, gains.data_ptr(), S, stream=stream),
            PROCESS: lambda: meter.process(f32_in.data_ptr(), cap, ch, fs, positions, reset_mask=everyone, stream=stream)}
    inner_of = {FLOOR: args.inner, PROCESS: args.inner}
    slow = cap > 4 * 16384  # reference order on a long call
    for sections, design in designs.items():
        for form in (1, 2):
            bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, 1)
            bank.configure_filter([design], ch, fs)
            bank.set_filter_form(form)
            banks[(sections, form)] = bank
            for place, dst in (("out of place", f32_out), ("in place", None)):
                name = f"filter, form {form}, {sections}, {place}"
                if dst is None:
                    arms[name] = lambda bank=bank: bank.filter(work.data_ptr(), work.data_ptr(), cap, stream=stream)
                else:
                    arms[name] = lambda bank=bank, dst=dst: bank.filter(f32_in.data_ptr(), dst.data_ptr(), cap, stream=stream)
                inner_of[name] = 1 if (slow and form == 1) else args.inner
    out[key] = t = alternated(arms, inner_of, args.warmup, args.reps)
    assert meter.last_form() == 2
    both = t[FLOOR]["median"] + t[PROCESS]["median"]
    for arm, r in t.items():
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f})")
        if arm == FLOOR:
            line += f", {8 * n / 1e9:.3f} GB read + written, {8 * n / (r['median'] * 1e-3) / 1e12:.2f} TB/s"
        elif arm != PROCESS:
            r["ratio_to_floor"], r["ratio_to_process"], r["ratio_to_both"] = r["median"] / t[FLOOR]["median"], r["median"] / t[PROCESS]["median"], r["median"] / both
            line += f", {r['ratio_to_floor']:.2f} x apply_gains, {r['ratio_to_process']:.2f} x process, {r['ratio_to_both']:.2f} x the sum of the two"
        say(line)
    for (sections, form), bank in banks.items():
        assert bank.last_filter_form() == form, (sections, form, bank.last_filter_form())
        rec = bank.fetch_filtered(S - 1)
        say(f"    form {form}, {sections}, stream {S - 1}: {int(rec['frames'])} frames of {int(rec['frames_total'])}, {int(rec['samples_over'])} over, "
            f"{int(rec['samples_nonfinite'])} not finite, peak {float(rec['out_sample_peak']):.6f}, form {int(rec['form'])}")
        bank.close()
    meter.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_filter.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_filter needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    shape("1024x2x16384", "1024 x 16 384 frames, 2 channels", api, 1024, 2, 16384, args, out)
    shape("1024x8x16384", "1024 x 16 384 frames, 8 channels", api, 1024, 8, 16384, args, out)
    shape("64x2x60s", "64 x 60 s at 48 kHz, 2 channels", api, 64, 2, 60 * 48000, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

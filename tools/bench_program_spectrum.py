"""Programme loudness bank, long-term spectrum (include/omx/program_spectrum.h): what `spectrum` costs beside `inspect` on the same PCM,
and beside the bytes it moves.

Both passes read the PCM once; the spectrum pass also writes one f64 row of N/2 + 1 bins per channel and run of 16 transforms and
reads it back in the chain pass.  Per transform and channel the work is an N/2-point complex transform, the untangling pass and N/2 + 1
f64 additions; at half overlap every sample is transformed twice.
Arms: 64 streams x 2 channels x 60 s at 48 kHz, 1024 streams x 8 channels x 16 384 frames, and ONE stream x 2 channels x 10 minutes
(no kernel walks a stream's frames: the long stream has to run as wide as the 64 short ones), all at N = 4096 on noise.  Every call
adds to the running sums; the streams are reset in time for the 2^32 - 1 frame limit.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The two arms of a shape ALTERNATE (a b a b ...), and per
arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those
two is the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_spectrum.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_spectrum.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import InspectRule, ProgramLoudnessBank, SpectrumRule, spectrum_plan, spectrum_transforms

LINES = []
YARDSTICK = "inspect on the same PCM"


def say(line):
    print(line, flush=True)
    LINES.append(line)


def alternated(arms, warm, reps, inner):
    """arms: name -> callable.  Every repetition runs each arm in turn, `inner` calls between its own pair of events; ms per call"""
    for _ in range(warm):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(reps):
        for name, run in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                run()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    out = {}
    for name, v in ms.items():
        s = sorted(v)
        out[name] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "reps": reps, "median_even": float(np.median(v[0::2])),
                     "median_odd": float(np.median(v[1::2])) if reps > 1 else s[0]}
    return out


def shape(key, title, api, S, ch, cap, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    n = S * cap * ch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    pcm = torch.empty((n,), device="cuda").uniform_(-0.5, 0.5, generator=gen)
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    bank.configure_inspect(InspectRule(), ch, [(0, 1)])
    rule = SpectrumRule(args.fft_size)
    bank.configure_spectrum(rule, ch)
    calls = {"inspect": 0, "spectrum": 0}

    def inspect():
        if (calls["inspect"] + 1) * cap > 2 ** 32 - 1:
            bank.reset_inspect()
            calls["inspect"] = 0
        calls["inspect"] += 1
        bank.inspect(pcm.data_ptr(), cap, stream=stream)

    def spectrum():
        if (calls["spectrum"] + 1) * cap > 2 ** 32 - 1:
            bank.reset_spectrum()
            calls["spectrum"] = 0
        calls["spectrum"] += 1
        bank.spectrum(pcm.data_ptr(), cap, stream=stream)

    name = f"spectrum, N = {args.fft_size}, {ch} channels"
    info = spectrum_plan(api, rule, ch, S, cap)
    hop, bins, run = int(info["hop"]), int(info["bins"]), int(info["run"])
    transforms = S * ch * (cap // hop)                      # per call in the steady state
    row_bytes = 2 * 8 * bins * S * ch * -(-(cap // hop) // run)   # written by the transform pass, read by the chain pass
    counts = {YARDSTICK: {"bytes": 4 * n}, name: {"bytes": 4 * n + row_bytes, "transforms": transforms, "scratch_bytes": int(info["scratch_bytes"])}}
    out[key] = t = alternated({YARDSTICK: inspect, name: spectrum}, args.warmup, args.reps, args.inner)
    for arm, r in t.items():
        c, sec = counts[arm], r["median"] * 1e-3
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {c['bytes'] / 1e9:.3f} GB read + written, {c['bytes'] / sec / 1e12:.3f} TB/s")
        if arm != YARDSTICK:
            rel = r["median"] / t[YARDSTICK]["median"]
            line += (f", {rel:.2f} x inspect; {transforms} transforms of {args.fft_size} points per call, {transforms / sec / 1e6:.2f} M transforms/s")
            r["ratio_to_inspect"] = rel
        say(line)
        r.update(c)
    rec, _ = bank.fetch_spectrum(S - 1)
    want = spectrum_transforms(api, int(rec["frames"]), False, args.fft_size)
    say(f"    stream {S - 1}: {int(rec['frames'])} frames in {calls['spectrum']} calls, {int(rec['transforms'][0])} transforms on channel 0 "
        f"(the grid gives {want}), {int(rec['skipped'][0])} skipped")
    bank.close()
    return t[name]["median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="calls between one pair of events")
    ap.add_argument("--fft-size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_spectrum.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_spectrum needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    wide = shape("64x2x60s", "64 x 60 s at 48 kHz, 2 channels", api, 64, 2, 60 * 48000, args, out)
    shape("1024x8x16384", "1024 x 16 384 frames, 8 channels", api, 1024, 8, 16384, args, out)
    long_one = shape("1x2x600s", "1 x 10 min at 48 kHz, 2 channels", api, 1, 2, 600 * 48000, args, out)
    ratio = long_one / (wide * 600.0 / (64 * 60.0))
    say(f"one 10-minute stream takes {ratio:.2f} x the time of its share of 64 streams of 60 s (1.00: as parallel)")
    out["long_stream_ratio"] = ratio
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

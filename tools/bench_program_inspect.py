"""Programme loudness bank, signal QC (include/omx/program_inspect.h): what `inspect` costs beside apply_gains out of place on the same
shape.

The yardstick reads N and writes N bytes of f32: the family's stand-in for a device-to-device copy of the input.  The inspector reads
N bytes once and writes 32 bytes per predicate and tile plus 8 bytes per sum and tile, well under one percent of N: `bytes ratio` is
0.5, the time a pass as good as the yardstick would take, in yardsticks.  The issue's expectation is a ratio at or under 1.0.
Arms: 1024 streams x 16 384 frames at 2 and at 8 channels (noise within +-1.2, some samples hot, one pair); 64 streams x 60 s at 48 kHz,
2 channels, on that noise, on all-quiet input (zeros: one silent run from end to end) and on all-hot input (ones: one clipping run per
channel from end to end), the worst cases for the run pass.  Every call adds to the running records (the streams are reset between
the arms of a shape only through a fresh bank), so the records show frames of all calls.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The two arms of a shape ALTERNATE (a b a b ...), and per
arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those
two is the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_inspect.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_inspect.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, InspectRule, ProgramLoudnessBank, inspect_plan, inspect_summarize

LINES = []
YARDSTICK = "apply_gains out of place on the same shape"


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


def shape(key, title, api, S, ch, cap, args, out, fill="noise"):
    stream = torch.cuda.current_stream().cuda_stream
    n = S * cap * ch
    if fill == "noise":
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        f32_in = torch.empty((n,), device="cuda").uniform_(-1.2, 1.2, generator=gen)
    else:
        f32_in = torch.full((n,), 0.0 if fill == "quiet" else 1.0, device="cuda")
    yard_out = torch.zeros((n,), device="cuda")
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.7)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    rule = InspectRule()
    bank.configure_inspect(rule, ch, [(0, 1)])
    name = f"inspect, {ch} channels, one pair"
    calls = {"n": 0}

    def inspect():
        # a stream takes at most 2^32 - 1 frames between resets: start over in time (the reset is one small kernel, inside the timing)
        if (calls["n"] + 1) * cap > 2 ** 32 - 1:
            bank.reset_inspect()
            calls["n"] = 0
        calls["n"] += 1
        bank.inspect(f32_in.data_ptr(), cap, stream=stream)

    arms = {YARDSTICK: lambda: bank.apply_gains(f32_in.data_ptr(), yard_out.data_ptr(), cap, ch, gains.data_ptr(), S, stream=stream),
            name: inspect}
    tile = int(inspect_plan(api, ch)["tile_frames"])
    tiles = (cap + tile - 1) // tile
    counts = {YARDSTICK: {"bytes": 8 * n}, name: {"bytes": 4 * n + S * tiles * (32 * (ch + 1) + 8 * (2 * ch + 3)), "tile_frames": tile}}
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    for arm, r in t.items():
        c, sec = counts[arm], r["median"] * 1e-3
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {c['bytes'] / 1e9:.3f} GB read + written, {c['bytes'] / sec / 1e12:.2f} TB/s")
        if arm != YARDSTICK:
            rel = r["median"] / t[YARDSTICK]["median"]
            line += f", {rel:.3f} x the yardstick (bytes ratio 0.500: {rel / 0.5:.3f} x yardstick x bytes ratio)"
            r["ratio_to_yardstick"], r["bytes_ratio"] = rel, 0.5
        say(line)
        r.update(c)
    rec = bank.fetch_inspected(S - 1)
    summary = inspect_summarize(api, rule, rec)
    say(f"    stream {S - 1}: {int(rec['frames'])} frames in {calls['n']} calls, {int(rec['silent_frames'])} silent, "
        f"{int(rec['channel'][0]['clipped_samples'])} clipped and {int(rec['channel'][0]['clip_runs'])} clipping runs on channel 0, longest "
        f"{int(rec['channel'][0]['longest_clip_run'])}, correlation {float(summary['correlation'][0]):.4f}, verdict {int(summary['verdict'])}")
    bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_inspect.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_inspect needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    shape("1024x2x16384", "1024 x 16 384 frames, 2 channels", api, 1024, 2, 16384, args, out)
    shape("1024x8x16384", "1024 x 16 384 frames, 8 channels", api, 1024, 8, 16384, args, out)
    shape("64x2x60s", "64 x 60 s at 48 kHz, 2 channels", api, 64, 2, 60 * 48000, args, out)
    shape("64x2x60s_quiet", "64 x 60 s at 48 kHz, 2 channels, input all zero (one silent run)", api, 64, 2, 60 * 48000, args, out, "quiet")
    shape("64x2x60s_hot", "64 x 60 s at 48 kHz, 2 channels, input all 1.0 (one clipping run per channel)", api, 64, 2, 60 * 48000, args, out, "hot")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

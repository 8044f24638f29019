"""Programme loudness bank, sample-rate conversion (include/omx/program_resample.h): what `resample` costs beside apply_gains out of
place on the input's shape.

The yardstick reads N and writes N bytes of f32.  A conversion reads N bytes and writes N * L / M; per output frame it does
channels * T multiplications and as many additions (nothing is fused) and reads T * channels * 4 bytes from LDS.  Arms per shape:
apply_gains out of place; resample 44.1 -> 48 kHz (L / M = 160 / 147, T = 64); resample 96 -> 48 kHz (1 / 2, T = 128).  Every resample
call continues its streams (no flush, no reset): the steady state of a programme cut into calls, with the carry in use.  Shapes: 1024
streams x 8 ch x 16 384 frames (the project's loudness shape) and 64 x 2 ch x 60 s at 48 kHz.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms ALTERNATE (a b c a b c ...), and per arm the
line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those two is
the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_resample.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_resample.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, ProgramLoudnessBank, ResampleRule, resample_frames, resample_plan

LINES = []
YARDSTICK = "apply_gains out of place (f32 to f32)"
RATES = {"resample 44.1 -> 48 kHz": (44100, 48000), "resample 96 -> 48 kHz": (96000, 48000)}


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
    f32_in = torch.empty((n,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    f32_out = torch.zeros((n,), device="cuda")
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.7)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    arms = {YARDSTICK: lambda: bank.apply_gains(f32_in.data_ptr(), f32_out.data_ptr(), cap, ch, gains.data_ptr(), S, stream=stream)}
    counts = {YARDSTICK: {"bytes": 8 * n, "multiply_adds": 0, "lds_bytes_per_output_frame": 0, "outputs": S * cap}}
    banks, outs = {}, {}
    for name, (rate_in, rate_out) in RATES.items():
        rule = ResampleRule(rate_in, rate_out)
        info = resample_plan(api, rule)
        L, M, T = int(info["L"]), int(info["M"]), int(info["taps"])
        out_cap = cap * L // M + 2
        rs = banks[name] = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
        rs.configure_resampler(rule, ch)
        d_out = outs[name] = torch.zeros((S * out_cap * ch,), device="cuda")
        arms[name] = lambda rs=rs, d_out=d_out, out_cap=out_cap: rs.resample(f32_in.data_ptr(), cap, d_out.data_ptr(), out_cap, stream=stream)
        steady = resample_frames(api, rule, 10 * cap, resample_frames(api, rule, 0, 0, 10 * cap, False), cap, False)      # frames a later call emits
        counts[name] = {"bytes": 4 * S * ch * (cap + steady), "multiply_adds": S * steady * ch * T, "lds_bytes_per_output_frame": T * ch * 4,
                        "outputs": S * steady, "L": L, "M": M, "taps": T, "tile_frames": int(info["tile_frames"])}
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    for name, r in t.items():
        c, sec = counts[name], r["median"] * 1e-3
        line = (f"{title}, {name}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {c['bytes'] / sec / 1e12:.2f} TB/s read + written")
        if name != YARDSTICK:
            line += (f", {r['median'] / t[YARDSTICK]['median']:.3f} x the yardstick; {c['multiply_adds'] / 1e9:.2f} G multiply-adds "
                     f"({c['multiply_adds'] / sec / 1e12:.2f} T/s), {c['lds_bytes_per_output_frame']} LDS bytes read per output frame "
                     f"({c['lds_bytes_per_output_frame'] * c['outputs'] / sec / 1e12:.1f} TB/s), L / M = {c['L']} / {c['M']}, T = {c['taps']}")
        say(line)
        r.update(c)
    for name, rs in banks.items():
        rec = rs.fetch_resampled(S - 1)
        say(f"    stream {S - 1}, {name}: {int(rec['frames_in'])} frames in, {int(rec['frames_out'])} out, {int(rec['samples_over'])} over, "
            f"peak {rec['out_sample_peak_db']:.3f} dB")
        rs.close()
    bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_resample.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_resample needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    shape("1024x8x16384", "1024 x 8 ch x 16 384 frames", api, 1024, 8, 16384, args, out)
    shape("64x2x60s", "64 x 2 ch x 60 s at 48 kHz", api, 64, 2, 60 * 48000, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

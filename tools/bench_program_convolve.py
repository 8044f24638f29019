"""Programme loudness bank, convolve stage (include/omx/program_convolve.h): what `convolve` costs at T = 1, 15, 63, 255, 1023 and 4095
taps beside three yardsticks.

Yardstick 1, apply_gains out of place on the same buffers: reads N and writes N bytes of f32, the family's stand-in for a
device-to-device copy.  It says something up to a few dozen taps, where the pass is still bound by HBM.
Yardstick 2, the resampler: `resample` at 44.1 -> 48 kHz with half_width 32 (64 taps per phase, L >= M) on the same input shape does
the same multiply-adds per output sample in f32 that `convolve` at T = 64 does in f64.
Yardstick 3, the f64 multiply-add rate: tools/microbench/fma64_rate.hip measures what a bare loop of independent v_fma_f64 reaches on
the same box; --fma-rate takes its figure (T multiply-adds per second) and the long FIRs are reported against it.  A pass of S
streams x F frames x C channels x T taps does S F C T multiply-adds.
Every convolve call is a streaming call on a running stream (the stage holds max_taps - 1 frames of each stream on the device): it
takes F frames and emits F, D = (T - 1) / 2.
Arms.  (a) 1024 streams x 16 384 frames at 2 and at 8 channels; (b) 64 streams x 60 s at 48 kHz stereo.  HIP events around `--inner`
back-to-back calls after a warm-up, one process.  The arms of a shape ALTERNATE (a b c a b c ...), and per arm the line gives the
median per call with min and max and the medians of its even and odd repetitions: the distance between those two is the spread of the
run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_convolve.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own, one tap count at a time (the stats are per kernel name):
rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_convolve.py --reps 3 --taps 1 --shapes a2,a8"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, ProgramLoudnessBank, ResampleRule, convolve_plan

LINES = []
YARDSTICK = "apply_gains out of place"
RESAMPLE = "resample 44.1 -> 48 kHz, 64 taps per phase (f32)"
TAPS = (1, 15, 63, 64, 255, 1023, 4095)


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


def shape(key, title, api, n, ch, frames, taps, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    d_in = torch.empty((n * frames * ch,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    out_cap = frames * 160 // 147 + 2      # what the resampler emits per call, at the most
    d_out = torch.zeros((n * out_cap * ch,), device="cuda")
    g = np.zeros((n,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.5)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    cfg = capi.LoudnessConfig(sample_rate=48000.0)
    yard = ProgramLoudnessBank(api, cfg, n, ch, 1)
    arms = {YARDSTICK: lambda: yard.apply_gains(d_in.data_ptr(), d_out.data_ptr(), frames, ch, gains.data_ptr(), n, stream=stream)}
    banks = [yard]
    rng = np.random.default_rng(9)
    for T in taps:
        bank = ProgramLoudnessBank(api, cfg, n, ch, 1)
        h = (rng.uniform(-1.0, 1.0, T) / max(T, 1) ** 0.5).astype(np.float32)
        bank.configure_convolve([h], ch, None, (T - 1) // 2)
        banks.append(bank)
        arms[f"convolve, {T} taps"] = lambda bank=bank: bank.convolve(d_in.data_ptr(), frames, d_out.data_ptr(), out_cap, stream=stream)
    rs = ProgramLoudnessBank(api, cfg, n, ch, 1)
    rs.configure_resampler(ResampleRule(44100, 48000, 32), ch)
    banks.append(rs)
    arms[RESAMPLE] = lambda: rs.resample(d_in.data_ptr(), frames, d_out.data_ptr(), out_cap, stream=stream)
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    samples = n * frames * ch
    y = t[YARDSTICK]["median"]
    for arm, r in t.items():
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f})")
        if arm.startswith("convolve"):
            T = int(arm.split()[1])
            r["ratio_to_yardstick"] = r["median"] / y
            r["fma_per_s"] = samples * T / (r["median"] * 1e-3)
            line += f", {r['ratio_to_yardstick']:.3f} x the yardstick, {8 * samples / (r['median'] * 1e-3) / 1e12:.2f} TB/s of PCM, {r['fma_per_s'] / 1e12:.3f} T f64 multiply-adds/s"
            if args.fma_rate > 0:
                r["fraction_of_fma_rate"] = r["fma_per_s"] / (args.fma_rate * 1e12)
                line += f" = {100 * r['fraction_of_fma_rate']:.1f} % of the bare loop's {args.fma_rate:.2f} T/s"
            if T == 64:
                r["ratio_to_resample"] = r["median"] / t[RESAMPLE]["median"]
                line += f"; {r['ratio_to_resample']:.3f} x the resample pass (which emits 160 / 147 as many frames, in f32)"
        elif arm == YARDSTICK:
            line += f", {8 * samples / (r['median'] * 1e-3) / 1e12:.2f} TB/s read + written"
        say(line)
    rec = banks[1].fetch_convolved(n - 1)
    say(f"    stream {n - 1} of the {taps[0]}-tap bank: {int(rec['frames_in'])} frames in, {int(rec['frames_out'])} out, "
        f"{int(rec['frames_written'])} written by the last call, peak {rec['out_sample_peak_db']:.3f} dB")
    for b in banks:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="calls between one pair of events")
    ap.add_argument("--fma-rate", type=float, default=0.0, help="T f64 multiply-adds per second of tools/microbench/fma64_rate.hip on this box")
    ap.add_argument("--shapes", default="a2,a8,b", help="which shapes to run")
    ap.add_argument("--taps", default=",".join(str(t) for t in TAPS), help="tap counts (64 is the one held against the resample pass)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_convolve.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_convolve needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    for ch in (2, 8):
        info = convolve_plan(api, ch, 4096)
        say(f"convolve plan at {ch} channels: tile {int(info['tile_frames'])} frames, {int(info['frames_per_thread'])} frames per thread, "
            f"tap block {int(info['tap_block'])}")
    which = args.shapes.split(",")
    taps = tuple(int(t) for t in args.taps.split(","))
    if "a2" in which:
        shape("a_1024x16384x2", "(a) 1024 streams x 16 384 frames, 2 channels", api, 1024, 2, 16384, taps, args, out)
    if "a8" in which:
        shape("a_1024x16384x8", "(a) 1024 streams x 16 384 frames, 8 channels", api, 1024, 8, 16384, taps, args, out)
    if "b" in which:
        shape("b_64x60s", "(b) 64 streams x 60 s at 48 kHz stereo", api, 64, 2, 60 * 48000, taps, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

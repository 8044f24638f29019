"""Programme loudness bank, channel remix (include/omx/program_remix.h): what `remix` costs beside apply_gains out of place on the
INPUT's shape.

The yardstick reads N and writes N bytes of f32: the family's stand-in for a device-to-device copy of the input.  A remix reads N bytes
and writes N * channels_out / channels_in; per frame it does one multiplication per term of the matrix and one addition per term but
the first of each row (nothing is fused).  `bytes ratio` is (channels_in + channels_out) / (2 * channels_in): the time a pass as good as
the yardstick would take, in yardsticks.
Arms: 1024 streams x 16 384 frames for 6 -> 2 (the BS.775 fold of 5.1), 8 -> 2 (the fold of 7.1), 2 -> 1 (the mono fold), 8 -> 8 (a
permutation) and 2 -> 6 (stereo into the front pair of 5.1, by remix_select); 64 streams x 60 s at 48 kHz for 6 -> 2.  The input is
noise within +-1, so a fold without OMX_REMIX_NORMALIZE goes over in every workgroup; the long shape runs again within +-0.1 and on
silence, which takes the workgroups' atomics on their stream's record away one by one (they are what binds that shape).
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The two arms of a shape ALTERNATE (a b a b ...), and per
arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those
two is the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_remix.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_remix.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, DownmixRule, ProgramLoudnessBank, REMIX_KIND_MONO, remix_downmix, remix_plan, remix_select

LINES = []
YARDSTICK = "apply_gains out of place on the input's shape"


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


def matrix_of(api, ci, co):
    """the matrix of an arm and what it is"""
    pos = capi.positions_fallback(ci)
    if (ci, co) in ((6, 2), (8, 2)):
        return remix_downmix(api, DownmixRule(), ci, pos)[0], "BS.775 fold"
    if (ci, co) == (2, 1):
        return remix_downmix(api, DownmixRule(kind=REMIX_KIND_MONO), ci, pos)[0], "mono fold"
    if ci == co:
        return remix_select(api, ci, pos, co, list(reversed(pos[:ci])))[0], "permutation"
    return remix_select(api, ci, pos, co, capi.positions_fallback(co))[0], "select"


def shape(key, title, api, S, ci, co, cap, args, out, amplitude=1.0):
    stream = torch.cuda.current_stream().cuda_stream
    n_in, n_out = S * cap * ci, S * cap * co
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    f32_in = torch.empty((n_in,), device="cuda").uniform_(-amplitude, amplitude, generator=gen)
    yard_out = torch.zeros((n_in,), device="cuda")
    mix_out = torch.zeros((n_out,), device="cuda")
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.7)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    matrix, what = matrix_of(api, ci, co)
    terms = int((matrix != 0).sum())
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ci, 1)
    bank.configure_remix(matrix, ci, co)
    name = f"remix {ci} -> {co} ({what}, {terms} terms)"
    arms = {YARDSTICK: lambda: bank.apply_gains(f32_in.data_ptr(), yard_out.data_ptr(), cap, ci, gains.data_ptr(), S, stream=stream),
            name: lambda: bank.remix(f32_in.data_ptr(), mix_out.data_ptr(), cap, stream=stream)}
    counts = {YARDSTICK: {"bytes": 8 * n_in}, name: {"bytes": 4 * (n_in + n_out), "terms": terms, "tile_frames": int(remix_plan(api, ci, co)["tile_frames"])}}
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    ratio = (ci + co) / (2.0 * ci)
    for arm, r in t.items():
        c, sec = counts[arm], r["median"] * 1e-3
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {c['bytes'] / 1e9:.3f} GB read + written, {c['bytes'] / sec / 1e12:.2f} TB/s")
        if arm != YARDSTICK:
            rel = r["median"] / t[YARDSTICK]["median"]
            line += f", {rel:.3f} x the yardstick (bytes ratio {ratio:.3f}: {rel / ratio:.3f} x yardstick x bytes ratio)"
            r["ratio_to_yardstick"], r["bytes_ratio"] = rel, ratio
        say(line)
        r.update(c)
    rec = bank.fetch_remixed(S - 1)
    say(f"    stream {S - 1}: {int(rec['frames'])} frames, {int(rec['samples_over'])} over, peak {rec['out_sample_peak_db']:.3f} dB, {int(rec['terms'])} terms")
    bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_remix.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_remix needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    for ci, co in ((6, 2), (8, 2), (2, 1), (8, 8), (2, 6)):
        shape(f"1024x{ci}to{co}x16384", f"1024 x 16 384 frames, {ci} -> {co}", api, 1024, ci, co, 16384, args, out)
    shape("64x6to2x60s", "64 x 60 s at 48 kHz, 6 -> 2", api, 64, 6, 2, 60 * 48000, args, out)
    # the same shape with what a workgroup adds to its stream's record taken away step by step: no sample over (the atomicAdd goes),
    # then silence (the atomicMax goes too)
    shape("64x6to2x60s_quiet", "64 x 60 s at 48 kHz, 6 -> 2, input within +-0.1 (no sample over)", api, 64, 6, 2, 60 * 48000, args, out, 0.1)
    shape("64x6to2x60s_silent", "64 x 60 s at 48 kHz, 6 -> 2, input all zero (no sample over, no peak)", api, 64, 6, 2, 60 * 48000, args, out, 0.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

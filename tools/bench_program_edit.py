"""Programme loudness bank, edit pass (include/omx/program_edit.h): what `edit` costs beside apply_gains out of place on the OUTPUT's
shape.

The yardstick reads N and writes N bytes of f32, N the bytes of the edit's output windows: the family's stand-in for a device-to-device
copy.  An edit writes N and reads 4 bytes per sample and clip that covers it; `bytes ratio` is (read + written) / (2 N), the time a
pass as good as the yardstick would take, in yardsticks.
Arms.  (a) 1024 streams x 16 384 frames at 2 and at 8 channels, one whole-row clip with gain 0.5 per stream (the yardstick's own
arithmetic).  (b) 64 x 60 s at 48 kHz stereo, one whole clip with gain 1 per stream (the copy path).  (c) the same input with a trim of
4801 frames at the head (an odd offset: the dword-load form), fades of 10 ms and pads of 0.5 s.  (d) the 64 sources joined into 8
outputs with equal-power crossfades of 5 s.  (e) the shape of (b) with src_first = 1: the dword-load form alone.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The two arms of a shape ALTERNATE (a b a b ...), and per
arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those
two is the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_edit.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_edit.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import (EDIT_CURVE_EQUAL_POWER, GAIN_RECORD_DTYPE, EditClip, ProgramLoudnessBank, edit_extent, edit_plan,
                                             edit_table)

LINES = []
YARDSTICK = "apply_gains out of place on the output's shape"


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


def shape(key, title, what, api, S, ch, cap, clips, n_out, args, out, tail=0):
    """S input streams of `cap` frames; the table renders n_out outputs whole (and `tail` frames of pad behind each), each in a row of
    the longest window's frames"""
    stream = torch.cuda.current_stream().cuda_stream
    table = edit_table(clips)
    extent = edit_extent(api, table, [cap] * S, n_out) + np.uint64(tail)
    out_cap = int(extent.max())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    f32_in = torch.empty((S * cap * ch,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    edit_out = torch.zeros((n_out * out_cap * ch,), device="cuda")
    yard_in = torch.empty((n_out * out_cap * ch,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    yard_out = torch.zeros((n_out * out_cap * ch,), device="cuda")
    g = np.zeros((n_out,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.5)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    out_frames = extent.astype(np.uint32)
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    bank.configure_edit(ch, n_out)
    yard = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), n_out, ch, 1)
    name = f"edit ({what})"
    arms = {YARDSTICK: lambda: yard.apply_gains(yard_in.data_ptr(), yard_out.data_ptr(), out_cap, ch, gains.data_ptr(), n_out,
                                                frames=out_frames, stream=stream),
            name: lambda: bank.edit(f32_in.data_ptr(), cap, table, edit_out.data_ptr(), out_cap, out_frames, stream=stream)}
    written = 4 * ch * int(extent.sum())
    read = 4 * ch * int(table["frames"].sum())
    counts = {YARDSTICK: {"bytes": 2 * written}, name: {"bytes": read + written, "clips": int(table.size), "tile_frames": int(edit_plan(api, ch)["tile_frames"])}}
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    ratio = (read + written) / (2.0 * written)
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
    rec = bank.fetch_edited(n_out - 1)
    say(f"    output {n_out - 1}: {int(rec['frames'])} frames, {int(rec['silent_frames'])} silent, {int(rec['faded_frames'])} faded, "
        f"{int(rec['mixed_frames'])} mixed, {int(rec['samples_over'])} over, peak {rec['out_sample_peak_db']:.3f} dB, {int(rec['clips'])} clips")
    bank.close()
    yard.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_edit.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_edit needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    for ch in (2, 8):
        clips = [EditClip(s, s, 0, 0, 16384, gain=0.5) for s in range(1024)]
        shape(f"a_1024x16384x{ch}", f"(a) 1024 x 16 384 frames, {ch} channels", "one whole-row clip per stream, gain 0.5", api, 1024, ch, 16384, clips,
              1024, args, out)
    long_ = 60 * 48000
    clips = [EditClip(s, s, 0, 0, long_) for s in range(64)]
    shape("b_64x60s", "(b) 64 x 60 s at 48 kHz stereo", "one whole clip per stream, gain 1: the copy path", api, 64, 2, long_, clips, 64, args, out)
    clips = [EditClip(s, s, 4801, 24000, long_ - 4801, 480, 480) for s in range(64)]
    shape("c_64x60s_trim", "(c) 64 x 60 s at 48 kHz stereo", "4801 frames trimmed at the head, fades of 10 ms, pads of 0.5 s in front and behind",
          api, 64, 2, long_, clips, 64, args, out, tail=24000)
    cross = 5 * 48000
    clips = []
    for o in range(8):
        at = 0
        for k in range(8):
            clips.append(EditClip(8 * o + k, o, 0, at, long_, cross if k else 0, cross if k < 7 else 0, EDIT_CURVE_EQUAL_POWER, EDIT_CURVE_EQUAL_POWER))
            at += long_ - cross
    shape("d_64into8", "(d) 64 x 60 s at 48 kHz stereo joined into 8 outputs", "equal-power crossfades of 5 s", api, 64, 2, long_, clips, 8, args, out)
    clips = [EditClip(s, s, 1, 0, long_ - 1) for s in range(64)]
    shape("e_64x60s_src1", "(e) 64 x 60 s at 48 kHz stereo", "one clip per stream from src_first 1, gain 1: the dword-load form", api, 64, 2, long_, clips,
          64, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

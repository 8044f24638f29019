"""Programme loudness bank, PCM formats (include/omx/program_pcm.h): what import_pcm and export_pcm cost beside apply_gains out of
place on the f32 side of the same shape.

The yardstick reads N and writes N bytes of f32; import and export move 0.75 (S16), 0.875 (S24) or 1.0 (S32) of those bytes.  Arms per
shape: apply_gains out of place; import_pcm in each format; export_pcm in each format without dither and with TPDF.  Shapes: 1024
streams x 8 ch x 16 384 frames (the project's loudness shape), the same ragged (per-stream frames uniform in [0, capacity]), and
64 x 2 ch x 60 s at 48 kHz.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms ALTERNATE (a b c a b c ...), and per arm the
line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those two is
the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_pcm.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_pcm.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import (DITHER_NONE, DITHER_TPDF, GAIN_RECORD_DTYPE, PCM_S16, PCM_S24, PCM_S32, ExportRule,
                                             ProgramLoudnessBank)

LINES = []
FORMATS = {"S16": (PCM_S16, 2), "S24": (PCM_S24, 3), "S32": (PCM_S32, 4)}
YARDSTICK = "apply_gains out of place (f32 to f32)"


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


def shape(key, title, api, S, ch, cap, args, out, ragged=False):
    stream = torch.cuda.current_stream().cuda_stream
    n = S * cap * ch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    f32_in = torch.empty((n,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    f32_out = torch.zeros((n,), device="cuda")
    pcm = torch.randint(0, 256, (n * 4,), device="cuda", dtype=torch.uint8, generator=gen)      # random bytes: every format reads its own share
    pcm_out = torch.zeros((n * 4,), device="cuda", dtype=torch.uint8)
    frames = np.random.default_rng(4).integers(0, cap + 1, S).astype(np.uint32) if ragged else None
    samples = ch * (int(frames.sum()) if ragged else S * cap)
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.7)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    arms = {YARDSTICK: lambda: bank.apply_gains(f32_in.data_ptr(), f32_out.data_ptr(), cap, ch, gains.data_ptr(), S, frames=frames, stream=stream)}
    moved = {YARDSTICK: 8 * samples}
    exporters = {}
    for name, (fmt, width) in FORMATS.items():
        arms[f"import_pcm {name}"] = lambda fmt=fmt: bank.import_pcm(pcm.data_ptr(), fmt, f32_out.data_ptr(), cap, ch, frames=frames, stream=stream)
        moved[f"import_pcm {name}"] = (4 + width) * samples
        for dname, dither in (("no dither", DITHER_NONE), ("TPDF", DITHER_TPDF)):
            ex = exporters[(name, dname)] = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
            ex.configure_export(ExportRule(fmt, dither, 1), ch)
            arms[f"export_pcm {name}, {dname}"] = lambda ex=ex: ex.export_pcm(f32_in.data_ptr(), pcm_out.data_ptr(), cap, frames=frames, stream=stream)
            moved[f"export_pcm {name}, {dname}"] = (4 + width) * samples
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    for name, r in t.items():
        ratio = f", {r['median'] / t[YARDSTICK]['median']:.3f} x the yardstick" if name != YARDSTICK else ""
        say(f"{title}, {name}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
            f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {moved[name] / (r['median'] * 1e-3) / 1e12:.2f} TB/s read + written{ratio}")
    rec = exporters[("S16", "TPDF")].fetch_exported(S - 1)
    say(f"    stream {S - 1}, S16 with TPDF: {int(rec['frames_out'])} frames out, {int(rec['samples_clipped'])} clipped, peak {rec['out_peak_db']:.3f} dB")
    out[key]["samples"] = samples
    bank.close()
    for ex in exporters.values():
        ex.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_pcm.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_pcm needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    shape("1024x8x16384", "1024 x 8 ch x 16 384 frames", api, 1024, 8, 16384, args, out)
    shape("1024x8x16384_ragged", "1024 x 8 ch x [0, 16 384] frames (ragged)", api, 1024, 8, 16384, args, out, ragged=True)
    shape("64x2x60s", "64 x 2 ch x 60 s at 48 kHz", api, 64, 2, 60 * 48000, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Programme loudness bank, peaks (include/omx/program_peaks.h): what measuring true peak and sample peak inside `process` costs,
against the only route to the same figure without it.

Variants, interleaved in one process on the same PCM, HIP events around each call:
  (a) process with peaks off
  (b) process with peaks on
  (c) process with peaks off + LoudnessBank.process_device over the same PCM in 256-frame blocks + note_snapshots
Per shape: median, min, max and the 10 % / 90 % points of each; (b) - (a) = the cost of the peak pass, and its rate as
S * frames * channels * 4 B over that time beside the 8 TB/s of the HBM.  The last line is one JSON object with every figure.
For the kernels' own times: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_peaks.py --reps 5"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import banks, capi
from openmeters_amd.program_loudness import ProgramLoudnessBank

SHAPES = {"64x2x60s@48k": (64, 2, 60 * 48000, 48000.0), "1024x8x16384@48k": (1024, 8, 16384, 48000.0), "64x2x60s@96k": (64, 2, 60 * 96000, 96000.0)}
HBM_BYTES_PER_S = 8.0e12
BLOCK = 256


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "p10": float(a[int(0.1 * (len(a) - 1))]),
            "p90": float(a[int(round(0.9 * (len(a) - 1)))])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_peaks needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name in args.shapes:
        S, ch, frames, fs = SHAPES[name]
        assert frames % BLOCK == 0
        pos = capi.SURROUND if ch == 8 else capi.positions_fallback(ch)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        pcm = torch.randn((S, frames, ch), device="cuda", generator=gen) * 0.1
        cfg = capi.LoudnessConfig(sample_rate=fs)
        seconds = int((args.reps + args.warmup + 1) * frames / fs) + 60       # every call adds its frames to the programmes
        off, on, off_c = (ProgramLoudnessBank(api, cfg, S, ch, seconds) for _ in range(3))
        on.set_peaks(True)
        meter = banks.LoudnessBank(api, cfg, S, ch)

        def a():
            off.process(pcm.data_ptr(), frames, ch, fs, pos, stream=stream)

        def b():
            on.process(pcm.data_ptr(), frames, ch, fs, pos, stream=stream)

        def c():
            off_c.process(pcm.data_ptr(), frames, ch, fs, pos, stream=stream)
            snaps = meter.process_device(pcm.data_ptr(), BLOCK, frames // BLOCK, ch, fs, pos, stream)
            off_c.note_snapshots(snaps, frames // BLOCK, stream=stream)

        variants = {"a_peaks_off": a, "b_peaks_on": b, "c_second_bank": c}
        times = {k: [] for k in variants}
        for rep in range(args.warmup + args.reps):
            for k, run in variants.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                run()
                stop.record()
                stop.synchronize()
                if rep >= args.warmup:
                    times[k].append(start.elapsed_time(stop))
        # same figure from both routes, on the last state
        same = all(np.float32(on.fetch(s).max_true_peak_db).tobytes() == np.float32(off_c.fetch(s).max_true_peak_db).tobytes() for s in range(0, S, max(S // 8, 1)))
        row = {k: stats(v) for k, v in times.items()}
        cost = row["b_peaks_on"]["median"] - row["a_peaks_off"]["median"]
        nbytes = S * frames * ch * 4
        row.update({"peak_pass_cost_ms": cost, "peak_pass_GBps": nbytes / (cost * 1e-3) / 1e9 if cost > 0 else None, "pcm_bytes": nbytes,
                    "share_of_hbm": nbytes / (cost * 1e-3) / HBM_BYTES_PER_S if cost > 0 else None, "reps": args.reps,
                    "b_below_c": row["b_peaks_on"]["median"] < row["c_second_bank"]["median"], "same_max_true_peak_db": bool(same)})
        out[name] = row
        for k in variants:
            r = row[k]
            print(f"{name} {k:14s}: median {r['median']:8.3f} ms  min {r['min']:8.3f}  p10 {r['p10']:8.3f}  p90 {r['p90']:8.3f}  max {r['max']:8.3f}  ({args.reps} reps)")
        print(f"{name} peak pass (b) - (a): {cost:.3f} ms = {nbytes / 1e9:.3f} GB of PCM at {row['peak_pass_GBps'] or float('nan'):.0f} GB/s "
              f"({100 * (row['share_of_hbm'] or float('nan')):.1f} % of 8 TB/s); (b) below (c): {row['b_below_c']}; "
              f"same max_true_peak_db from both routes: {same}")
        for bank in (off, on, off_c, meter):
            bank.close()
        del pcm
    print(json.dumps(out))


if __name__ == "__main__":
    main()

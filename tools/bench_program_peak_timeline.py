"""Programme loudness bank, peak timeline (include/omx/program_peak_timeline.h): what keeping the per-segment peaks costs inside
`process`, and what its readers cost.

Arms, alternated in one process on the same PCM, HIP events around `--calls` back-to-back calls after a warm-up:
  off: process with set_peaks(True)                      (the yardstick: the parent's code path)
  on : process with set_peaks(True) + set_peak_timeline(True)
Per shape: median, min, max of each arm, the ratio on / off of the medians and the spread of the off arm's repetitions.
Readers (`--readers`): peak_rows of 64 streams x 1 h at strides 1 and 10, the interval peak of one 24 h stream, the group peaks of 1024
one-track groups; each the median of `--reps` enqueued calls.  The last line is one JSON object with every figure.
For the kernels' own times: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_peak_timeline.py --reps 5"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import PEAK_ROW_DTYPE, TO_END, ProgramLoudnessBank

# (at 44.1 kHz a segment is 4410 frames, no multiple of a lane's run of 16: the only shape here whose segment boundaries cut runs)
SHAPES = {"1024x8x16384@48k": (1024, 8, 16384, 48000.0), "64x2x60s@48k": (64, 2, 60 * 48000, 48000.0), "64x2x60s@96k": (64, 2, 60 * 96000, 96000.0),
          "64x2x60s@44k1": (64, 2, 60 * 44100, 44100.0)}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1])}


def timed(run, reps, warmup):
    out = []
    for rep in range(warmup + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        stop.record()
        stop.synchronize()
        if rep >= warmup:
            out.append(start.elapsed_time(stop))
    return stats(out)


def process_arms(api, name, reps, warmup, calls, stream):
    S, ch, frames, fs = SHAPES[name]
    pos = capi.SURROUND if ch == 8 else capi.positions_fallback(ch)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    pcm = torch.randn((S, frames, ch), device="cuda", generator=gen) * 0.1
    cfg = capi.LoudnessConfig(sample_rate=fs)
    seconds = int((reps + warmup + 1) * calls * frames / fs) + 60       # every call adds its frames to the programmes
    banks = {"off": ProgramLoudnessBank(api, cfg, S, ch, seconds), "on": ProgramLoudnessBank(api, cfg, S, ch, seconds)}
    for bank in banks.values():
        bank.set_peaks(True)
    banks["on"].set_peak_timeline(True)
    times = {k: [] for k in banks}
    for rep in range(warmup + reps):
        for k, bank in banks.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                bank.process(pcm.data_ptr(), frames, ch, fs, pos, stream=stream)
            stop.record()
            stop.synchronize()
            if rep >= warmup:
                times[k].append(start.elapsed_time(stop) / calls)
    same = all(banks["on"].fetch_peaks(s).tobytes() == banks["off"].fetch_peaks(s).tobytes() for s in range(0, S, max(S // 8, 1)))
    row = {k: stats(v) for k, v in times.items()}
    row.update({"ratio_on_over_off": row["on"]["median"] / row["off"]["median"],
                "off_spread": (row["off"]["max"] - row["off"]["min"]) / row["off"]["median"], "reps": reps, "calls": calls,
                "same_peak_records": bool(same)})
    for k in banks:
        r = row[k]
        print(f"{name} process, timeline {k:3s}: median {r['median']:8.3f} ms per call  min {r['min']:8.3f}  max {r['max']:8.3f}  ({reps} reps of {calls} calls)")
    print(f"{name} on / off = {row['ratio_on_over_off']:.4f}; spread of the off arm (max - min) / median = {row['off_spread']:.4f}; "
          f"peak records equal: {same}")
    extra = None
    if S == 1024:       # the group peaks of 1024 one-track groups, on the programmes the arms have just fed
        members = [(s, 0, TO_END) for s in range(S)]
        groups = [(s, 1) for s in range(S)]
        extra = timed(lambda: banks["on"].measure_group_peaks(members, groups, stream=stream), reps, warmup)
        print(f"{name} group peaks, 1024 one-track groups of {banks['on'].fetch(0).segments} segments: median {extra['median']:.3f} ms "
              f"(host tables and upload included)  min {extra['min']:.3f}  max {extra['max']:.3f}")
    for bank in banks.values():
        bank.close()
    del pcm
    return row, extra


def readers(api, reps, warmup, stream):
    out = {}
    fs, ch = 48000.0, 2
    pos = capi.positions_fallback(ch)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    cfg = capi.LoudnessConfig(sample_rate=fs)
    # 64 streams x 1 h, fed a minute at a time
    S, minute = 64, 60 * 48000
    pcm = torch.randn((S, minute, ch), device="cuda", generator=gen) * 0.1
    bank = ProgramLoudnessBank(api, cfg, S, ch, 3600)
    bank.set_peaks(True)
    bank.set_peak_timeline(True)
    for _ in range(60):
        bank.process(pcm.data_ptr(), minute, ch, fs, pos, stream=stream)
    for stride in (1, 10):
        count = 36000 // stride
        d_rows = torch.empty((S * count * PEAK_ROW_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
        out[f"peak_rows_64x1h_stride{stride}"] = r = timed(lambda: bank.peak_rows(d_rows.data_ptr(), 0, stride, count, stream=stream), reps, warmup)
        print(f"peak_rows, 64 streams x 1 h, stride {stride:2d} ({count} rows per stream): median {r['median']:.3f} ms  min {r['min']:.3f}  max {r['max']:.3f}")
        del d_rows
    bank.close()
    # one stream x 24 h
    day = ProgramLoudnessBank(api, cfg, 1, ch, 86400)
    day.set_peaks(True)
    day.set_peak_timeline(True)
    for _ in range(24 * 60):
        day.process(pcm.data_ptr(), minute, ch, fs, pos, stream=stream)
    assert day.fetch(0).segments == 864000
    out["interval_peak_24h"] = r = timed(lambda: day.measure_interval_peaks([(0, 0, TO_END)], stream=stream), reps, warmup)
    print(f"interval peak, one stereo stream x 24 h (864 000 segments, one workgroup): median {r['median']:.3f} ms  min {r['min']:.3f}  max {r['max']:.3f}")
    day.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--readers", action="store_true")
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_peak_timeline needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name in args.shapes:
        out[name], extra = process_arms(api, name, args.reps, args.warmup, args.calls, stream)
        if extra:
            out["group_peaks_1024_one_track_groups"] = extra
    if args.readers:
        out.update(readers(api, args.reps, args.warmup, stream))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

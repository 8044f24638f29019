"""Programme loudness bank, bounded storage (include/omx/program_histogram.h): what the histogram fold adds to a process call and what
the result pass over the histograms costs, next to the stored mode on the same tree.

  live    : process of 1024 streams x 2 ch x 256 frames at 48 kHz, call after call; the calls that complete a segment (every 18th or
            19th: 4800 frames per segment) and those that complete none are reported apart
  long    : process of 64 streams x 10 min at 8 kHz mono in one call (the banks are reset, untimed, before every call)
  results : the result pass for 64 x 10 min and for 8 x 4 h
Each shape runs a stored bank and a bounded bank of this tree.  --parent-lib PATH also runs the stored bank of another build of the
library (the parent commit's) on `live` and on the 64 x 10 min result pass, alternated twice with this tree's in the same process.
HIP events around each call after 2 warm-up calls, 7 repetitions; per measurement the median with min and max.
The last line is one JSON object with every figure.
Kernels on their own, in a run of its own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_histogram.py --shapes live"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import ProgramLoudnessBank

FS8 = 8000.0


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "reps": len(ms)}


def show(name, t, unit="ms"):
    k = 1e3 if unit == "us" else 1.0
    print(f"{name}: median {t['median'] * k:.3f} {unit} [{t['min'] * k:.3f} ... {t['max'] * k:.3f}], {t['reps']} reps", flush=True)
    return t


def event_ms(run):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make(api, storage, fs, S, ch, seconds):
    if storage == "histogram":
        return ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, storage="histogram")
    return ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, seconds)


def live(api, storage, args, stream):
    """per-call times of the live cadence, apart for the calls that complete a segment and those that do not"""
    S, ch, n, fs, seg = 1024, 2, 256, 48000.0, 4800
    bank = make(api, storage, fs, S, ch, 60)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    pcm = 0.1 * torch.randn((S, n, ch), device="cuda", generator=gen)
    pos = capi.positions_fallback(ch)
    completes, none, k = [], [], 0
    while len(completes) < args.reps + args.warmup:
        ms = event_ms(lambda: bank.process(pcm.data_ptr(), n, ch, fs, pos, stream=stream))
        (completes if (k + 1) * n // seg > k * n // seg else none).append(ms)
        k += 1
    bank.close()
    return {"completes_a_segment": stats(completes[args.warmup:]), "completes_none": stats(none[args.warmup:])}


def stepped_noise(S, seconds):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    n, step = int(seconds * FS8), int(5 * FS8)
    steps = 10.0 ** (torch.empty((S, n // step + 1, 1), device="cuda").uniform_(-70.0, -10.0, generator=gen) / 20.0)
    return torch.randn((S, n, 1), device="cuda", generator=gen) * steps.repeat_interleave(step, dim=1)[:, :n], n


def long_call(api, storage, pcm, n, S, seconds, args, stream):
    """(times of the one-call process, the filled bank)"""
    bank = make(api, storage, FS8, S, 1, seconds)
    ms = []
    for _ in range(args.warmup + args.reps):
        bank.reset()
        torch.cuda.synchronize()
        ms.append(event_ms(lambda: bank.process(pcm.data_ptr(), n, 1, FS8, capi.positions_fallback(1), stream=stream)))
    assert bank.fetch(0).segments == seconds * 10
    return stats(ms[args.warmup:]), bank


def result_pass(bank, args, stream):
    ms = [event_ms(lambda: bank.results(stream)) for _ in range(args.warmup + args.reps)]
    return stats(ms[args.warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="live,long,results", help="comma-separated: live, long (with the 64 x 10 min result pass), results (8 x 4 h)")
    ap.add_argument("--parent-lib", default=None, help="another build of libomx_hip.so whose stored bank runs beside this tree's")
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_histogram needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    parent = capi.Api(args.parent_lib, "omx_") if args.parent_lib else None
    stream = torch.cuda.current_stream().cuda_stream
    shapes = args.shapes.split(",")
    out = {}

    if "live" in shapes:
        for storage in ("segments", "histogram"):
            t = live(api, storage, args, stream)
            out[f"live_{storage}"] = t
            for kind, v in t.items():
                show(f"live, 1024 x 2 ch x 256 frames, {storage}, call {kind.replace('_', ' ')}", v, "us")
        for kind in ("completes_a_segment", "completes_none"):
            d = out["live_histogram"][kind]["median"] - out["live_segments"][kind]["median"]
            out[f"live_fold_adds_us_{kind}"] = d * 1e3
            print(f"live: the bounded bank's call that {kind.replace('_', ' ')} takes {d * 1e3:+.1f} us against the stored bank's (medians)", flush=True)
        if parent:
            for turn in range(2):
                for name, lib in (("this tree", api), ("parent", parent)):
                    t = live(lib, "segments", args, stream)
                    out[f"live_segments_{name.replace(' ', '_')}_turn{turn}"] = t
                    for kind, v in t.items():
                        show(f"live, stored, {name}, turn {turn}, call {kind.replace('_', ' ')}", v, "us")

    if "long" in shapes:
        pcm, n = stepped_noise(64, 600)
        banks = {}
        for storage in ("segments", "histogram"):
            t, banks[storage] = long_call(api, storage, pcm, n, 64, 600, args, stream)
            out[f"long_64x10min_{storage}"] = show(f"process, 64 x 10 min at 8 kHz mono in one call, {storage}", t)
        out["long_fold_adds_us"] = (out["long_64x10min_histogram"]["median"] - out["long_64x10min_segments"]["median"]) * 1e3
        print(f"long: the bounded bank's call takes {out['long_fold_adds_us']:+.1f} us against the stored bank's (medians)", flush=True)
        for storage, bank in banks.items():
            out[f"results_64x10min_{storage}"] = show(f"result pass, 64 x 10 min, {storage}", result_pass(bank, args, stream))
        a, b = banks["segments"].fetch(0), banks["histogram"].fetch(0)
        print(f"stream 0: stored I {a.integrated_lufs:.4f} LRA {a.loudness_range_lu:.4f}; bounded I {b.integrated_lufs:.4f} LRA {b.loudness_range_lu:.4f}", flush=True)
        if parent:
            _, pbank = long_call(parent, "segments", pcm, n, 64, 600, args, stream)
            for turn in range(2):
                for name, bank in (("this tree", banks["segments"]), ("parent", pbank)):
                    out[f"results_64x10min_segments_{name.replace(' ', '_')}_turn{turn}"] = show(
                        f"result pass, 64 x 10 min, stored, {name}, turn {turn}", result_pass(bank, args, stream))
            pbank.close()
        for bank in banks.values():
            bank.close()
        del pcm

    if "results" in shapes:
        pcm, n = stepped_noise(8, 4 * 3600)
        for storage in ("segments", "histogram"):
            bank = make(api, storage, FS8, 8, 1, 4 * 3600)
            fill = event_ms(lambda: bank.process(pcm.data_ptr(), n, 1, FS8, capi.positions_fallback(1), stream=stream))
            assert bank.fetch(0).segments == 144000
            out[f"fill_8x4h_{storage}_ms"] = fill
            out[f"results_8x4h_{storage}"] = show(f"result pass, 8 x 4 h (filled in one call of {fill:.1f} ms), {storage}", result_pass(bank, args, stream))
            bank.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

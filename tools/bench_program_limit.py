"""Programme loudness bank, limiter (include/omx/program_limit.h): what apply_limited costs beside the two passes the bank already had
for the same bytes.

  yardstick = (process with peaks on - process with peaks off) + apply_gains out of place
      the peak pass reads the PCM once and runs the interpolator the limiter's level pass runs; apply_gains reads and writes it once.
      Neither is touched by the limiter, so this tree's library measures what the parent commit's would.
  apply_limited in its steady state: every call brings frames_capacity frames per stream and emits as many (no flush, no reset; the
      streams keep running), ceiling -1 dBTP, attack 64 frames, hold 480 frames.
on 64 streams x 2 ch x 60 s at 48 kHz and on 1024 x 8 ch x 16 384 frames.  Both process arms reset every stream in every call, so
that no stream fills its capacity; the reset is in both and leaves their difference alone.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms ALTERNATE (a b c d a b c d ...), and per arm the
line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those two is the
spread of the run.  The lines go to --out (default profiles/program_limit.txt) as well; the last line printed is one JSON object.
The passes on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_limit.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, LimitRule, ProgramLoudnessBank

LINES = []
RULE = LimitRule(-1.0, 64, 480)


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


def shape(key, title, api, S, ch, cap, fs, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    d_in = torch.empty((S, cap, ch), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    d_out = torch.zeros((S, cap, ch), device="cuda")
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(1.0)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    pos, resets = capi.positions_fallback(ch), [1] * S
    seconds = int(cap / fs) + 2
    plain = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, seconds)
    peaks = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, seconds)
    peaks.set_peaks(True)
    limiter = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, ch, 1)
    limiter.configure_limiter(RULE, ch, fs)
    arms = {"process, peaks off": lambda: plain.process(d_in.data_ptr(), cap, ch, fs, pos, reset_mask=resets, stream=stream),
            "process, peaks on": lambda: peaks.process(d_in.data_ptr(), cap, ch, fs, pos, reset_mask=resets, stream=stream),
            "apply_gains out of place": lambda: limiter.apply_gains(d_in.data_ptr(), d_out.data_ptr(), cap, ch, gains.data_ptr(), S, stream=stream),
            "apply_limited": lambda: limiter.apply_limited(d_in.data_ptr(), cap, d_out.data_ptr(), cap, gains.data_ptr(), S, stream=stream)}
    t = alternated(arms, args.warmup, args.reps, args.inner)
    for name, r in t.items():
        say(f"{title}, {name}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
            f"{r['median_even']:.4f} / {r['median_odd']:.4f})")
    peak_pass = t["process, peaks on"]["median"] - t["process, peaks off"]["median"]
    yardstick = peak_pass + t["apply_gains out of place"]["median"]
    ratio = t["apply_limited"]["median"] / yardstick
    say(f"{title}: peak pass {peak_pass:.4f} ms + apply_gains {t['apply_gains out of place']['median']:.4f} ms = yardstick {yardstick:.4f} ms; "
        f"apply_limited {t['apply_limited']['median']:.4f} ms = {ratio:.3f} x the yardstick")
    rec = limiter.fetch_limited(S - 1)
    say(f"    stream {S - 1}: {int(rec['frames_in'])} frames in, {int(rec['frames_out'])} out, {int(rec['frames_limited'])} limited, "
        f"deepest reduction {rec['max_reduction_db']:.2f} dB, output sample peak {rec['out_sample_peak_db']:.3f} dB")
    t["peak_pass_ms"], t["yardstick_ms"], t["ratio"] = peak_pass, yardstick, ratio
    out[key] = t
    for bank in (plain, peaks, limiter):
        bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_limit.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_limit needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    say(f"limiter: ceiling {RULE.ceiling_db} dBTP, attack {RULE.attack_frames} frames, hold {RULE.release_hold_frames} frames")
    shape("64x2x60s", "64 x 2 ch x 60 s at 48 kHz", api, 64, 2, 60 * 48000, 48000.0, args, out)
    shape("1024x8x16384", "1024 x 8 ch x 16 384 frames at 48 kHz", api, 1024, 8, 16384, 48000.0, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

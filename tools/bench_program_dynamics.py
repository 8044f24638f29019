"""Programme loudness bank, dynamics (include/omx/program_dynamics.h): what a dynamics call costs beside apply_limited on the same
shapes and in the same run.

  yardstick = apply_limited in its steady state (ceiling -1 dBTP, attack 64 frames, hold 480 frames, unity gain)
  dynamics  = a 4:1 compressor at -20 dB with a 6 dB knee, attack 64 frames, hold 480 frames, release 60 dB/s, in its steady state:
      every call brings frames_capacity frames per stream and emits as many (no flush, no reset; the streams keep running), once
      without and once with the gain trace.
on 64 streams x 2 ch x 60 s at 48 kHz and on 1024 x 8 ch x 16 384 frames.  The input is noise at -40 dB with a burst at -6 dB in one
tenth of a second out of four, so that the gain falls and is released all along the programme.
The dynamics call has a cheaper level pass than the limiter (no 4x interpolation) and one pass more (the release scan moves one int64
per frame out and in), so the bar is apply_limited's time plus the time of the limiter's smooth pass, the pass whose traffic the scan
repeats; both are read from one kernel trace of this run:
    rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_dynamics.py --reps 3
The last section shows that a single long stream is time-parallel: 1 stream x 2 ch x 10 min beside 64 streams of the same total frames.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms ALTERNATE, and per arm the line gives the median
per call with min and max and the medians of its even and odd repetitions.  The lines go to --out (default
profiles/program_dynamics.txt) as well; the last line printed is one JSON object."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import (GAIN_RECORD_DTYPE, DynamicsCurve, DynamicsSpec, LimitRule, ProgramLoudnessBank, dynamics_design,
                                             dynamics_time)
from bench_program_limit import alternated

LINES = []
RULE = LimitRule(-1.0, 64, 480)
FS = 48000.0


def say(line):
    print(line, flush=True)
    LINES.append(line)


def bursty(S, cap, ch):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    x = torch.empty((S, cap, ch), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    loud = ((torch.arange(cap, device="cuda") // 4800) % 4 == 0).to(torch.float32) * 0.49 + 0.01
    return (x * loud[None, :, None]).contiguous()


def curve_of(api, ch, attack, hold, step):
    return DynamicsCurve(dynamics_design(api, DynamicsSpec(-20.0, 4.0, 6.0)), (1 << ch) - 1, attack, hold, step)


def line(title, name, r):
    say(f"{title}, {name}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
        f"{r['median_even']:.4f} / {r['median_odd']:.4f})")


def shape(key, title, api, S, ch, cap, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    d_in, d_out = bursty(S, cap, ch), torch.zeros((S, cap, ch), device="cuda")
    d_trace = torch.zeros((S, cap), device="cuda")
    g = np.zeros((S,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(1.0)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    limiter = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, ch, 1)
    limiter.configure_limiter(RULE, ch, FS)
    dyn = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, ch, 1)
    _a, _h, step = dynamics_time(api, FS, 1.0, 10.0, 60.0)
    c = curve_of(api, ch, 64, 480, step)
    dyn.configure_dynamics([c], ch)
    traced = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, ch, 1)
    traced.configure_dynamics([c], ch)
    arms = {"apply_limited": lambda: limiter.apply_limited(d_in.data_ptr(), cap, d_out.data_ptr(), cap, gains.data_ptr(), S, stream=stream),
            "dynamics": lambda: dyn.dynamics(d_in.data_ptr(), cap, d_out.data_ptr(), cap, stream=stream),
            "dynamics with the gain trace": lambda: traced.dynamics(d_in.data_ptr(), cap, d_out.data_ptr(), cap, d_gain_db=d_trace.data_ptr(),
                                                                    stream=stream)}
    t = alternated(arms, args.warmup, args.reps, args.inner)
    for name, r in t.items():
        line(title, name, r)
    ratio = t["dynamics"]["median"] / t["apply_limited"]["median"]
    bytes_moved = S * cap * ch * 8
    say(f"{title}: dynamics {t['dynamics']['median']:.4f} ms = {ratio:.3f} x apply_limited {t['apply_limited']['median']:.4f} ms; "
        f"{bytes_moved / t['dynamics']['median'] / 1e6:.1f} GB/s of PCM read and written")
    rec = dyn.fetch_dynamics(S - 1)
    say(f"    stream {S - 1}: {int(rec['frames_in'])} frames in, {int(rec['frames_out'])} out, {int(rec['frames_reduced'])} reduced, "
        f"deepest gain {rec['min_gain_db']:.2f} dB, output sample peak {rec['out_sample_peak_db']:.3f} dB")
    t["ratio_to_apply_limited"] = ratio
    out[key] = t
    for bank in (limiter, dyn, traced):
        bank.close()


def long_stream(api, args, out):
    """one stream of 10 minutes beside 64 streams of the same total frames: the only serial part is one carry per release tile"""
    stream = torch.cuda.current_stream().cuda_stream
    ch, total = 2, 600 * 48000
    _a, _h, step = dynamics_time(api, FS, 1.0, 10.0, 60.0)
    c = curve_of(api, ch, 64, 480, step)
    arms, keep = {}, []
    for S in (1, 64):
        cap = total // S
        d_in, d_out = bursty(S, cap, ch), torch.zeros((S, cap, ch), device="cuda")
        bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, ch, 1)
        bank.configure_dynamics([c], ch)
        keep.append((d_in, d_out, bank))
        arms[f"{S} x 2 ch x {cap} frames"] = (lambda b=bank, i=d_in, o=d_out, n=cap: b.dynamics(i.data_ptr(), n, o.data_ptr(), n, stream=stream))
    t = alternated(arms, args.warmup, args.reps, args.inner)
    for name, r in t.items():
        line("28.8 M frames", name, r)
    names = list(t)
    say(f"one 10 min stream takes {t[names[0]]['median'] / t[names[1]]['median']:.3f} x the time of 64 streams of the same total frames")
    out["long_stream"] = t
    for _i, _o, bank in keep:
        bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_dynamics.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_dynamics needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    say("dynamics: 4:1 at -20 dB, knee 6 dB, attack 64 frames, hold 480 frames, release 60 dB/s; "
        f"limiter: ceiling {RULE.ceiling_db} dBTP, attack {RULE.attack_frames} frames, hold {RULE.release_hold_frames} frames")
    shape("64x2x60s", "64 x 2 ch x 60 s at 48 kHz", api, 64, 2, 60 * 48000, args, out)
    shape("1024x8x16384", "1024 x 8 ch x 16 384 frames at 48 kHz", api, 1024, 8, 16384, args, out)
    long_stream(api, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

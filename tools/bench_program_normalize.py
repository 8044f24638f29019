"""Programme loudness bank, normalisation (include/omx/program_normalize.h): what apply_gains costs beside the copy of the same
bytes, and what plan_gains adds to the result pass.

  (a) apply_gains, out of place and in place, beside hipMemcpyDtoDAsync of the same bytes (a copy reads N and writes N bytes: exactly
      the pass's compulsory traffic), on 1024 streams x 8 ch x 16 384 frames (the project's loudness shape) and 64 x 2 ch x 60 s at
      48 kHz; the first shape also ragged (per-stream frames uniform in [0, capacity], the copy then moves the same total), and with
      d_in one float off its 16-byte boundary (the dword-load form of the kernel)
  (b) plan_gains for 1024 streams beside results() alone
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms of a comparison ALTERNATE (a b a b ...), and
per arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between
those two is the spread of the run, and an arm is slower than another only beyond it.
--tuning-lib PATH adds the out-of-place pass of the tuning library (make TUNING=1) with plain and with non-temporal stores
(OMX_NORMALIZE_STORES=nt, read by that library only), alternated with the rest.  --other-lib NAME=PATH (repeatable) runs the result
pass of another build of the library in (b): that is how the parent commit's result pass is measured beside this tree's.
The lines go to --out (default profiles/program_normalize.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_normalize.py --reps 3"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import GAIN_RECORD_DTYPE, GainRule, ProgramLoudnessBank

LINES = []


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


def show(title, t, moved_bytes=None, yardstick=None):
    for name, r in t.items():
        rate = f", {moved_bytes / (r['median'] * 1e-3) / 1e12:.2f} TB/s read + written" if moved_bytes else ""
        ratio = f", {r['median'] / t[yardstick]['median']:.3f} x the copy" if yardstick and name != yardstick else ""
        say(f"{title}, {name}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
            f"{r['median_even']:.4f} / {r['median_odd']:.4f}){rate}{ratio}")


def device_copy():
    """hipMemcpyDtoDAsync of the HIP runtime the process has already loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    fn = C.CDLL(path).hipMemcpyDtoDAsync
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int
    return fn


def gains_on_device(n):
    g = np.zeros((n,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(10.0 ** (-3.0 / 20.0)) * (1.0 - 0.0002 * np.arange(n, dtype=np.float32))      # below 1: the in-place arm scales its buffer again and again
    return torch.from_numpy(g.view(np.uint8).copy()).cuda()


def apply_shape(key, title, api, tuning, S, ch, cap, args, out, ragged=False, misaligned=False):
    stream = torch.cuda.current_stream().cuda_stream
    copy = device_copy()
    n = S * cap * ch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    store_in = torch.empty((n + 4,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    store_out, store_place = torch.zeros((n + 4,), device="cuda"), store_in.clone()
    d_in, d_out, d_place = store_in.data_ptr() + (4 if misaligned else 0), store_out.data_ptr(), store_place.data_ptr()
    frames = np.random.default_rng(4).integers(0, cap + 1, S).astype(np.uint32) if ragged else None
    moved = 2 * 4 * ch * (int(frames.sum()) if ragged else S * cap)
    gains = gains_on_device(S)
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)
    arms = {"hipMemcpyDtoDAsync of the same bytes": lambda: copy(d_out, d_in, moved // 2, C.c_void_p(stream)),
            "apply_gains out of place": lambda: bank.apply_gains(d_in, d_out, cap, ch, gains.data_ptr(), S, frames=frames, stream=stream)}
    if not misaligned:
        arms["apply_gains in place"] = lambda: bank.apply_gains(d_place, d_place, cap, ch, gains.data_ptr(), S, frames=frames, stream=stream)
    tbank = None
    if tuning is not None and not misaligned:
        tbank = ProgramLoudnessBank(tuning, capi.LoudnessConfig(sample_rate=48000.0), S, ch, 1)

        def with_stores(kind):
            os.environ["OMX_NORMALIZE_STORES"] = kind
            tbank.apply_gains(d_in, d_out, cap, ch, gains.data_ptr(), S, frames=frames, stream=stream)
        arms["tuning library, out of place, plain stores"] = lambda: with_stores("plain")
        arms["tuning library, out of place, non-temporal stores"] = lambda: with_stores("nt")
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    out[key]["bytes_read_and_written"] = moved
    show(title, {k: v for k, v in t.items() if isinstance(v, dict)}, moved, "hipMemcpyDtoDAsync of the same bytes")
    rec = bank.fetch_applied(S - 1)
    say(f"    stream {S - 1}: {int(rec['frames'])} frames by {rec['gain']:.6f}, {int(rec['samples_over'])} samples over, peak {rec['out_sample_peak_db']:.3f} dB")
    bank.close()
    if tbank is not None:
        tbank.close()


def plan_beside_results(apis, args, out):
    stream = torch.cuda.current_stream().cuda_stream
    S, fs, seconds = 1024, 8000.0, 60
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    n, step = int(seconds * fs), int(5 * fs)
    steps = 10.0 ** (torch.empty((S, n // step + 1, 1), device="cuda").uniform_(-70.0, -10.0, generator=gen) / 20.0)
    pcm = torch.randn((S, n, 1), device="cuda", generator=gen) * steps.repeat_interleave(step, dim=1)[:, :n]
    banks, arms = {}, {}
    rule = GainRule(-23.0, -1.0, -20.0, 20.0, 1)
    for name, api in apis.items():
        banks[name] = bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=fs), S, 1, seconds)
        bank.set_peaks(True)
        bank.process(pcm.data_ptr(), n, 1, fs, capi.positions_fallback(1), stream=stream)
        torch.cuda.synchronize()
        arms[f"results, {name}"] = lambda bank=bank: bank.results(stream=stream)
        if api.has("program_loudness_bank_plan_gains"):
            arms[f"plan_gains alone (records fresh), {name}"] = lambda bank=bank: bank.plan_gains(rule, stream=stream)
            arms[f"results then plan_gains, {name}"] = lambda bank=bank: (bank.results(stream=stream), bank.plan_gains(rule, stream=stream))
    out["b_plan_1024_streams"] = t = alternated(arms, args.warmup, args.reps, args.inner)
    show("(b) 1024 streams x 1 min", t)
    g = banks["this tree"].fetch_gains()
    say(f"    gains: {float(g['gain_db'].min()):.2f} ... {float(g['gain_db'].max()):.2f} dB, limited by "
        f"{np.bincount(g['limited_by'], minlength=5).tolist()} (target, peak, max, min, no measurement)")
    for bank in banks.values():
        bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--tuning-lib", default=None, help="libomx_hip_tuning.so: adds the plain / non-temporal store A/B")
    ap.add_argument("--other-lib", action="append", default=[], metavar="NAME=PATH", help="another build of libomx_hip.so beside this tree's in (b)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_normalize.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_normalize needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    tuning = capi.Api(args.tuning_lib, "omx_") if args.tuning_lib else None
    apis = {"this tree": api}
    for spec in args.other_lib:
        name, path = spec.split("=", 1)
        apis[name] = capi.Api(path, "omx_")
    out = {}
    apply_shape("a_1024x8x16384", "(a) 1024 x 8 ch x 16 384 frames", api, tuning, 1024, 8, 16384, args, out)
    apply_shape("a_1024x8x16384_ragged", "(a) 1024 x 8 ch x [0, 16 384] frames (ragged)", api, tuning, 1024, 8, 16384, args, out, ragged=True)
    apply_shape("a_1024x8x16384_misaligned_loads", "(a) 1024 x 8 ch x 16 384 frames, d_in 4 bytes off a 16-byte boundary", api, None, 1024, 8, 16384,
                args, out, misaligned=True)
    apply_shape("a_64x2x60s", "(a) 64 x 2 ch x 60 s at 48 kHz", api, tuning, 64, 2, 60 * 48000, args, out)
    plan_beside_results(apis, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

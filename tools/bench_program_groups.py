"""Programme loudness bank, groups (include/omx/program_groups.h): what the record of an album costs, from segments (or histograms)
that are already stored.

  (a) one-member groups against measure_intervals of the same 4096 intervals (30 s ... 10 min over a 64 x 10 min bank): the same work
      through the group kernel and through the interval kernel
  (b) one album of 12 x 5 min and one of 8 x 4 h, beside the per-stream result pass (results()) over the same banks
  (c) one bounded group of 1024 streams, beside the per-stream result pass of that bounded bank
HIP events around each call after a warm-up, one process.  The arms of a comparison ALTERNATE (a b a b ...), and per arm the line
gives the median with min and max and the medians of its even and odd repetitions: the distance between those two is the spread of
the run, and an arm is slower than another only beyond it.
--other-lib NAME=PATH (repeatable) runs another build of the library beside this tree's in (b), alternated with it in the same
process: its per-stream result pass and, when it has the group interface, its group call.  That is how the per-stream pass of the
parent commit and the group kernel without staging (the tuning library with OMX_GROUPS_STAGING=0) are measured.
The banks are filled at 8 kHz mono (stepped noise): the result passes read the segment energies or histograms only.
The last line is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_groups.py --reps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import TO_END, ProgramLoudnessBank

FS = 8000.0


def alternated(arms, warm, reps):
    """arms: name -> callable.  Every repetition runs each arm once, in turn, each between its own pair of events"""
    for _ in range(warm):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(reps):
        for name, run in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    out = {}
    for name, v in ms.items():
        s = sorted(v)
        out[name] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "reps": reps, "median_even": float(np.median(v[0::2])),
                     "median_odd": float(np.median(v[1::2])) if reps > 1 else s[0]}
    return out


def show(title, t):
    for name, r in t.items():
        print(f"{title}, {name}: median {r['median']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}, {r['reps']} reps; even / odd repetitions "
              f"{r['median_even']:.3f} / {r['median_odd']:.3f})", flush=True)


def filled_banks(apis, S, seconds, stream, storage="segments"):
    """per library a bank of S programmes of `seconds` of noise whose level steps every 5 s between -70 and -10 dBFS (the same PCM)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    n, step = int(seconds * FS), int(5 * FS)
    steps = 10.0 ** (torch.empty((S, n // step + 1, 1), device="cuda").uniform_(-70.0, -10.0, generator=gen) / 20.0)
    pcm = torch.randn((S, n, 1), device="cuda", generator=gen) * steps.repeat_interleave(step, dim=1)[:, :n]
    banks = {}
    for name, api in apis.items():
        banks[name] = bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, 1, seconds, storage=storage)
        bank.process(pcm.data_ptr(), n, 1, FS, capi.positions_fallback(1), stream=stream)
        torch.cuda.synchronize()
        assert bank.fetch(0).segments == seconds * 10
    return banks


def album(banks, S, stream):
    """the arms of one album: per library the per-stream result pass and, where the library has it, one group of all streams"""
    members = ProgramLoudnessBank._intervals([(s, 0, TO_END) for s in range(S)])
    groups = ProgramLoudnessBank._groups([(0, S)])
    arms = {}
    for name, bank in banks.items():
        arms[f"per-stream result pass, {name}"] = lambda bank=bank: bank.results(stream=stream)
        if bank.api.has("program_loudness_bank_measure_groups"):
            arms[f"one group of all streams, {name}"] = lambda bank=bank: bank.measure_groups(members, groups, stream=stream)
    return arms


def close(banks):
    for bank in banks.values():
        bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--other-lib", action="append", default=[], metavar="NAME=PATH", help="another build of libomx_hip.so beside this tree's in (b)")
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_groups needs a gfx950 device: there is no CPU fallback"
    this = {"this tree": openmeters_amd.api()}
    apis = dict(this)
    for spec in args.other_lib:
        name, path = spec.split("=", 1)
        apis[name] = capi.Api(path, "omx_")
    stream = torch.cuda.current_stream().cuda_stream
    out = {}

    bank = filled_banks(this, 64, 600, stream)["this tree"]
    rng = np.random.default_rng(5)
    intervals = []
    for _ in range(4096):
        c = int(rng.integers(300, 6001))
        intervals.append((int(rng.integers(0, 64)), int(rng.integers(0, 6000 - c + 1)), c))
    packed = ProgramLoudnessBank._intervals(intervals)
    singles = ProgramLoudnessBank._groups([(i, 1) for i in range(len(intervals))])
    t = alternated({"measure_intervals": lambda: bank.measure_intervals(packed, stream=stream),
                    "one-member groups": lambda: bank.measure_groups(packed, singles, stream=stream)}, args.warmup, args.reps)
    assert bank.fetch_groups(packed, singles).tobytes() == bank.fetch_intervals(packed).tobytes()
    out["a_4096_one_member_groups_over_64x10min"] = t
    show("(a) 4096 parts of 30 s ... 10 min over 64 x 10 min", t)
    bank.close()

    for key, title, S, seconds in (("b_album_12x5min", "(b) 12 x 5 min (36 000 segments)", 12, 300),
                                   ("b_album_8x4h", "(b) 8 x 4 h (1 152 000 segments)", 8, 4 * 3600)):
        banks = filled_banks(apis, S, seconds, stream)
        out[key] = t = alternated(album(banks, S, stream), args.warmup, args.reps)
        show(title, t)
        recs = {name: b.fetch_groups([(s, 0, TO_END) for s in range(S)], [(0, S)])[0] for name, b in banks.items()
                if b.api.has("program_loudness_bank_measure_groups")}
        rec = recs["this tree"]
        assert all(r.tobytes() == rec.tobytes() for r in recs.values())      # staged or not, the same bytes
        print(f"    the album: I {rec['integrated_lufs']:.3f} LUFS, LRA {rec['loudness_range_lu']:.3f} LU, "
              f"{int(rec['gating_above_relative'])}/{int(rec['gating_blocks'])} gating blocks", flush=True)
        close(banks)

    banks = filled_banks(this, 1024, 60, stream, storage="histogram")
    out["c_bounded_group_of_1024"] = t = alternated(album(banks, 1024, stream), args.warmup, args.reps)
    show("(c) bounded bank, 1024 streams x 1 min", t)
    close(banks)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

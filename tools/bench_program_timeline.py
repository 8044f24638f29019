"""Programme loudness bank, timeline and intervals (include/omx/program_timeline.h): what the loudness log and the records of parts
of a programme cost, from segments that are already stored.

  timeline : 64 streams x 10 min (6000 segments) at stride 1; 8 streams x 4 h (144 000 segments) at stride 1 and at stride 10
  intervals: 4096 intervals of 30 s ... 10 min over the 64 x 10 min bank
HIP events around each call after a warm-up, one process; per measurement the median with min and max.  Beside each timeline time:
the count of block visits of the all-pairs pass, sum over the streams of segments^2 / (2 stride), and the time that count takes at
the VALU issue rate (3.93e13 lane-instructions per second: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz, the way DESIGN.md prices by issue)
with the instructions per visit read from the ISA of tl_rows_kernel's inner loop (VALU_PER_VISIT below).
The banks are filled at 8 kHz mono (stepped noise): the timeline and the intervals read the segment energies only.
The last line is one JSON object with every figure.
The two kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_timeline.py --reps 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.program_loudness import TIMELINE_ROW_DTYPE, ProgramLoudnessBank

FS = 8000.0
ISSUE_RATE = 3.93e13
# tl_rows_kernel, the loop over a tile that lies wholly before the wavefront's rows, per block visit: v_cmp_gt_f64, two v_cndmask_b32
# (the value or 0.0), v_add_f64, one v_cndmask_b32 and half a v_add3_u32 (the count) = 5.5 VALU; an eighth of a ds_read_b128 beside them
VALU_PER_VISIT = 5.5


def timed(run, warm, reps):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "reps": reps}


def filled_bank(api, S, seconds, stream):
    """S programmes of `seconds` of noise whose level steps every 5 s between -70 and -10 dBFS"""
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=FS), S, 1, seconds)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    n, step = int(seconds * FS), int(5 * FS)
    steps = 10.0 ** (torch.empty((S, n // step + 1, 1), device="cuda").uniform_(-70.0, -10.0, generator=gen) / 20.0)
    pcm = torch.randn((S, n, 1), device="cuda", generator=gen) * steps.repeat_interleave(step, dim=1)[:, :n]
    bank.process(pcm.data_ptr(), n, 1, FS, capi.positions_fallback(1), stream=stream)
    torch.cuda.synchronize()
    assert bank.fetch(0).segments == seconds * 10
    return bank


def timeline_row(name, bank, S, segments, stride, args, stream):
    count = (segments + stride - 1) // stride
    rows = torch.empty((S * count * TIMELINE_ROW_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    t = timed(lambda: bank.timeline(rows.data_ptr(), 0, stride, count, stream=stream), args.warmup, args.reps)
    visits = S * segments * segments / (2.0 * stride)
    t.update({"block_visits": visits, "valu_per_visit": VALU_PER_VISIT, "issue_bound_ms": visits * VALU_PER_VISIT / ISSUE_RATE * 1e3, "rows": S * count})
    last = rows.cpu().numpy().view(TIMELINE_ROW_DTYPE).reshape(S, count)[0, -1]
    print(f"timeline {name}, stride {stride}: median {t['median']:.3f} ms (min {t['min']:.3f}, max {t['max']:.3f}, {args.reps} reps); "
          f"{visits:.3e} block visits x {VALU_PER_VISIT} VALU = {t['issue_bound_ms']:.3f} ms at the issue rate "
          f"({100 * t['issue_bound_ms'] / t['median']:.0f} % of it); stream 0, last row: I {last['integrated_lufs']:.3f} LUFS, "
          f"{last['gating_above_relative']}/{last['gating_above_absolute']} blocks", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement of one 6000-segment timeline on this node's CPU (context)")
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_timeline needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    bank = filled_bank(api, 64, 600, stream)
    out["timeline_64x10min_stride1"] = timeline_row("64 x 10 min", bank, 64, 6000, 1, args, stream)
    rng = np.random.default_rng(5)
    intervals = []
    for _ in range(4096):
        c = int(rng.integers(300, 6001))
        intervals.append((int(rng.integers(0, 64)), int(rng.integers(0, 6000 - c + 1)), c))
    packed = ProgramLoudnessBank._intervals(intervals)
    t = timed(lambda: bank.measure_intervals(packed, stream=stream), args.warmup, args.reps)
    t["segments_read"] = int(sum(c for _, _, c in intervals))
    out["intervals_4096_over_64x10min"] = t
    print(f"intervals, 4096 of 30 s ... 10 min over 64 x 10 min ({t['segments_read']} segments in all): median {t['median']:.3f} ms "
          f"(min {t['min']:.3f}, max {t['max']:.3f}, {args.reps} reps)", flush=True)
    if args.cpu:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import program_timeline_ref as tl
        e = bank.fetch_segments(0)
        t0 = time.perf_counter()
        tl.timeline(e)
        out["numpy_restatement_one_stream_6000_s"] = time.perf_counter() - t0
        print(f"numpy restatement, one stream of 6000 segments at stride 1: {out['numpy_restatement_one_stream_6000_s']:.2f} s on the CPU (context)", flush=True)
    bank.close()
    bank = filled_bank(api, 8, 4 * 3600, stream)
    out["timeline_8x4h_stride1"] = timeline_row("8 x 4 h", bank, 8, 144000, 1, args, stream)
    out["timeline_8x4h_stride10"] = timeline_row("8 x 4 h", bank, 8, 144000, 10, args, stream)
    bank.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Programme loudness bank, mix pass (include/omx/program_mix.h): what `mix` costs beside apply_gains out of place on the OUTPUT's
shape, and beside the chain of edit calls it replaces.

Yardstick 1 reads N and writes N bytes of f32, N the bytes of the mix's output windows: the family's stand-in for a device-to-device
copy, 8 B per sample.  A mix of L full layers writes N and reads L N, 4 (L + 1) B per sample; `x yardstick x (L + 1) / 2` is the time
of the mix over the time a pass as good as the yardstick would take for those bytes: the aim is 1.0.
Yardstick 2 is the chain: L - 1 edit calls, each adding one more source to the running sum through two scratch buffers that take
turns, 12 (L - 1) B per sample.
Arms.  (a) 1024 buses x 16 384 frames at 2 and at 8 channels, L = 1, 2, 4, 8, 16 whole-row sends per bus from L distinct input
streams, gains 0.5 (the yardstick's own gain); at 2 channels also the chains of L = 4 and 8, and L = 4 with src_first = 1 (every
source 8 bytes off a 16-byte boundary: the same 16-byte loads at unaligned addresses).  (b) 64 x 60 s at 48 kHz stereo into 8 buses, 8 layers each, and its
chain.  (c) the host: wall time of a call that renders no frame (validation, spans, blob, upload, two small launches) for 1024 buses
x 8 sends.
HIP events around `--inner` back-to-back calls after a warm-up, one process.  The arms of a shape ALTERNATE (a b c a b c ...), and per
arm the line gives the median per call with min and max and the medians of its even and odd repetitions: the distance between those
two is the spread of the run, and an arm is slower than another only beyond it.
The lines go to --out (default profiles/program_mix.txt) as well; the last line printed is one JSON object with every figure.
The kernels on their own: rocprofv3 --kernel-trace --stats -- python3 tools/bench_program_mix.py --reps 3"""
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
from openmeters_amd.program_loudness import (EDIT_CLIP_DTYPE, GAIN_RECORD_DTYPE, MIX_SEND_DTYPE, ProgramLoudnessBank, mix_plan)

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


def mix_sends(n_out, max_layers, layers, frames, src_first=0):
    """bus o takes input streams o * max_layers + l, l < layers, whole rows"""
    t = np.zeros((n_out, layers), MIX_SEND_DTYPE)
    t["dst_bus"] = np.arange(n_out)[:, None]
    t["src_stream"] = np.arange(n_out)[:, None] * max_layers + np.arange(layers)[None, :]
    t["src_first"] = src_first
    t["frames"] = frames
    t["gain"] = np.float32(0.5)
    return t.reshape(-1)


def chain_tables(n_out, max_layers, layers, frames, n_sources):
    """The edit calls that add layer after layer.  The device row order is [scratch A x n_out][sources][scratch B x n_out]; call k
    reads through a d_in that starts at A (streams: A, then the sources) or at the sources (streams: the sources, then B) and writes
    the other scratch.  -> list of (d_in starts at A?, clip table)"""
    calls = []
    for k in range(1, layers):
        from_a = k % 2 == 0      # call 1 writes A, call 2 reads A and writes B, ...
        t = np.zeros((n_out, 2), EDIT_CLIP_DTYPE)
        t["dst_stream"] = np.arange(n_out)[:, None]
        t["frames"] = frames
        t["gain"] = np.float32(0.5)
        source_base = n_out if from_a else 0
        if k == 1:
            t["src_stream"][:, 0] = np.arange(n_out) * max_layers
        else:
            t["src_stream"][:, 0] = np.arange(n_out) if from_a else n_sources + np.arange(n_out)
            t["gain"][:, 0] = np.float32(1.0)
        t["src_stream"][:, 1] = source_base + np.arange(n_out) * max_layers + k
        calls.append((from_a, t.reshape(-1)))
    return calls


def shape(key, title, api, n_out, ch, frames, layer_counts, chains, args, out, unaligned_layers=0):
    stream = torch.cuda.current_stream().cuda_stream
    max_layers = max(layer_counts)
    n_sources = n_out * max_layers
    cap = frames + 2      # (an even number of frames: rows stay 16-byte aligned at even channel counts; src_first = 1 has room)
    row = cap * ch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    # [scratch A x n_out][sources][scratch B x n_out]: the chain's layout; the mix reads the sources alone
    pool = torch.empty(((2 * n_out + n_sources) * row,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    p_a, p_src = pool.data_ptr(), pool.data_ptr() + 4 * n_out * row
    p_b = p_src + 4 * n_sources * row
    mix_out = torch.zeros((n_out * row,), device="cuda")
    yard_in = torch.empty((n_out * row,), device="cuda").uniform_(-1.0, 1.0, generator=gen)
    yard_out = torch.zeros((n_out * row,), device="cuda")
    g = np.zeros((n_out,), GAIN_RECORD_DTYPE)
    g["gain"] = np.float32(0.5)
    gains = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    out_frames = np.full((n_out,), frames, np.uint32)
    cfg = capi.LoudnessConfig(sample_rate=48000.0)
    bank = ProgramLoudnessBank(api, cfg, n_sources, ch, 1)
    bank.configure_mix(ch, n_out)
    yard = ProgramLoudnessBank(api, cfg, n_out, ch, 1)
    arms = {YARDSTICK: lambda: yard.apply_gains(yard_in.data_ptr(), yard_out.data_ptr(), cap, ch, gains.data_ptr(), n_out, frames=out_frames,
                                                stream=stream)}
    layers_of, bytes_of = {}, {YARDSTICK: 8}

    def add_mix(name, layers, src_first=0):
        table = mix_sends(n_out, max_layers, layers, frames, src_first)
        arms[name] = lambda: bank.mix(p_src, cap, table, mix_out.data_ptr(), cap, out_frames, stream=stream)
        layers_of[name], bytes_of[name] = layers, 4 * (layers + 1)

    for layers in layer_counts:
        add_mix(f"mix, {layers} layer{'s' if layers > 1 else ''}", layers)
    if unaligned_layers:
        add_mix(f"mix, {unaligned_layers} layers from src_first 1 (sources off the 16-byte boundary)", unaligned_layers, 1)
    chain_bank = None
    if chains:
        chain_bank = ProgramLoudnessBank(api, cfg, n_sources + n_out, ch, 1)
        chain_bank.configure_edit(ch, n_out)
        for layers in chains:
            calls = chain_tables(n_out, max_layers, layers, frames, n_sources)

            def run(calls=calls):
                for from_a, table in calls:
                    chain_bank.edit(p_a if from_a else p_src, cap, table, p_b if from_a else p_a, cap, out_frames, stream=stream)

            name = f"chain of {layers - 1} edit calls ({layers} layers)"
            arms[name] = run
            layers_of[name], bytes_of[name] = layers, 12 * (layers - 1)
    out[key] = t = alternated(arms, args.warmup, args.reps, args.inner)
    samples = n_out * frames * ch
    y = t[YARDSTICK]["median"]
    for arm, r in t.items():
        moved = bytes_of[arm] * samples
        line = (f"{title}, {arm}: median {r['median']:.4f} ms (min {r['min']:.4f}, max {r['max']:.4f}, {r['reps']} reps; even / odd repetitions "
                f"{r['median_even']:.4f} / {r['median_odd']:.4f}), {moved / 1e9:.3f} GB read + written, {moved / (r['median'] * 1e-3) / 1e12:.2f} TB/s")
        if arm.startswith("mix"):
            layers = layers_of[arm]
            r["ratio_to_yardstick"] = r["median"] / y
            r["ratio_to_bytes"] = r["median"] / (y * (layers + 1) / 2.0)
            line += f", {r['ratio_to_yardstick']:.3f} x the yardstick, {r['ratio_to_bytes']:.3f} x yardstick x (L + 1) / 2"
        elif arm.startswith("chain"):
            layers = layers_of[arm]
            mix_ms = t[f"mix, {layers} layers"]["median"]
            r["mix_over_chain"] = mix_ms / r["median"]
            line += f"; mix of {layers} layers / chain = {r['mix_over_chain']:.3f} (bytes: {4 * (layers + 1) / (12.0 * (layers - 1)):.3f})"
        r["bytes"] = moved
        say(line)
    rec = bank.fetch_mixed(n_out - 1)
    say(f"    bus {n_out - 1} of the last mix call: {int(rec['frames'])} frames, {int(rec['mixed_frames'])} mixed, {int(rec['samples_over'])} over, "
        f"peak {rec['out_sample_peak_db']:.3f} dB, {int(rec['sends'])} sends, {int(rec['max_layers'])} layers deep")
    bank.close()
    yard.close()
    if chain_bank:
        chain_bank.close()


def host_side(api, args, out):
    """wall time of a call that renders no frame: what the host does per call for 1024 buses x 8 sends"""
    n_out, layers, frames, ch = 1024, 8, 16384, 2
    bank = ProgramLoudnessBank(api, capi.LoudnessConfig(sample_rate=48000.0), n_out * layers, ch, 1)
    bank.configure_mix(ch, n_out)
    table = mix_sends(n_out, layers, layers, frames)
    none = np.zeros((n_out,), np.uint32)
    d = torch.zeros((16,), device="cuda")
    ms = []
    for i in range(args.reps + args.warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank.mix(d.data_ptr(), frames, table, d.data_ptr(), 0, none)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[args.warmup:])
    out["c_host_1024x8"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "sends": int(table.size)}
    say(f"(c) host side of one call, 1024 buses x 8 sends (validation, spans, blob of the tables, upload, begin and finish launches; no frame "
        f"rendered): median {ms[len(ms) // 2]:.4f} ms wall (min {ms[0]:.4f}, max {ms[-1]:.4f}, {len(ms)} calls)")
    bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "program_mix.txt"))
    args = ap.parse_args()
    assert openmeters_amd.device_available(), "bench_program_mix needs a gfx950 device: there is no CPU fallback"
    api = openmeters_amd.api()
    out = {}
    info = mix_plan(api, 2)
    say(f"mix plan at 2 channels: tile {int(info['tile_frames'])} frames, {int(info['layers_per_batch'])} layers per batch")
    shape("a_1024x16384x2", "(a) 1024 buses x 16 384 frames, 2 channels", api, 1024, 2, 16384, [1, 2, 4, 8, 16], [4, 8], args, out, unaligned_layers=4)
    shape("a_1024x16384x8", "(a) 1024 buses x 16 384 frames, 8 channels", api, 1024, 8, 16384, [1, 2, 4, 8, 16], [], args, out)
    shape("b_64x60s_into8", "(b) 64 x 60 s at 48 kHz stereo into 8 buses", api, 8, 2, 60 * 48000, [8], [8], args, out)
    host_side(api, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

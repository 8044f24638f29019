"""Programme loudness bank on the GPU (`-m gpu`): the product (openmeters_amd.program_loudness) against the numpy restatement
(tests/program_loudness_ref.py, pinned to the oracle and to the EBU synthetic cases by tests/test_cpu_program_loudness.py).

Bars: 1e-4 LU on every LUFS / LU field (the project's loudness bar, tests/test_gpu_parity_meters.py), exact equality on every count.
Inputs keep a gate margin of 2e-3 LU in the restatement (asserted on the CPU), so no block may change sides of a gate."""
import subprocess

import numpy as np
import pytest

import program_loudness_ref as ref
from openmeters_amd import banks, capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, ProgramLoudnessBank, ProgramLoudnessRecord)
from parity import bar

pytestmark = pytest.mark.gpu
BAR = 1e-4
LEVELS = [f for f in ProgramLoudnessRecord.LEVEL_FIELDS if f != "max_true_peak_db"]
COUNTS = ProgramLoudnessRecord.COUNT_FIELDS
FLOOR = -99.9


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_rows(torch, xs, ch):
    """programmes of different lengths as one device array [S][longest][ch] (zero padded)"""
    longest = max(len(x) for x in xs)
    host = np.zeros((len(xs), longest, ch), np.float32)
    for s, x in enumerate(xs):
        host[s, :len(x)] = x
    return torch.from_numpy(host).cuda(), longest


def run_once(torch, omx, xs, fs, ch, pos, form=0, capacity_seconds=200):
    """every programme whole, in ONE call (per-stream frame counts)"""
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, capacity_seconds)
    bank.set_option(capi.OPT_KERNEL_FORM, form)
    d, longest = device_rows(torch, xs, ch)
    bank.process(d.data_ptr(), longest, ch, fs, pos, frames=[len(x) for x in xs], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bank


def run_schedule(torch, omx, xs, fs, ch, pos, schedule, form=FORM_REFERENCE_ORDER, capacity_seconds=200, resets=None):
    """schedule: per call an array of per-stream frame counts; every stream walks its own programme"""
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, capacity_seconds)
    bank.set_option(capi.OPT_KERNEL_FORM, form)
    cursor = [0] * len(xs)
    for k, counts in enumerate(schedule):
        cap = max(int(max(counts)), 1)
        host = np.zeros((len(xs), cap, ch), np.float32)
        for s, n in enumerate(counts):
            host[s, :n] = xs[s][cursor[s]:cursor[s] + n]
            cursor[s] += int(n)
        d = torch.from_numpy(host).cuda()
        bank.process(d.data_ptr(), cap, ch, fs, pos, frames=counts, reset_mask=resets[k] if resets else None,
                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return bank


def check_record(rec, want, tag, measured=None):
    for f in LEVELS:
        d = bar(f"program loudness: |d {f}| LU", abs(float(getattr(rec, f)) - float(want[f])), BAR, (tag, getattr(rec, f), want[f]))
        if measured is not None:
            measured[f] = max(measured.get(f, 0.0), d)
    for f in COUNTS:
        assert getattr(rec, f) == want[f], (tag, f, getattr(rec, f), want[f])


def coefficients(oracle, fs):
    return oracle.k_weighting_coefficients(ref.sanitize_rate(fs))


def test_ebu_cases_through_the_product(torch_dev, omx, oracle):
    """the nine EBU Tech 3341 / 3342 cases as nine streams of one bank, each whole in one call: against the restatement (1e-4 LU, counts
    exact) and against the documents' own tolerances"""
    fs, pos = 48000.0, capi.positions_fallback(2)
    cases = ref.EBU_3341 + ref.EBU_3342
    xs = [ref.tone_programme(fs, spans) for _, spans, _ in cases]
    measured = {}
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_once(torch_dev, omx, xs, fs, 2, pos, form)
        assert bank.last_form() == form
        for s, (name, _, want) in enumerate(cases):
            rec = bank.fetch(s)
            check_record(rec, ref.restate(xs[s], fs, pos, coefficients(oracle, fs)), (name, form), measured)
            if name.startswith("3341"):
                assert abs(rec.integrated_lufs - want) <= 0.1, (name, rec.integrated_lufs)
            else:
                assert abs(rec.loudness_range_lu - want) <= 1.0, (name, rec.loudness_range_lu)
            print(name, "form", form, rec.integrated_lufs, rec.loudness_range_lu)
    print("EBU cases, measured maxima (LU):", {k: f"{v:.2e}" for k, v in measured.items()})


@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_seeded_programmes_against_the_restatement_in_both_forms(torch_dev, omx, oracle, fs, ch, seeds):
    """40 s programmes with blocks on both sides of both gates: each form against the restatement, and the time-parallel form against
    the reference-order form (L of every gating block above -70 LUFS within 1e-4 dB)"""
    pos = capi.positions_fallback(ch)
    xs = [ref.programme(seed, fs, ch, ref.SEEDED_SECONDS) for seed in seeds]
    want = [ref.restate(x, fs, pos, coefficients(oracle, fs)) for x in xs]
    segs, measured = {}, {}
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_once(torch_dev, omx, xs, fs, ch, pos, form)
        assert bank.last_form() == form
        for s in range(len(xs)):
            check_record(bank.fetch(s), want[s], (fs, ch, seeds[s], form), measured)
        segs[form] = [bank.fetch_segments(s) for s in range(len(xs))]
    worst = 0.0
    for s in range(len(xs)):
        a, b = ref.sliding_mean(segs[FORM_REFERENCE_ORDER][s], 4), ref.sliding_mean(segs[FORM_TIME_PARALLEL][s], 4)
        keep = a > ref.ABSOLUTE_GATE
        worst = max(worst, float(np.abs(ref.level(a[keep]) - ref.level(b[keep])).max()))
        rel = np.abs(segs[FORM_REFERENCE_ORDER][s] - want[s]["e"]) / np.maximum(want[s]["e"], 1e-30)
        print(f"{fs} Hz {ch} ch seed {seeds[s]}: segment energies vs restatement, worst relative {rel[want[s]['e'] > 1e-12].max():.2e}")
    print(f"{fs} Hz {ch} ch: time-parallel vs reference order, gating blocks above -70 LUFS: {worst:.2e} dB;",
          "vs restatement (LU):", {k: f"{v:.2e}" for k, v in measured.items()})
    bar("program loudness: time-parallel vs reference-order gating blocks, dB", worst, BAR, (fs, ch))


def ragged_schedule(rng, lengths, lo, hi):
    left, out = list(lengths), []
    while any(left):
        counts = [0 if rng.random() < 0.2 else int(min(rng.integers(lo, hi), n)) for n in left]
        left = [n - c for n, c in zip(left, counts)]
        out.append(np.array(counts, np.uint32))
    return out


@pytest.mark.parametrize("fs,ch", [(48000.0, 2), (44100.0, 6)])
def test_segment_energies_do_not_depend_on_the_call_partition(torch_dev, omx, fs, ch):
    """one call, 256-frame calls, ragged calls with random per-stream counts including 0: the reference-order form's stored segment
    energies are bit-identical; a stream in a mixed bank equals the same stream alone in a bank"""
    seconds = 12
    pos = capi.positions_fallback(ch)
    xs = [ref.programme(seed, fs, ch, seconds) for seed in (0, 1, 3)]
    T = len(xs[0])
    whole = run_once(torch_dev, omx, xs, fs, ch, pos, FORM_REFERENCE_ORDER)
    base = [whole.fetch_segments(s) for s in range(3)]
    assert all(len(b) == T // ref.segment_frames(fs) for b in base)
    blocks = [np.full(3, min(256, T - t), np.uint32) for t in range(0, T, 256)]
    rng = np.random.default_rng(5)
    for name, schedule in (("256-frame calls", blocks), ("ragged calls", ragged_schedule(rng, [T] * 3, 1, 9000))):
        bank = run_schedule(torch_dev, omx, xs, fs, ch, pos, schedule)
        for s in range(3):
            got = bank.fetch_segments(s)
            assert got.tobytes() == base[s].tobytes(), (name, s, np.abs(got - base[s]).max())
            assert bank.fetch(s) == whole.fetch(s), (name, s)
    alone = run_once(torch_dev, omx, xs[1:2], fs, ch, pos, FORM_REFERENCE_ORDER)
    assert alone.fetch_segments(0).tobytes() == base[1].tobytes() and alone.fetch(0) == whole.fetch(1)


def test_reset_per_stream_and_reset_mask_inside_process(torch_dev, omx, oracle):
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    co = coefficients(oracle, fs)
    xs = [ref.programme(seed, fs, ch, 10) for seed in (0, 1)]
    half = len(xs[0]) // 2 + 1234
    # stream 1 is reset by the mask of the second call: its programme is its second part alone
    schedule = [np.array([half, half], np.uint32), np.array([len(xs[0]) - half] * 2, np.uint32)]
    bank = run_schedule(torch_dev, omx, xs, fs, ch, pos, schedule, resets=[None, [0, 1]])
    check_record(bank.fetch(0), ref.restate(xs[0], fs, pos, co), "not reset")
    check_record(bank.fetch(1), ref.restate(xs[1][half:], fs, pos, co), "reset by the call's mask")
    # reset() of stream 0 alone: floor values, stream 1 untouched
    before = bank.fetch(1)
    bank.reset([1, 0])
    empty = bank.fetch(0)
    assert bank.fetch(1) == before
    assert empty.frames == 0 and empty.segments == 0 and empty.gating_blocks == 0 and not empty.overflow
    for f in ("integrated_lufs", "momentary_lufs", "short_term_lufs", "max_momentary_lufs", "max_short_term_lufs", "max_true_peak_db"):
        assert getattr(empty, f) == np.float32(FLOOR), f
    assert empty.loudness_range_lu == 0.0 and empty.integrated_energy == 0.0
    # and it starts over like a new bank
    d = torch_dev.from_numpy(np.stack([xs[0], xs[1]])).cuda()
    bank.process(d.data_ptr(), len(xs[0]), ch, fs, pos, frames=[len(xs[0]), 0])
    check_record(bank.fetch(0), ref.restate(xs[0], fs, pos, co), "after reset()")
    assert bank.fetch(1) == before


def test_floor_values_before_the_first_block_and_rate_change_is_refused(torch_dev, omx, oracle):
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    x = ref.programme(4, fs, ch, 2)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, 60)
    d = torch_dev.from_numpy(x[None]).cuda()
    bank.process(d.data_ptr(), len(x), ch, fs, pos, frames=[3 * 4800 + 100])     # three segments: no gating block yet
    rec = bank.fetch(0)
    assert rec.segments == 3 and rec.gating_blocks == 0 and rec.frames == 3 * 4800 + 100
    assert rec.integrated_lufs == np.float32(FLOOR) and rec.momentary_lufs == np.float32(FLOOR) and rec.loudness_range_lu == 0.0
    with pytest.raises(capi.OmxError) as e:
        bank.process(d.data_ptr(), len(x), ch, 44100.0, pos, frames=[100])
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OmxError) as e:
        bank.process(d.data_ptr(), len(x) // 2, 1, fs, pos, frames=[100])
    assert e.value.status == capi.ERR_INVALID
    assert bank.fetch(0) == rec
    bank.process(d.data_ptr(), len(x), ch, 44100.0, pos, frames=[len(x)], reset_mask=[1])     # with a reset in the same call: accepted
    check_record(bank.fetch(0), ref.restate(x, 44100.0, pos, coefficients(oracle, 44100.0)), "rate change with reset")


def test_overflow_at_a_small_capacity(torch_dev, omx, oracle):
    """capacity 5 s = 50 segments: the flag is set, the counts stop, the results are those of the stored part"""
    fs, ch, pos = 48000.0, 2, capi.positions_fallback(2)
    xs = [ref.programme(seed, fs, ch, 8) for seed in (0, 3)]
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_schedule(torch_dev, omx, xs, fs, ch, pos, [np.array([100000, 150000], np.uint32)] * 2 + [np.array([100000, 84000], np.uint32), np.array([84000, 0], np.uint32)],
                            form=form, capacity_seconds=5)
        for s in range(2):
            rec = bank.fetch(s)
            assert rec.overflow and rec.segments == 50 and rec.frames == 50 * 4800
            check_record(rec, ref.restate(xs[s], fs, pos, coefficients(oracle, fs), capacity_segments=50), ("overflow", form, s))
    small = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), 1, ch, 5)
    d = torch_dev.from_numpy(xs[0][None]).cuda()
    small.process(d.data_ptr(), len(xs[0]), ch, fs, pos, frames=[4800 * 49])
    assert not small.fetch(0).overflow


def test_note_snapshots_folds_the_true_peaks_of_a_loudness_bank(torch_dev, omx):
    fs, ch, pos, S, blocks = 48000.0, 2, capi.positions_fallback(2), 3, 16
    xs = np.stack([ref.programme(seed, fs, ch, 1)[:256 * blocks * 2] for seed in (1, 3, 4)])
    meter = banks.LoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch, 60)
    assert bank.fetch(0).max_true_peak_db == np.float32(FLOOR)
    want = np.full(S, np.float32(FLOOR))
    for half in range(2):
        d = torch_dev.from_numpy(np.ascontiguousarray(xs[:, half * 256 * blocks:(half + 1) * 256 * blocks])).cuda()
        snaps = meter.process_device(d.data_ptr(), 256, blocks, ch, fs, pos)
        bank.note_snapshots(snaps, blocks)
        for s in range(S):
            for k in range(blocks):
                want[s] = max(want[s], meter.fetch(s, k).true_peak_db[:ch].max())
    for s in range(S):
        assert bank.fetch(s).max_true_peak_db == want[s], (s, bank.fetch(s).max_true_peak_db, want[s])
    bank.reset([0, 1, 0])
    assert bank.fetch(1).max_true_peak_db == np.float32(FLOOR) and bank.fetch(2).max_true_peak_db == want[2]


def test_lfe_and_surround_weights_and_a_non_finite_sample(torch_dev, omx, oracle):
    """5.1 + sides with the LFE loud (weight 0) and the rear / side channels at 1.41; a NaN in one channel silences that channel from
    there on (the filter state stays non-finite, every later energy counts as 0: WindowedMeans::push) and nothing else"""
    fs, ch = 48000.0, 8
    pos = ref.SURROUND_71
    x = ref.programme(7, fs, ch, 12)
    x[:, 3] *= 30.0
    y = x.copy()
    y[200000, 5] = np.nan
    z = x.copy()
    z[300000, 0] = np.inf
    co = coefficients(oracle, fs)
    for form in (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL):
        bank = run_once(torch_dev, omx, [x, y, z], fs, ch, pos, form)
        for s, prog in enumerate((x, y, z)):
            want = ref.restate(prog, fs, pos, co)
            assert want["gate_margin"] >= ref.GATE_MARGIN_MIN
            check_record(bank.fetch(s), want, ("weights / non-finite", form, s))
    no_lfe = x.copy()
    no_lfe[:, 3] = 0.0
    assert ref.restate(no_lfe, fs, pos, co)["integrated_energy"] == pytest.approx(ref.restate(x, fs, pos, co)["integrated_energy"], rel=1e-12)


def test_full_shape_once(torch_dev, omx, oracle):
    """1024 streams x 8 ch x 16 384 frames per call, four calls (two in each form), a sample of streams against the restatement"""
    torch = torch_dev
    fs, ch, S, frames, calls = 48000.0, 8, 1024, 16384, 4
    pos = ref.SURROUND_71
    sample = [0, 1, 63, 64, 511, 777, 1023]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    levels = 10.0 ** (torch.empty((calls, S, 1, 1), device="cuda").uniform_(-60.0, -10.0, generator=gen) / 20.0)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), S, ch, 30)
    kept = {s: [] for s in sample}
    for k in range(calls):
        pcm = torch.randn((S, frames, ch), device="cuda", generator=gen) * levels[k]
        bank.set_option(capi.OPT_KERNEL_FORM, FORM_REFERENCE_ORDER if k % 2 == 0 else FORM_TIME_PARALLEL)
        bank.process(pcm.data_ptr(), frames, ch, fs, pos, stream=torch.cuda.current_stream().cuda_stream)
        for s in sample:
            kept[s].append(pcm[s].cpu().numpy())
        torch.cuda.synchronize()
    measured = {}
    for s in sample:
        want = ref.restate(np.concatenate(kept[s]), fs, pos, coefficients(oracle, fs))
        assert want["gate_margin"] >= ref.GATE_MARGIN_MIN and want["gating_blocks"] == 10
        check_record(bank.fetch(s), want, ("full shape", s), measured)
    print("full shape, measured maxima (LU):", {k: f"{v:.2e}" for k, v in measured.items()})


def test_c99_host_gets_the_ebu_numbers(tmp_path, omx):
    """tests/c_abi/program_loudness_demo.c: Tech 3341 cases 1 and 2 from a plain C host in calls of 0.37 s"""
    from test_cpu_program_loudness import build_demo
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    v = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)}
    assert abs(v["integrated0"] + 23.0) <= 0.1 and abs(v["integrated1"] + 33.0) <= 0.1 and v["lra0"] < 0.01
    assert v["segments"] == 200 and v["gating"] == 197 and v["above_rel"] == 197 and v["overflow"] == 0 and v["form"] in (1, 2)

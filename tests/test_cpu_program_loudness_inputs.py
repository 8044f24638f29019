"""Conditions on the INPUTS of tests/test_gpu_program_loudness_matrix.py, checked without a device: the lowest rate follows from the
filter's poles; every programme the GPU tests compare keeps its distance from the gates in the restatement (and has blocks on both
sides of both gates where the test says it exercises them); the bound of the result-pass energies holds for both summation orders."""
import math

import numpy as np
import pytest

import program_loudness_ref as ref
from openmeters_amd import capi


def coefficients(oracle, fs):
    return oracle.k_weighting_coefficients(ref.sanitize_rate(fs))


def pole_radius(oracle, fs):
    return float(np.abs(np.roots(np.asarray(coefficients(oracle, fs)[1], np.float64))).max())


def test_lowest_rate_is_where_every_pole_is_inside_the_unit_circle(oracle):
    """The shelf of k_weighting_coefficients sits at 1681.97 Hz: up to twice that the bilinear transform yields poles outside the unit
    circle (the state overflows within a few hundred frames): every whole rate from 1682 Hz to MIN_RATE - 1 is unstable, every one
    from MIN_RATE on is stable, and MIN_RATE is the limit the bank refuses below.  (Below 1682 Hz the shelf lies above the rate itself
    and the tangent of the transform wraps: poles outside the circle again from 1 kHz to 1121 Hz, inside it between — a stable filter
    there, but no K-weighting.)"""
    radii = {fs: pole_radius(oracle, float(fs)) for fs in range(1000, 8001)}
    unstable = [fs for fs, r in radii.items() if r >= 1.0]
    print("unstable whole rates:", min(unstable), "...", max(unstable), "; radius at 1 kHz %.3f, 2 kHz %.3f, 3 kHz %.3f, %d Hz %.6f, %d Hz %.6f, 4 kHz %.3f, 8 kHz %.3f"
          % (radii[1000], radii[2000], radii[3000], max(unstable), radii[max(unstable)], max(unstable) + 1, radii[max(unstable) + 1], radii[4000], radii[8000]))
    assert unstable == list(range(1000, 1122)) + list(range(1682, int(ref.MIN_RATE)))
    assert ref.MIN_RATE == max(unstable) + 1 and ref.MIN_RATE - 1 < 2 * 1681.97 < ref.MIN_RATE
    for fs in (8000, 9000, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000, 768000):
        assert pole_radius(oracle, float(fs)) < 1.0, fs
    # the product states the same limits (csrc/program/ is the only place they live)
    import os
    hpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openmeters_amd", "csrc", "program", "program_loudness.hpp")).read()
    assert f"kPlMinRate = {ref.MIN_RATE:.1f}f" in hpp and f"kPlTimeParallelMaxRate = {ref.TIME_PARALLEL_MAX_RATE:.1f}f" in hpp


@pytest.mark.parametrize("fs,ch,seconds,seeds", ref.MATRIX_CASES)
def test_matrix_programmes_keep_their_distance_from_the_gates(oracle, fs, ch, seconds, seeds):
    """a gate margin of at least 2e-3 LU (20 x the bar) and gating blocks on both sides of both gates, for every seed of every row"""
    assert len(seeds) == 3
    for seed in seeds:
        r = ref.restate(ref.programme(seed, fs, ch, seconds), fs, capi.positions_fallback(ch), coefficients(oracle, fs))
        print(fs, ch, seed, f"margin {r['gate_margin']:.4f} LU", r["gating_blocks"], r["gating_above_absolute"], r["gating_above_relative"])
        assert r["gate_margin"] >= ref.GATE_MARGIN_MIN, (fs, ch, seed, r["gate_margin"])
        assert r["gating_blocks"] > r["gating_above_absolute"] > r["gating_above_relative"] > 0
        assert r["short_term_above_relative"] > 0


def test_matrix_covers_what_the_bank_accepts():
    rows = [(fs, ch) for fs, ch, _, _ in ref.MATRIX_CASES]
    assert {ch for _, ch in rows} >= {1, 3, 4, 5, 7}                        # (2, 6 and 8 channels: tests/test_gpu_program_loudness.py)
    assert {fs for fs, _ in rows} >= {ref.MIN_RATE, 8000.0, 9000.0, 11025.0, 22050.0, 32000.0, 88200.0, 176400.0, 192000.0, 384000.0, ref.MAX_RATE}
    assert ref.segment_frames(9000.0) == 900 and 900 % 32 != 0               # an item that is no whole number of tiles
    assert ref.segment_frames(11025.0) == 1103 and ref.segment_frames(8000.0) < 1024 < ref.segment_frames(11025.0)
    assert ref.sanitize_rate(1e9) == ref.MAX_RATE


@pytest.mark.parametrize("ch", [1, 8])
@pytest.mark.parametrize("fs", ref.HARD_RATES)
def test_hard_inputs_keep_their_distance_from_the_gates(oracle, fs, ch):
    pos = ref.SURROUND_71 if ch == 8 else capi.positions_fallback(ch)
    for kind in ref.HARD_KINDS:
        r = ref.restate(ref.hard_input(kind, fs, ch), fs, pos, coefficients(oracle, fs))
        print(fs, ch, kind, f"margin {r['gate_margin']:.4f} LU", r["gating_blocks"], r["gating_above_absolute"], r["gating_above_relative"],
              r["integrated_lufs"], r["momentary_lufs"])
        assert r["gate_margin"] >= ref.GATE_MARGIN_MIN, (fs, ch, kind, r["gate_margin"])
        assert r["gating_above_absolute"] >= 60 and r["momentary_lufs"] > -60.0 and r["short_term_lufs"] > -60.0   # the quiet end is above the gate
        if kind == "drop":      # the 100 dB drop is below the absolute gate, the quiet end above it and below the relative gate
            assert r["gating_blocks"] > r["gating_above_absolute"] > r["gating_above_relative"] > 0


@pytest.mark.parametrize("ch", [1, 8])
def test_ninety_seconds_at_full_scale_then_quiet_keeps_its_distance_from_the_gates(oracle, ch):
    fs, pos = 48000.0, ref.SURROUND_71 if ch == 8 else capi.positions_fallback(ch)
    r = ref.restate(ref.long_loud_then_quiet(fs, ch), fs, pos, coefficients(oracle, fs))
    print(ch, f"margin {r['gate_margin']:.4f} LU", r["gating_above_absolute"], r["gating_above_relative"], r["integrated_lufs"], r["momentary_lufs"])
    assert r["gate_margin"] >= ref.GATE_MARGIN_MIN
    assert r["gating_above_absolute"] > r["gating_above_relative"] > 0 and -60.0 < r["momentary_lufs"] < -40.0


def test_small_inputs_of_the_shape_tests_keep_their_distance_from_the_gates(oracle):
    """the 2 ch / 3 ch programmes of the bank-shape, ragged and per-call-weight tests (ref.SHAPE_POOL, ref.WEIGHT_CHANGE_CASE)"""
    for fs, ch, seconds, seeds in ref.SHAPE_CASES:
        for seed in seeds:
            r = ref.restate(ref.programme(seed, fs, ch, seconds), fs, capi.positions_fallback(ch), coefficients(oracle, fs))
            print(fs, ch, seconds, seed, f"margin {r['gate_margin']:.4f} LU")
            assert r["gate_margin"] >= ref.GATE_MARGIN_MIN, (fs, ch, seconds, seed, r["gate_margin"])
    fs, ch, seconds, seed = ref.WEIGHT_CHANGE_CASE
    x = ref.programme(seed, fs, ch, seconds)
    half = len(x) // 2 + 777
    e = ref.segment_energies_per_call(x, fs, [(half, ref.REAR_POSITIONS), (len(x) - half, ref.FRONT_POSITIONS)], coefficients(oracle, fs))
    r = ref.results(e)
    assert r["gate_margin"] >= ref.GATE_MARGIN_MIN and r["gating_above_relative"] > 0
    # the variant is the plain restatement when the positions never change, and 1.41 x it while all channels are rear ones
    same = ref.segment_energies_per_call(x, fs, [(half, ref.FRONT_POSITIONS), (len(x) - half, ref.FRONT_POSITIONS)], coefficients(oracle, fs))
    plain = ref.segment_energies(x, fs, ref.FRONT_POSITIONS, coefficients(oracle, fs))
    assert np.allclose(same, plain, rtol=1e-13, atol=0.0)
    n_first = half // ref.segment_frames(fs)
    assert np.allclose(e[:n_first], 1.41 * plain[:n_first], rtol=1e-13, atol=0.0) and np.allclose(e[n_first + 1:], plain[n_first + 1:], rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("kind", ["tone", "steps"])
def test_hour_programmes_for_the_result_pass(oracle, kind):
    """1 h at 8 kHz mono: compared through the result pass only (ref.results of the fetched e[] against the record), where the margin
    has to exceed the energy bound alone: at least 1e-6 LU.  `steps` has blocks on both sides of both gates; in `tone` both
    loudness-range ranks fall inside runs of thousands of equal short-term blocks."""
    fs = ref.HOUR_RATE
    r = ref.restate(ref.hour_programme(kind), fs, capi.positions_fallback(1), coefficients(oracle, fs))
    print(kind, f"margin {r['gate_margin']:.2e} LU", r["gating_blocks"], r["gating_above_absolute"], r["gating_above_relative"],
          r["short_term_above_absolute"], r["short_term_above_relative"], r["integrated_lufs"], r["loudness_range_lu"])
    assert r["segments"] == 36000 and r["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN
    stream, seg, at = ("tone", "steps").index(kind), ref.segment_frames(fs), 0
    assert sum(c[stream] for c in ref.HOUR_CALLS) == 36000 * seg - (seg + seg // 2 if kind == "tone" else 0)
    for c in ref.HOUR_CALLS:        # the test looks at the records after every call: the condition holds for every such prefix
        at += c[stream]
        prefix = ref.results(r["e"][:at // seg])
        print(kind, "after", at, f"frames: margin {prefix['gate_margin']:.2e} LU")
        assert prefix["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN, (kind, at, prefix["gate_margin"])
    assert ref.RESULT_PASS_MARGIN_MIN == 1e-6 and 10 * np.log10(1 + ref.energy_bound(36000)) < 1e-10     # (the bound, in LU, is far below the margin)
    assert r["gating_blocks"] > r["gating_above_absolute"] > r["gating_above_relative"] > 0
    assert r["short_term_blocks"] > r["short_term_above_absolute"] > r["short_term_above_relative"] > 0
    st = ref.sliding_mean(r["e"], 30)
    sa = st[st > ref.ABSOLUTE_GATE]
    sr = np.sort(sa[sa > 0.01 * sa.mean()])
    runs = []
    for q in (0.10, 0.95):
        k = int(np.floor((len(sr) - 1) * q + 0.5))
        equal, below = int((sr == sr[k]).sum()), int((sr < sr[k]).sum())
        runs.append(equal)
        assert below <= k < below + equal
        if kind == "tone":
            assert equal > 10000 and below < k < below + equal - 1       # strictly inside a run of equal keys
    print(kind, "equal keys at the two ranks:", runs)
    if kind == "tone":
        assert r["lra_low_energy"] < r["lra_high_energy"]


def test_energy_bound_covers_both_summation_orders():
    """(n + 30) * 2^-53 (ref.energy_bound): the mean in the result pass's order (256 strided partials, binary tree) and numpy's mean,
    each against the exact mean (math.fsum), and against each other, for n from 1 to 144 000 non-negative values over 12 decades"""
    rng = np.random.default_rng(8)
    worst = 0.0
    for n in (1, 2, 3, 31, 255, 256, 257, 771, 5000, 36000, 144000):
        for spread in (0.0, 3.0, 12.0):
            v = 10.0 ** (rng.uniform(-spread, 0.0, n)) * rng.uniform(0.5, 1.0, n)
            exact = math.fsum(v) / n
            a, b = ref.result_pass_order_mean(v), float(v.mean())
            for d in (abs(a - exact), abs(b - exact), abs(a - b)):
                assert d <= ref.energy_bound(n) * exact, (n, spread, d / exact)
                worst = max(worst, d / exact / ref.energy_bound(n))
    print(f"largest distance, as a fraction of the bound: {worst:.3f}")
    assert ref.energy_bound(0) == 30 * 2.0 ** -53


def test_four_hour_programme_for_the_result_pass(oracle):
    """144 000 segments (8 kHz mono, stepped levels), compared through the result pass only: margin at least 1e-6 LU, blocks on both sides
    of both gates; filtered in chunks, which is the plain restatement (same recurrence, state carried), bit for bit"""
    fs, pos = ref.HOUR_RATE, capi.positions_fallback(1)
    hour = ref.hour_programme("steps")
    assert (ref.segment_energies_long(hour, fs, pos, coefficients(oracle, fs), chunk_segments=7001) == ref.segment_energies(hour, fs, pos, coefficients(oracle, fs))).all()
    x = ref.hour_programme("steps", seconds=ref.FOUR_HOURS_SECONDS, seed=ref.FOUR_HOURS_SEED)
    r = ref.results(ref.segment_energies_long(x, fs, pos, coefficients(oracle, fs)))
    print(f"four hours: margin {r['gate_margin']:.2e} LU", r["gating_blocks"], r["gating_above_absolute"], r["gating_above_relative"], r["short_term_above_relative"])
    assert r["segments"] == 144000 and r["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN
    assert r["gating_blocks"] > r["gating_above_absolute"] > r["gating_above_relative"] > 0
    assert r["short_term_blocks"] > r["short_term_above_absolute"] > r["short_term_above_relative"] > 0

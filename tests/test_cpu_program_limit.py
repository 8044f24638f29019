"""Programme bank limiter (include/omx/program_limit.h), CPU side: the header as C99, its structures' sizes and offsets, the exported
functions, omx_program_limit_latency and every invalid rule; the numpy restatement (tests/program_limit_ref.py) against itself: an
input under the ceiling passes as x * g, the sample-peak bound, the fast form against a frame-by-frame evaluation of the definition,
pieces with carried state against the whole; and the fairness of the GPU file's round trip: the true peak of the restated output of
the programmes that file sends round, measured by program_peaks_ref, lies within 0.01 dB above the ceiling.

Bars.  Sample peak: |out| <= c (1 + 2^-21), from the definition (DESIGN.md section 10 "Limiter" derives it).  True peak: 0.01 dB, the
figure the GPU round trip is held to; the measured overshoot is printed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_limit_ref as lr
import program_loudness_ref as ref
import program_normalize_ref as nr
import program_peaks_ref as pk
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
FLOOR = -99.9
TRUE_PEAK_BAR_DB = 0.01


@pytest.fixture(scope="module")
def coeffs(oracle):
    return pk.coefficients(oracle)


# ---------------------------------------------------------------- the header
def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


C99_USE = r'''
#include <stddef.h>
#include "omx/program_limit.h"
typedef char limit_rule_is_16_bytes[sizeof(omx_program_limit_rule) == 16 ? 1 : -1];
typedef char limit_record_is_80_bytes[sizeof(omx_program_limit_record) == 80 ? 1 : -1];
int main(void) {
    omx_program_limit_rule rule;
    rule.ceiling_db = -1.0f; rule.attack_frames = 64; rule.release_hold_frames = 0; rule.flags = 0;
    return (int)sizeof(rule) - 16 + (int)offsetof(omx_program_limit_record, gain) - 40 + (int)offsetof(omx_program_limit_record, gain_index) - 64
        + (int)offsetof(omx_program_limit_record, latency_frames) - 72 + (int)(OMX_LIMIT_IDLE + OMX_LIMIT_RUNNING + OMX_LIMIT_FLUSHED) - 3
        + (int)rule.flags;
}
'''


def test_header_is_c99_its_structures_have_their_sizes_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text(C99_USE)
    exe = tmp_path / "use"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    assert subprocess.run([str(exe)]).returncode == 0
    import openmeters_amd
    assert C.sizeof(openmeters_amd.CProgramLimitRule) == 16 and C.sizeof(openmeters_amd.CProgramLimitRecord) == 80
    assert openmeters_amd.LIMIT_RECORD_DTYPE.itemsize == 80 and openmeters_amd.LIMIT_RECORD_DTYPE.names == lr.RECORD_FIELDS
    for f in openmeters_amd.LIMIT_RECORD_DTYPE.names:
        assert openmeters_amd.LIMIT_RECORD_DTYPE.fields[f][1] == getattr(openmeters_amd.CProgramLimitRecord, f).offset, f
    assert [getattr(openmeters_amd.CProgramLimitRule, f).offset for f in ("ceiling_db", "attack_frames", "release_hold_frames", "flags")] == [0, 4, 8, 12]
    syms = declared(os.path.join(INCLUDE, "program_limit.h"))
    assert syms == ["omx_program_limit_latency", "omx_program_loudness_bank_apply_limited", "omx_program_loudness_bank_fetch_limited",
                    "omx_program_loudness_bank_limiter_configure", "omx_program_loudness_bank_limiter_reset"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_limit.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_limit" not in open(os.path.join(ROOT, "include", "omx.h")).read()


def test_python_surface():
    import openmeters_amd
    for name in ("configure_limiter", "reset_limiter", "apply_limited", "fetch_limited"):
        assert callable(getattr(openmeters_amd.ProgramLoudnessBank, name)), name
    c = openmeters_amd.LimitRule(-2.5, 48, 96).to_c()
    assert (c.ceiling_db, c.attack_frames, c.release_hold_frames, c.flags) == (-2.5, 48, 96, 0)


def test_latency_is_the_attack_plus_23(omx):
    import openmeters_amd
    for A in (1, 2, 16, 240, 1024, 4096):
        for R in (0, 100, 16384):
            assert openmeters_amd.limit_latency(omx, openmeters_amd.LimitRule(-1.0, A, R)) == A + 23 == lr.latency((-1.0, A, R))


BAD_RULES = [(np.nan, 16, 0, 0), (np.inf, 16, 0, 0), (-np.inf, 16, 0, 0), (-120.001, 16, 0, 0), (20.001, 16, 0, 0),
             (-1.0, 0, 0, 0), (-1.0, 4097, 0, 0), (-1.0, 2 ** 32 - 1, 0, 0), (-1.0, 16, 16385, 0), (-1.0, 16, 2 ** 32 - 1, 0),
             (-1.0, 16, 0, 1), (-1.0, 16, 0, 2 ** 31)]
GOOD_RULES = [(-120.0, 1, 0, 0), (20.0, 4096, 16384, 0), (-1.0, 16, 100, 0), (-0.0, 1, 16384, 0)]


def test_every_invalid_rule_is_refused_and_writes_nothing(omx):
    import openmeters_amd
    fn = omx.fn("program_limit_latency", C.c_int, [C.c_void_p, C.c_void_p])
    out = C.c_uint32(0xA5A5A5A5)
    for bad in BAD_RULES:
        assert not lr.rule_valid(bad), bad
        c = openmeters_amd.LimitRule(*bad).to_c()
        assert fn(C.byref(c), C.byref(out)) == capi.ERR_INVALID and out.value == 0xA5A5A5A5, bad
        with pytest.raises(capi.OmxError) as err:
            openmeters_amd.limit_latency(omx, openmeters_amd.LimitRule(*bad))
        assert err.value.status == capi.ERR_INVALID
    for good in GOOD_RULES:
        assert lr.rule_valid(good), good
        c = openmeters_amd.LimitRule(*good).to_c()
        assert fn(None, C.byref(out)) == capi.ERR_INVALID and fn(C.byref(c), None) == capi.ERR_INVALID
        assert fn(C.byref(c), C.byref(out)) == 0 and out.value == good[1] + 23, good
        out.value = 0xA5A5A5A5


# ---------------------------------------------------------------- the restatement against itself
def rules():
    return [(lr.CEILING_DB, A, R) for A in lr.ATTACKS for R in lr.HOLDS]


def test_an_input_under_the_ceiling_passes_as_x_times_g(coeffs):
    for fs in lr.RATES:
        x = lr.noise(1, 3000, 2, 0.05)
        for rule in rules():
            out, gf, rec = lr.restate(x, fs, coeffs, lr.GAIN, rule)
            want, over, peak = nr.apply(x, lr.GAIN)
            assert out.tobytes() == want.tobytes() and (gf == np.float32(1.0)).all(), (fs, rule)
            assert (rec["frames_limited"], rec["samples_over"], rec["min_envelope"]) == (0, over, 1.0) and rec["out_sample_peak"] == peak
            assert rec["max_reduction_db"] == 0.0 and rec["frames_in"] == rec["frames_out"] == 3000 and rec["state"] == lr.FLUSHED


def test_sample_peak_stays_under_the_bound(coeffs):
    """inputs 6 and 20 dB over the ceiling, every rate band and rule"""
    worst = 0.0
    for fs in lr.RATES:
        for over_db in (6.0, 20.0):
            g = 10.0 ** ((over_db + lr.CEILING_DB) / 20.0) / 0.9      # noise reaches 0.9
            for make in (lr.noise, lambda s, n, c: lr.gated_tone(s, n, c, fs)):
                x = make(3, 4000, 2)
                for rule in rules():
                    out, gf, rec = lr.restate(x, fs, coeffs, g, rule)
                    c = float(lr.ceiling(rule))
                    peak = float(np.abs(out).max())
                    worst = max(worst, peak / c - 1.0)
                    assert peak <= c * (1.0 + 2.0 ** -21), (fs, over_db, rule, peak, c)
                    assert rec["frames_limited"] > 0 and rec["min_envelope"] < 1.0 and float(rec["out_sample_peak"]) == peak
    print(f"largest |out| / c - 1 = {worst:.3e} (bound {2.0 ** -21:.3e})")


def test_fast_restatement_equals_the_definition_frame_by_frame(coeffs):
    for fs, ch, rule in ((48000.0, 2, (lr.CEILING_DB, 16, 100)), (96000.0, 1, (lr.CEILING_DB, 1, 0)), (192000.0, 3, (lr.CEILING_DB, 240, 0)),
                         (48000.0, 1, (-6.0, 7, 3))):
        for x in (lr.noise(5, 2000, ch), lr.gated_tone(6, 2000, ch, fs), lr.planted(lr.noise(7, 2000, ch), 7)):
            out, gf, _ = lr.restate(x, fs, coeffs, lr.GAIN, rule)
            want, want_gf = lr.direct(x, fs, coeffs, lr.GAIN, rule)
            assert gf.tobytes() == want_gf.tobytes(), (fs, rule)
            assert out.tobytes() == want.tobytes(), (fs, rule)


def test_sliding_minimum_and_boxcar_on_small_windows():
    q = np.random.default_rng(8).integers(0, lr.UNITY_Q + 1, 300).astype(np.uint32)
    for W in (1, 2, 3, 5, 8, 25, 64, 100, 299, 300):
        want = np.array([q[i - W + 1:i + 1].min() for i in range(W - 1, len(q))], np.uint32)
        assert np.array_equal(lr.sliding_min(q, W), want), W
        want = np.array([int(q[i - W + 1:i + 1].astype(np.uint64).sum()) for i in range(W - 1, len(q))], np.uint64)
        assert np.array_equal(lr.boxcar(q, W), want), W


def test_pieces_with_carried_state_equal_the_whole(coeffs):
    for fs, ch, rule in ((48000.0, 2, (lr.CEILING_DB, 16, 100)), (96000.0, 3, (lr.CEILING_DB, 240, 0)), (192000.0, 1, (lr.CEILING_DB, 1, 0))):
        x = lr.planted(lr.noise(9, 5000, ch), 9)
        whole, whole_gf, whole_rec = lr.restate(x, fs, coeffs, lr.GAIN, rule)
        LA = lr.latency(rule)
        for cuts in (lr.ragged_cuts(10, 5000), [0, 1, LA - 1, 1, 5000 - LA - 1], [5000]):
            lim = lr.Limiter(rule, fs, coeffs, ch)
            outs, at = [], 0
            for f in cuts:
                o, _ = lim.feed(x[at:at + f], gain=lr.GAIN, gain_index=0)
                assert lim.E == max(0, lim.N - LA) and len(o) == lim.frames_written
                outs.append(o)
                at += f
            o, _ = lim.feed(x[:0], flush=True)
            outs.append(o)
            assert np.concatenate(outs).tobytes() == whole.tobytes(), (fs, rule, cuts[:5])
            rec = lim.record()
            for f in lr.EXACT_FIELDS:
                if f != "frames_written":
                    assert np.asarray(rec[f]).tobytes() == np.asarray(whole_rec[f]).tobytes(), f


# ---------------------------------------------------------------- fairness of the GPU file's inputs
def overshoot_db(out, fs, coeffs, c):
    peak = max(float(pk.channel_peaks(out[:, k], fs, coeffs)[0]) for k in range(out.shape[1]))
    return 20.0 * np.log10(peak / float(c)) if peak > 0 else -np.inf


def test_true_peak_of_the_restated_output_stays_within_the_bar(coeffs, oracle):
    """the round-trip programmes of tests/test_gpu_program_limit.py at the gain the plan gives them: held to the bar.  The bit-equality
    inputs of that file are not round-tripped; their overshoot is measured and printed per rule, because it is a property of the
    definition (the envelope moves inside the interpolator's window) that DESIGN.md writes down: full-band noise under an attack of
    one frame is its worst case"""
    worst = {}
    for fs in lr.RATES:
        for ch in lr.CHANNELS:
            for name, x, g in lr.case_streams(100 + ch, ch, fs):
                if not np.isfinite(x).all():
                    continue
                for rule in rules():
                    out, _, rec = lr.restate(x, fs, coeffs, g, rule)
                    d = overshoot_db(out, fs, coeffs, lr.ceiling(rule))
                    assert not np.isnan(d)
                    if d > worst.get((name, rule[1]), (-np.inf,))[0]:
                        worst[(name, rule[1])] = (d, fs, ch, rule[2])
    for (name, A), (d, fs, ch, R) in sorted(worst.items()):
        print(f"bit-equality input {name!r}, attack {A}: largest true peak over the ceiling {d:+.3e} dB (at {fs:.0f} Hz, {ch} ch, hold {R})")
    kw = oracle.k_weighting_coefficients(ref.sanitize_rate(lr.ROUND_TRIP_RATE))
    pos = capi.positions_fallback(2)
    for s, x in enumerate(lr.round_trip_programmes()):
        src = ref.restate(x, lr.ROUND_TRIP_RATE, pos, kw, FLOOR)
        peak_db = max(pk.db_f64(pk.channel_peaks(x[:, k], lr.ROUND_TRIP_RATE, coeffs)[0], FLOOR) for k in range(2))
        plan = nr.gain((lr.ROUND_TRIP_TARGET, lr.CEILING_DB, -60.0, 60.0, 0), src["integrated_lufs"], src["gating_above_relative"], peak_db, FLOOR)
        assert plan["limited_by"] == nr.BY_TARGET and float(plan["predicted_peak_db"]) > lr.CEILING_DB + 1.0, (s, plan)
        out, _, rec = lr.restate(x, lr.ROUND_TRIP_RATE, coeffs, plan["gain"], lr.ROUND_TRIP_RULE)
        d = overshoot_db(out, lr.ROUND_TRIP_RATE, coeffs, lr.ceiling(lr.ROUND_TRIP_RULE))
        after = ref.restate(out, lr.ROUND_TRIP_RATE, pos, kw, FLOOR)
        print(f"round trip {s}: gain {float(plan['gain_db']):+.2f} dB, predicted peak {float(plan['predicted_peak_db']):+.2f} dBTP, "
              f"limited {rec['frames_limited']} frames by up to {rec['max_reduction_db']:.2f} dB, true peak {d:+.3e} dB over the ceiling, "
              f"{float(after['integrated_lufs']):.2f} LUFS")
        assert d <= TRUE_PEAK_BAR_DB and rec["frames_limited"] > 0, (s, d)
        assert after["gate_margin"] >= ref.GATE_MARGIN_MIN, (s, after["gate_margin"])

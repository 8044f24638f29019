"""Programme bank filter stage without a device: the numpy restatement (tests/program_filter_ref.py) pinned by hand, and the host-only
functions of include/omx/program_filter.h (design, cascade, check, response, plan) against it.

Bars.  Designed coefficients equal the restated formulas to 1e-12 relative: far above any libm difference, far below anything audible.
The Butterworth kinds have |H| = 10 log10(1/2) = -3.0103 dB at the corner to 1e-9 dB.  The model of the time-parallel schedule, before
its output is rounded to f32, stays within a quarter of the form's bar 2^-23 x max(peak in, peak out) on every hard input: the bar is one
rounding flip at the loudest sample, and a deviation below a quarter of it can flip one rounding and no more."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import program_filter_ref as fr
from openmeters_amd.capi import OmxError
from openmeters_amd.program_loudness import (FILTER_BYPASS, FILTER_DTYPE, FILTER_INFO_DTYPE, FILTER_RECORD_DTYPE, CProgramFilter,
                                             CProgramFilterInfo, CProgramFilterRecord, CProgramFilterSection, CProgramFilterSpec,
                                             FilterSpec, filter_cascade, filter_check, filter_design, filter_plan, filter_response,
                                             filter_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -3, -2
RATES = (8000.0, 44100.0, 48000.0, 192000.0, 768000.0)


def build_demo(tmp_path):
    """tests/c_abi/program_filter_demo.c: a plain C99 host that takes a DC offset out of a tone with a 20 Hz fourth-order high-pass"""
    out = str(tmp_path / "program_filter_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_filter_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def sections_of(f):
    return [tuple(float(f["section"][k][n]) for n in ("b0", "b1", "b2", "a1", "a2")) for k in range(int(f["n_sections"]))]


def refused(status, call, *args):
    with pytest.raises(OmxError) as e:
        call(*args)
    assert e.value.status == status, e.value
    assert "program loudness filter" in str(e.value), e.value


def specs(fs):
    """(name, FilterSpec, the restatement's keyword arguments) of every kind at a rate"""
    f = min(1000.0, fs / 8.0)
    out = []
    for kind, name in ((fr.HIGHPASS, "highpass"), (fr.LOWPASS, "lowpass")):
        for order in (1, 2, 4):
            out.append((f"{name}{order}", dict(kind=kind, order=order, frequency_hz=f)))
        out.append((f"{name}2q", dict(kind=kind, order=2, frequency_hz=f, q=2.5)))
    for kind, name in ((fr.LOW_SHELF, "low_shelf"), (fr.HIGH_SHELF, "high_shelf"), (fr.PEAKING, "peaking")):
        out.append((name + "+", dict(kind=kind, frequency_hz=f, gain_db=6.0)))
        out.append((name + "-", dict(kind=kind, frequency_hz=f, gain_db=-9.5, q=1.3)))
    out.append(("notch", dict(kind=fr.NOTCH, frequency_hz=f, q=4.0)))
    out.append(("dc_block", dict(kind=fr.DC_BLOCK, frequency_hz=5.0)))
    out.append(("deemphasis75", dict(kind=fr.DEEMPHASIS, time_constant_us=75.0)))
    out.append(("deemphasis50", dict(kind=fr.DEEMPHASIS, time_constant_us=50.0)))
    out.append(("deemphasis50/15", dict(kind=fr.DEEMPHASIS, time_constant_us=50.0, time_constant_zero_us=15.0)))
    out.append(("preemphasis50/15", dict(kind=fr.PREEMPHASIS, time_constant_us=50.0, time_constant_zero_us=15.0)))
    return [(name, FilterSpec(**kw), kw) for name, kw in out]


def impulse_response(sections, n):
    x = np.zeros((n, 1), np.float32)
    x[0] = 1.0
    coef, count, bypass = fr.lane_table([sections], None, 1, 1)
    unrounded = np.zeros((n, 1))
    fr.run(x, coef, count, bypass, unrounded=unrounded)
    return unrounded[:, 0]


# ---------------------------------------------------------------- the restatement by hand
def test_restatement_impulse_through_a_hand_computed_section():
    """b = (0.5, 0.25, 0.125), a = (-0.5, 0.25): every value below is exact in binary and worked out on paper from the definition
    (y0 = b0; s1 = b1 - a1 y0 = 0.5, s2 = b2 - a2 y0 = 0; y1 = s1 = 0.5; ...)"""
    got = impulse_response([(0.5, 0.25, 0.125, -0.5, 0.25)], 5)
    assert got.tolist() == [0.5, 0.5, 0.25, 0.0, -0.0625]


def test_restatement_two_sections_bypass_and_carried_state():
    sec_a, sec_b = (0.5, 0.25, 0.125, -0.5, 0.25), (1.0, -1.0, 0.0, -0.5, 0.0)
    x = np.zeros((6, 3), np.float32)
    x[0] = 1.0
    x[3, 2] = np.float32(-0.0)
    coef, count, bypass = fr.lane_table([[sec_a], [sec_a, sec_b]], [[0, 1, FILTER_BYPASS]], 1, 3)
    out, state = fr.run(x, coef, count, bypass)
    # lane 1: the first section's output 0.5, 0.5, 0.25, 0, -0.0625 through y = x - x1 + 0.5 y1
    assert out[:5, 0].tolist() == [0.5, 0.5, 0.25, 0.0, -0.0625]
    assert out[:5, 1].tolist() == [0.5, 0.25, -0.125, -0.3125, -0.21875]
    assert out[:, 2].tobytes() == x[:, 2].tobytes() and state[:, 2].tolist() == [0.0] * 4
    # cut into calls at every frame: the same bytes
    st, parts = None, []
    for i in range(6):
        o, st = fr.run(x[i:i + 1], coef, count, bypass, st)
        parts.append(o)
    assert np.concatenate(parts).tobytes() == out.tobytes() and st.tobytes() == state.tobytes()


def test_restatement_record():
    out = np.array([[0.5, -1.5], [np.nan, 1.0], [np.inf, -0.25]], np.float32)
    r = fr.record(out, 10, 1, -120.0)
    assert (int(r["frames"]), int(r["frames_total"]), int(r["samples_over"]), int(r["samples_nonfinite"])) == (3, 10, 2, 2)
    assert r["out_sample_peak"] == np.float32(np.inf) and int(r["form"]) == 1
    r = fr.record(np.zeros((0, 2), np.float32), 7, 2, -120.0)
    assert (int(r["frames"]), int(r["frames_total"]), int(r["form"])) == (0, 7, 0) and r["out_sample_peak_db"] == np.float32(-120.0)


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("fs", RATES)
def test_designed_coefficients_equal_the_restated_formulas(omx, fs):
    for name, spec, kw in specs(fs):
        got, want = sections_of(filter_design(omx, spec, fs)), fr.design(fs=fs, **kw)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert abs(a - b) <= 1e-12 * abs(b), (name, fs, g, w)
        assert filter_check(omx, got) == 0


@pytest.mark.parametrize("fs", RATES)
def test_gains_at_dc_nyquist_and_corner(omx, fs):
    def db(sections, hz):
        return filter_response(omx, sections, fs, hz)[0]

    f = min(1000.0, fs / 8.0)
    for kind, passes_dc in ((fr.LOWPASS, True), (fr.HIGHPASS, False)):
        for order in (1, 2, 4):
            s = sections_of(filter_design(omx, FilterSpec(kind, order, f), fs))
            kept, gone = (0.0, fs / 2) if passes_dc else (fs / 2, 0.0)
            assert abs(db(s, kept)) <= 1e-9, (kind, order)
            assert db(s, gone) < -250.0, (kind, order, db(s, gone))
            assert abs(db(s, f) - 10.0 * math.log10(0.5)) <= 1e-9, (kind, order, db(s, f))
    for gain in (6.0, -9.5):
        s = sections_of(filter_design(omx, FilterSpec(fr.LOW_SHELF, 0, f, 0.0, gain), fs))
        assert abs(db(s, 0.0) - gain) <= 1e-9 and abs(db(s, fs / 2)) <= 1e-9
        s = sections_of(filter_design(omx, FilterSpec(fr.HIGH_SHELF, 0, f, 0.0, gain), fs))
        assert abs(db(s, 0.0)) <= 1e-9 and abs(db(s, fs / 2) - gain) <= 1e-9
        s = sections_of(filter_design(omx, FilterSpec(fr.PEAKING, 0, f, 2.0, gain), fs))
        assert abs(db(s, 0.0)) <= 1e-9 and abs(db(s, fs / 2)) <= 1e-9 and abs(db(s, f) - gain) <= 1e-9
    s = sections_of(filter_design(omx, FilterSpec(fr.NOTCH, 0, f, 4.0), fs))
    assert abs(db(s, 0.0)) <= 1e-9 and abs(db(s, fs / 2)) <= 1e-9 and db(s, f) < -200.0
    s = sections_of(filter_design(omx, FilterSpec(fr.DC_BLOCK, 0, 5.0), fs))
    assert db(s, 0.0) == -math.inf and abs(db(s, fs / 2) - 20.0 * math.log10(2.0 / (2.0 - 2.0 * math.pi * 5.0 / fs))) <= 1e-9
    # the emphasis kinds: unity at DC; the analogue curve's level at the frequency the bilinear transform maps to fs / 8
    for t1, t2 in ((75.0, 0.0), (50.0, 0.0), (50.0, 15.0)):
        s = sections_of(filter_design(omx, FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, t1, t2), fs))
        assert abs(db(s, 0.0)) <= 1e-9
        w = 2.0 * fs * math.tan(math.pi / 8.0)  # the analogue frequency of fs / 8
        analogue = 10.0 * math.log10((1.0 + (w * t2 * 1e-6) ** 2) / (1.0 + (w * t1 * 1e-6) ** 2))
        assert abs(db(s, fs / 8.0) - analogue) <= 1e-9, (t1, t2, fs)
        if t2 == 0.0:
            assert db(s, fs / 2) < -250.0


@pytest.mark.parametrize("fs", (44100.0, 48000.0, 192000.0))
def test_preemphasis_then_deemphasis_gives_the_impulse_back(omx, fs):
    pre = filter_design(omx, FilterSpec(fr.PREEMPHASIS, 0, 0.0, 0.0, 0.0, 50.0, 15.0), fs)
    de = filter_design(omx, FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, 50.0, 15.0), fs)
    both = filter_cascade(omx, pre, de)
    assert int(both["n_sections"]) == 2 and sections_of(both) == sections_of(pre) + sections_of(de)
    y = impulse_response(sections_of(both), 4096)
    assert abs(y[0] - 1.0) <= 1e-12 and np.abs(y[1:]).max() <= 1e-12
    # without a zero the inverse has its pole on the unit circle
    refused(UNSUPPORTED, filter_design, omx, FilterSpec(fr.PREEMPHASIS, 0, 0.0, 0.0, 0.0, 75.0), fs)


def test_response_is_the_steady_state_of_a_long_sine(omx):
    fs, hz, n = 48000.0, 1500.0, 48000
    for name, spec, kw in specs(fs):
        sections = fr.design(fs=fs, **kw)
        mag_db, phase = filter_response(omx, sections, fs, hz)
        h = fr.response(sections, fs, hz)
        assert abs(mag_db - 20.0 * math.log10(abs(h))) <= 1e-9 and abs(phase - math.atan2(h.imag, h.real)) <= 1e-9, name
    for name in ("highpass4", "peaking+", "deemphasis50/15"):
        kw = dict((n_, k) for n_, _, k in specs(fs))[name]
        sections = fr.design(fs=fs, **kw)
        t = np.arange(n) / fs
        x = (0.5 * np.sin(2.0 * np.pi * hz * t)).astype(np.float32)[:, None]
        coef, count, bypass = fr.lane_table([sections], None, 1, 1)
        y = np.zeros((n, 1))
        fr.run(x, coef, count, bypass, unrounded=y)
        tail = slice(n - 4800, n)  # 150 whole periods, behind every transient
        basis = np.exp(-2j * np.pi * hz * t[tail])
        got = 2.0 * (y[tail, 0] * basis).mean() / (2.0 * (x[tail, 0].astype(np.float64) * basis).mean())
        mag_db, phase = filter_response(omx, sections, fs, hz)
        assert abs(20.0 * math.log10(abs(got)) - mag_db) <= 1e-4 and abs(np.angle(got) - phase) <= 1e-5, (name, got, mag_db, phase)


# ---------------------------------------------------------------- refusals
def test_design_refusals(omx):
    fs = 48000.0
    bad = [FilterSpec(9, 0, 100.0), FilterSpec(fr.HIGHPASS, 3, 100.0), FilterSpec(fr.HIGHPASS, 0, 100.0), FilterSpec(fr.PEAKING, 4, 100.0),
           FilterSpec(fr.DC_BLOCK, 2, 5.0), FilterSpec(fr.LOWPASS, 2, 0.0), FilterSpec(fr.LOWPASS, 2, -5.0), FilterSpec(fr.LOWPASS, 2, math.nan),
           FilterSpec(fr.LOWPASS, 2, math.inf), FilterSpec(fr.LOWPASS, 2, 24000.0), FilterSpec(fr.LOWPASS, 2, 30000.0),
           FilterSpec(fr.LOWPASS, 2, 100.0, math.nan), FilterSpec(fr.LOWPASS, 2, 100.0, -1.0), FilterSpec(fr.PEAKING, 0, 100.0, 1.0, math.inf),
           FilterSpec(fr.LOW_SHELF, 0, 100.0, 1.0, math.nan), FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, 0.0),
           FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, math.nan), FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, 50.0, 50.0),
           FilterSpec(fr.DEEMPHASIS, 0, 0.0, 0.0, 0.0, 50.0, -1.0)]
    for spec in bad:
        refused(INVALID, filter_design, omx, spec, fs)
    for rate in (0.0, -48000.0, math.nan, math.inf):
        refused(INVALID, filter_design, omx, FilterSpec(fr.HIGHPASS, 2, 100.0), rate)
    # a DC blocker whose R = 1 - 2 pi f / fs leaves the unit circle
    refused(UNSUPPORTED, filter_design, omx, FilterSpec(fr.DC_BLOCK, 0, 16000.0), fs)
    design = omx.fn("program_filter_design", C.c_int, [C.c_void_p, C.c_double, C.c_void_p])
    spec, out = FilterSpec(fr.HIGHPASS, 2, 100.0).to_c(), CProgramFilter()
    assert design(None, fs, C.byref(out)) == INVALID and design(C.byref(spec), fs, None) == INVALID
    # a refused design writes nothing
    canary = np.full((1,), 0x5A, np.uint8).repeat(88).view(FILTER_DTYPE)
    bad_spec = FilterSpec(fr.HIGHPASS, 3, 100.0).to_c()
    assert design(C.byref(bad_spec), fs, canary.ctypes.data) == INVALID and canary.tobytes() == b"\x5a" * 88


def test_check_refusals_and_the_stability_triangle(omx):
    ok = (1.0, 0.0, 0.0, -1.2, 0.5)
    assert filter_check(omx, [ok]) == 0 and filter_check(omx, [ok, ok]) == 0
    for bad in (math.nan, math.inf, -math.inf):
        for at in range(5):
            sec = list(ok)
            sec[at] = bad
            refused(INVALID, filter_check, omx, [sec])
            refused(INVALID, filter_check, omx, [ok, sec])
    table = filter_table([[ok]])
    for n in (0, 3, 0xFFFFFFFF):
        table[0]["n_sections"] = n
        refused(INVALID, filter_check, omx, table[0])
    assert omx.fn("program_filter_check", C.c_int, [C.c_void_p])(None) == INVALID
    # the triangle |a2| < 1 && |a1| < 1 + a2: its edges are outside, one ulp inside is inside
    below_one = math.nextafter(1.0, 0.0)
    for a1, a2, inside in ((0.0, 1.0, False), (0.0, below_one, True), (0.0, -1.0, False), (0.0, -below_one, True),
                           (1.5, 0.5, False), (-1.5, 0.5, False), (math.nextafter(1.5, 0.0), 0.5, True),
                           (-math.nextafter(1.5, 0.0), 0.5, True), (2.0, 1.0, False), (1.0, 0.0, False), (below_one, 0.0, True)):
        assert fr.stable((1.0, 0.0, 0.0, a1, a2)) == inside
        if inside:
            assert filter_check(omx, [(1.0, 0.0, 0.0, a1, a2)]) == 0
            assert filter_check(omx, [ok, (1.0, 0.0, 0.0, a1, a2)]) == 0
        else:
            refused(UNSUPPORTED, filter_check, omx, [(1.0, 0.0, 0.0, a1, a2)])
            refused(UNSUPPORTED, filter_check, omx, [ok, (1.0, 0.0, 0.0, a1, a2)])


def test_cascade_response_plan_refusals(omx):
    one, two = [(1.0, 0.0, 0.0, -0.5, 0.0)], [(1.0, 0.0, 0.0, -0.5, 0.0), (0.5, 0.0, 0.0, 0.25, 0.0)]
    assert sections_of(filter_cascade(omx, one, one)) == one + one
    refused(INVALID, filter_cascade, omx, one, two)
    refused(INVALID, filter_cascade, omx, two, one)
    empty = filter_table([one])
    empty[0]["n_sections"] = 0
    refused(INVALID, filter_cascade, omx, empty[0], one)
    cascade = omx.fn("program_filter_cascade", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    t = filter_table([one])
    assert cascade(None, t.ctypes.data, t.ctypes.data) == INVALID and cascade(t.ctypes.data, t.ctypes.data, None) == INVALID
    for fs, hz in ((0.0, 10.0), (math.nan, 10.0), (48000.0, math.nan), (48000.0, -1.0), (-1.0, 10.0)):
        refused(INVALID, filter_response, omx, one, fs, hz)
    refused(INVALID, filter_response, omx, empty[0], 48000.0, 10.0)
    for ch, fs in ((0, 48000.0), (9, 48000.0), (2, 0.0), (2, math.nan), (2, -1.0)):
        refused(INVALID, filter_plan, omx, ch, fs)
    assert omx.fn("program_filter_plan", C.c_int, [C.c_uint32, C.c_double, C.c_void_p])(2, 48000.0, None) == INVALID
    for ch in range(1, 9):
        info = filter_plan(omx, ch, 48000.0)
        assert (int(info["chunk_frames"]), int(info["tile_frames"]), int(info["channels"])) == (fr.CHUNK_FRAMES, fr.TILE_FRAMES, ch)
        assert int(info["streams_per_wavefront"]) == {1: 64, 2: 32, 3: 16, 4: 16}.get(ch, 8)


def test_structure_sizes():
    assert (C.sizeof(CProgramFilterSection), C.sizeof(CProgramFilter), C.sizeof(CProgramFilterSpec), C.sizeof(CProgramFilterInfo),
            C.sizeof(CProgramFilterRecord)) == (40, 88, 48, 16, 48)
    assert (FILTER_DTYPE.itemsize, FILTER_INFO_DTYPE.itemsize, FILTER_RECORD_DTYPE.itemsize, fr.RECORD_DTYPE.itemsize) == (88, 16, 48, 48)
    assert FILTER_RECORD_DTYPE == fr.RECORD_DTYPE and FILTER_BYPASS == fr.BYPASS == 0xFFFFFFFF


# ---------------------------------------------------------------- the model of the time-parallel schedule
def hard_inputs(fs, n, seed=5):
    """DESIGN.md section 10's hard inputs as f32 [n][4]: DC 0.5, a 5 Hz sine at 0.5, noise at -6 dBFS, noise at -66 dBFS"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return np.stack([np.full(n, 0.5), 0.5 * np.sin(2.0 * np.pi * 5.0 * t + 1.0), rng.uniform(-0.5, 0.5, n),
                     rng.uniform(-0.5, 0.5, n) * 1e-3], 1).astype(np.float32)


def hard_filters(fs):
    return {"highpass4@20": fr.design(fr.HIGHPASS, fs, 20.0, order=4), "dc_block@5": fr.design(fr.DC_BLOCK, fs, 5.0)}


@pytest.mark.parametrize("fs", (48000.0, 192000.0))
def test_model_of_the_time_parallel_schedule_holds_the_bar_with_a_factor_4_to_spare(fs):
    n = 6 * fr.CHUNK_FRAMES + 17
    x = hard_inputs(fs, n)
    for name, sections in hard_filters(fs).items():
        assert fr.time_parallel_ok(sections), (name, fs, fr.predicted_start_error(sections))
        coef, count, bypass = fr.lane_table([sections], None, 1, x.shape[1])
        u_ref, u_tp = np.zeros(x.shape), np.zeros(x.shape)
        ref, _ = fr.run(x, coef, count, bypass, unrounded=u_ref)
        tp, _ = fr.run_time_parallel(x, sections, unrounded=u_tp)
        for lane in range(x.shape[1]):
            bar = 2.0 ** -23 * max(np.abs(x[:, lane]).max(), np.abs(ref[:, lane]).max())
            before_rounding = np.abs(u_tp[:, lane] - u_ref[:, lane]).max()
            after = np.abs(tp[:, lane].astype(np.float64) - ref[:, lane]).max()
            print(f"{fs:.0f} {name} input {lane}: model before rounding {before_rounding / bar:.3e} of the bar, after {after / bar:.3e}")
            assert before_rounding <= bar / 4.0 and after <= bar, (name, fs, lane, before_rounding, after, bar)


def test_rule_accepts_every_designed_kind_and_rejects_the_undamped_resonator():
    for fs in RATES:
        for name, _, kw in specs(fs):
            sections = fr.design(fs=fs, **kw)
            assert fr.time_parallel_ok(sections), (name, fs, fr.predicted_start_error(sections))
    sections = resonator_768k()
    assert all(fr.stable(s) for s in sections)
    assert fr.predicted_start_error(sections) > 2.0 ** -25 and not fr.time_parallel_ok(sections)


def resonator_768k():
    """Two all-pole sections with their poles at 20 Hz and radius 1 - 1e-6 at 768 kHz: strictly stable, and over one work item its
    state grows by ten orders of magnitude: the filter the fall-back rule rejects"""
    w0, r = 2.0 * math.pi * 20.0 / 768000.0, 1.0 - 1e-6
    return [(1.0, 0.0, 0.0, -2.0 * r * math.cos(w0), r * r)] * 2


# ---------------------------------------------------------------- the C99 demo
def test_c99_demo_builds_and_designs_without_a_device(tmp_path, omx):
    exe = build_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], words[1::2]))
    assert int(out["sections"]) == 2 and int(out["chunk"]) == fr.CHUNK_FRAMES and int(out["tile"]) == fr.TILE_FRAMES
    assert abs(float(out["corner_db"]) - 10.0 * math.log10(0.5)) <= 1e-6
    h = fr.response(fr.design(fr.HIGHPASS, 48000.0, 20.0, order=4), 48000.0, 1000.0)
    assert abs(float(out["tone_db"]) - 20.0 * math.log10(abs(h))) <= 1e-6

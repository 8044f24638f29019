"""Programme bank peaks (include/omx/program_peaks.h), CPU side: the numpy restatement (tests/program_peaks_ref.py) against the
reference-pinned oracle's sample-by-sample TruePeakMeter and against the EBU Tech 3341 true-peak tones; the new header, its record
and its exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_peaks_ref as ref
from openmeters_amd import capi
from openmeters_amd.capi import AudioBlock, LoudnessConfig, LoudnessProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omx", "program_peaks.h")
BASE_HEADER = os.path.join(ROOT, "include", "omx", "program_loudness.h")
FLOOR = -99.9


@pytest.mark.parametrize("fs,ch", [(44100.0, 2), (48000.0, 6), (96000.0, 8), (176400.0, 1), (192000.0, 2)])
def test_restatement_is_pinned_to_the_oracle(oracle, fs, ch):
    """LoudnessProcessor(oracle) fed a programme in uneven blocks (one channel starts with zeros: lazy channel activation), the
    per-channel maximum of true_peak_db over its snapshots against the restatement's dB.  Bar 1e-5 dB: the peaks themselves are the
    same f32 operations in the same order; what is left is numpy's f32 log standing in for logf (1 ulp of the dB value, <= 9.5e-7)."""
    x = ref.programme(3, fs, ch, 0.25)
    x[:700, ch - 1] = 0.0
    cuts = [0, 100, 356, 5000, len(x)]
    pos = capi.positions_fallback(ch)
    proc = LoudnessProcessor(oracle, LoudnessConfig(sample_rate=fs))
    got = np.full(ch, -np.inf)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        snap = proc.process_block(AudioBlock(x[lo:hi].reshape(-1), ch, fs, pos))
        got = np.maximum(got, np.asarray(snap.true_peak_db[:ch], np.float64))
    want = ref.restate(x, fs, ref.coefficients(oracle), FLOOR)
    worst = float(np.abs(got - want["true_peak_db"][:ch].astype(np.float64)).max())
    print(f"restatement vs oracle, {fs} Hz / {ch} ch: {worst:.2e} dB; oversampling {want['oversampling']}")
    assert want["oversampling"] == {44100.0: 4, 48000.0: 4, 96000.0: 2, 176400.0: 2, 192000.0: 1}[fs]
    assert worst <= 1e-5, (got, want["true_peak_db"])


@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0, 176400.0])
def test_restatement_meets_the_ebu_true_peak_tones(oracle, fs):
    """EBU Tech 3341 true-peak tones: fs/4 at 0 degrees and at 45 degrees (amplitude 0.5) read -6.0 dBTP, fs/4 at 45 degrees with
    amplitude 1.41 reads +3.0 dBTP, each within +0.2 / -0.4 dB; the 45 degree tones have a sample peak of -9.03 / -0.03 dBFS."""
    co = ref.coefficients(oracle)
    for phase, amplitude, want_tp, want_sp in ((0.0, 0.5, -6.0, -6.02), (45.0, 0.5, -6.0, -9.03), (45.0, 1.41, 3.0, -0.03)):
        r = ref.restate(ref.tone(fs, 4, phase, amplitude), fs, co, FLOOR)
        tp, sp = float(r["true_peak_db"][0]), float(r["sample_peak_db"][0])
        print(f"{fs} Hz fs/4 at {phase} deg x {amplitude}: true peak {tp:.3f} dBTP, sample peak {sp:.3f} dBFS")
        assert want_tp - 0.4 <= tp <= want_tp + 0.2, (fs, phase, amplitude, tp)
        assert abs(sp - want_sp) <= 0.01, (fs, phase, amplitude, sp)
    # fs/6 at 60 degrees and fs/8 at 67.5 degrees: the reference's 48-tap Hann-windowed sinc reads them 0.3 .. 0.7 dB high; that is the
    # reference's filter, so the EBU tolerance is NOT asserted for them (the GPU tests hold the product to the restatement on them)
    for divisor, phase in ((6, 60.0), (8, 67.5)):
        r = ref.restate(ref.tone(fs, divisor, phase, 0.5), fs, co, FLOOR)
        print(f"{fs} Hz fs/{divisor} at {phase} deg x 0.5: true peak {float(r['true_peak_db'][0]):.3f} dBTP (target -6.0)")
        assert r["true_peak"][0] >= r["sample_peak"][0]


def test_restatement_rules(oracle):
    """first frame of the peak, silence, a NaN sample (adds nothing for its own frame and the next 11), an infinite one"""
    co = ref.coefficients(oracle)
    quiet = ref.restate(np.zeros((100, 2), np.float32), 48000.0, co, FLOOR)
    assert quiet["true_peak"].max() == 0 and quiet["true_peak_frame"].max() == 0 and quiet["max_true_peak_db"] == np.float32(FLOOR)
    assert quiet["channels"] == 2 and quiet["oversampling"] == 4 and quiet["max_true_peak_channel"] == 0
    x = np.zeros((300, 1), np.float32)
    x[[50, 200], 0] = 0.25
    r = ref.restate(x, 48000.0, co, FLOOR)
    assert r["sample_peak_frame"][0] == 50 and r["sample_peak"][0] == np.float32(0.25) and 50 <= r["true_peak_frame"][0] < 62
    clean = ref.programme(1, 48000.0, 1, 0.05)
    dirty = clean.copy()
    dirty[1000, 0] = np.nan
    r = ref.restate(dirty, 48000.0, co, FLOOR)
    assert np.isfinite(r["true_peak"][0]) and r["true_peak"][0] >= r["sample_peak"][0] == np.abs(np.delete(clean[:, 0], 1000)).max()
    # the twelve outputs that hold the NaN are gone, nothing else: the peak of the interpolated outputs outside frames 1000 .. 1011
    outs = np.stack([np.abs(ref.interpolated(clean[:, 0], co[0][:, p])) for p in range(3)])
    outs[:, 1000:1012] = 0.0
    assert r["true_peak"][0] == max(outs.max(), r["sample_peak"][0])
    dirty[1000, 0] = np.inf
    assert np.isinf(ref.restate(dirty, 48000.0, co, FLOOR)["true_peak"][0])


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_its_record_is_288_bytes_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text('#include "omx/program_peaks.h"\nint main(void) { omx_program_peak_record r; r.channels = 0; '
                   'return (int)r.channels + (int)sizeof(r) - 288 + (int)sizeof(omx_program_loudness_record) - 168; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "use")], check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "use")]).returncode == 0
    from openmeters_amd.program_loudness import CProgramPeakRecord
    assert C.sizeof(CProgramPeakRecord) == 288
    syms = declared(HEADER)
    assert syms == ["omx_program_loudness_bank_fetch_peaks", "omx_program_loudness_bank_peaks", "omx_program_loudness_bank_set_peaks"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_peaks.h but not exported: {s}"
    assert len(declared(BASE_HEADER)) == 10     # the additive header leaves program_loudness.h as it was


def build_demo(tmp_path):
    """tests/c_abi/program_peaks_demo.c: a plain C99 host of the bank's peaks (needs the HIP runtime for its device buffer)"""
    out = str(tmp_path / "program_peaks_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_peaks_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))

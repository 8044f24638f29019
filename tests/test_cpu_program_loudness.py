"""Programme loudness (include/omx/program_loudness.h), CPU side: the numpy restatement (tests/program_loudness_ref.py) against the
EBU Tech 3341 / 3342 synthetic cases and against the reference-pinned oracle; the new header and its exports; the input condition
(gate margin) of every seeded case the GPU tests compare."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_loudness_ref as ref
from openmeters_amd import capi
from openmeters_amd.capi import AudioBlock, LoudnessConfig, LoudnessProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omx", "program_loudness.h")


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_restatement_meets_the_ebu_synthetic_cases(oracle, fs):
    """Tech 3341 #1-#5 within +-0.1 LU, Tech 3342 #1-#4 within +-1 LU (stereo 1 kHz sine)"""
    co = oracle.k_weighting_coefficients(ref.sanitize_rate(fs))
    for name, spans, want in ref.EBU_3341:
        r = ref.restate(ref.tone_programme(fs, spans), fs, capi.positions_fallback(2), co)
        print(name, fs, float(r["integrated_lufs"]))
        assert abs(float(r["integrated_lufs"]) - want) <= 0.1, (name, r["integrated_lufs"])
    for name, spans, want in ref.EBU_3342:
        r = ref.restate(ref.tone_programme(fs, spans), fs, capi.positions_fallback(2), co)
        print(name, fs, float(r["loudness_range_lu"]))
        assert abs(float(r["loudness_range_lu"]) - want) <= 1.0, (name, r["loudness_range_lu"])


def stepped_noise(fs, ch, seconds, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((int(fs * seconds), ch))
    steps = 10.0 ** (rng.uniform(-50, -10, int(seconds * 2) + 1) / 20.0)
    return (x * np.repeat(steps, int(fs / 2) + 1)[:len(x), None]).astype(np.float32)


@pytest.mark.parametrize("fs,ch", [(48000.0, 2), (44100.0, 6), (96000.0, 8)])
def test_restatement_is_pinned_to_the_oracle(oracle, fs, ch):
    """LoudnessProcessor(oracle) fed blocks of one segment: from the 4th block on its momentary loudness, from the 30th its short-term
    loudness, are L of the restatement's gating / short-term blocks within the project's loudness bar (1e-4 dB; measured ~2e-6: the
    oracle's f32 rounding).  Holds where uint(fs * 0.4f) = 4 seg and uint(fs * 3.0f) = 30 seg."""
    seg = ref.segment_frames(fs)
    assert int(np.float32(fs) * np.float32(0.4)) == 4 * seg and int(np.float32(fs) * np.float32(3.0)) == 30 * seg
    x = stepped_noise(fs, ch, 8.0, 11)
    pos = capi.positions_fallback(ch)
    e = ref.segment_energies(x, fs, pos, oracle.k_weighting_coefficients(ref.sanitize_rate(fs)))
    g, st = ref.sliding_mean(e, 4), ref.sliding_mean(e, 30)
    proc = LoudnessProcessor(oracle, LoudnessConfig(sample_rate=fs))
    worst = 0.0
    for j in range(len(e)):
        snap = proc.process_block(AudioBlock(x[j * seg:(j + 1) * seg].reshape(-1), ch, fs, pos))
        if j >= 3:
            worst = max(worst, abs(float(snap.momentary_loudness) - ref.level(g[j - 3])))
        if j >= 29:
            worst = max(worst, abs(float(snap.short_term_loudness) - ref.level(st[j - 29])))
    print(f"restatement vs oracle, {fs} Hz / {ch} ch: {worst:.2e} dB")
    assert len(st) > 40 and worst <= 1e-4


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_every_function_is_exported_as_a_bank_function(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text('#include "omx/program_loudness.h"\nint main(void) { omx_program_loudness_record r; r.overflow = 0; return (int)r.overflow + (int)sizeof(r) - 168; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "use")], check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "use")]).returncode == 0     # the record is 168 bytes, as the Python mirror
    from openmeters_amd.program_loudness import CProgramLoudnessRecord
    assert C.sizeof(CProgramLoudnessRecord) == 168
    syms = declared()
    assert len(syms) == 10
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_loudness.h but not exported: {s}"
        assert "_bank_" in s or "_debug_" in s, s


def test_no_cpu_fallback_without_a_device(omx):
    import openmeters_amd
    from openmeters_amd.program_loudness import ProgramLoudnessBank
    assert openmeters_amd.ProgramLoudnessBank is ProgramLoudnessBank
    if openmeters_amd.device_available():
        bank = ProgramLoudnessBank(omx, LoudnessConfig(), 2, 2, 60)    # (on a GPU host: the handle exists and reports floor values)
        assert bank.fetch(0).segments == 0
        return
    with pytest.raises(capi.OmxError) as e:
        ProgramLoudnessBank(omx, LoudnessConfig(), 4, 2, 60)
    assert e.value.status == capi.ERR_NO_DEVICE


def build_demo(tmp_path):
    """tests/c_abi/program_loudness_demo.c: a plain C99 host of the bank (needs the HIP runtime for its device buffers)"""
    out = str(tmp_path / "program_loudness_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_loudness_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_seeded_programmes_keep_their_distance_from_the_gates(oracle, fs, ch, seeds):
    """condition on the INPUTS of tests/test_gpu_program_loudness.py: a gate margin of at least 2e-3 LU (20 x the bar) in the restatement,
    and blocks on both sides of both gates"""
    co = oracle.k_weighting_coefficients(ref.sanitize_rate(fs))
    for seed in seeds:
        r = ref.restate(ref.programme(seed, fs, ch, ref.SEEDED_SECONDS), fs, capi.positions_fallback(ch), co)
        print(fs, ch, seed, f"margin {r['gate_margin']:.4f} LU", r["gating_blocks"], r["gating_above_absolute"], r["gating_above_relative"])
        assert r["gate_margin"] >= ref.GATE_MARGIN_MIN, (fs, ch, seed, r["gate_margin"])
        assert r["gating_blocks"] > r["gating_above_absolute"] > r["gating_above_relative"] > 0

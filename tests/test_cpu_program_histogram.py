"""Programme bank, bounded storage (include/omx/program_histogram.h), CPU side: the library's boundaries, the numpy restatement
(tests/program_histogram_ref.py) against the EBU cases and pinned to the stored restatement (program_loudness_ref.results), the
condition every input of tests/test_gpu_program_histogram.py has to meet (bin-clean), the new header, its structure and exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_histogram_ref as hr
import program_loudness_ref as ref
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
FS = 48000.0
SAME_BITS = ("momentary_energy", "short_term_energy", "max_momentary_energy", "max_short_term_energy")


@pytest.fixture(scope="module")
def B(omx):
    import openmeters_amd
    return openmeters_amd.histogram_boundaries(omx)


def coefficients(oracle, fs):
    return oracle.k_weighting_coefficients(ref.sanitize_rate(fs))


def energies(oracle, x, fs):
    return ref.segment_energies(x, fs, capi.positions_fallback(x.shape[1]), coefficients(oracle, fs))


def test_boundaries_from_the_library(B):
    """B[0] is the absolute gate bit for bit, B increases strictly, every entry within 4 ulp of numpy's value of the same expression"""
    assert B.shape == (hr.BINS + 1,) and B.dtype == np.float64
    assert B[0].tobytes() == np.float64(ref.ABSOLUTE_GATE).tobytes()
    assert (np.diff(B) > 0.0).all()
    want = hr.numpy_boundaries()
    ulps = np.abs(B - want) / np.spacing(want)
    print(f"boundaries: at most {ulps.max():.1f} ulp from numpy's")
    assert ulps.max() <= 4.0
    # bin i is (B[i], B[i + 1]]: a block on a boundary belongs below it, the top bin is open above
    assert list(hr.bin_of(np.array([np.nextafter(B[0], 1.0), B[1], np.nextafter(B[1], 1.0), B[999], B[1000], 1e30]), B)) == [0, 0, 1, 998, 999, 999]
    count, total = hr.fold(np.array([B[0], B[1], B[1], 1e30]), B)
    assert count[0] == 2 and total[0] == B[1] + B[1] and count[999] == 1 and count.sum() == 3   # (B[0] itself is not above the gate)


def test_ebu_cases_through_the_restatement(oracle, B):
    """the nine EBU cases at 48 kHz within the documents' own tolerances: Tech 3341 +-0.1 LU, Tech 3342 +-1 LU"""
    for name, spans, want in ref.EBU_3341 + ref.EBU_3342:
        r = hr.results(energies(oracle, ref.tone_programme(FS, spans), FS), B)
        print(name, r["integrated_lufs"], r["loudness_range_lu"])
        if name.startswith("3341"):
            assert abs(float(r["integrated_lufs"]) - want) <= 0.1, (name, r["integrated_lufs"])
        else:
            assert abs(float(r["loudness_range_lu"]) - want) <= 1.0, (name, r["loudness_range_lu"])


def pin(e, B, tag, measured):
    """the bounded restatement against the stored one on the same e[]"""
    got, want = hr.results(e, B), ref.results(e)
    h = got["histogram"]
    assert h["segments"] == len(e) and h["tail"].tobytes() == e[max(len(e) - hr.TAIL, 0):].tobytes()
    for f in ("segments", "gating_blocks", "short_term_blocks", "gating_above_absolute", "short_term_above_absolute"):
        assert got[f] == want[f], (tag, f, got[f], want[f])
    for f in SAME_BITS:
        assert np.float64(got[f]).tobytes() == np.float64(want[f]).tobytes(), (tag, f, got[f], want[f])
    assert hr.bin_clean(e, B), (tag, "not bin-clean: replace its seed")
    for f in ("gating_above_relative", "short_term_above_relative"):
        assert got[f] == want[f], (tag, f, got[f], want[f])
    exp = float(want["integrated_energy"])
    rel = abs(float(got["integrated_energy"]) - exp) / exp if exp > 0.0 else abs(float(got["integrated_energy"]))
    assert rel <= ref.energy_bound(want["gating_above_relative"]), (tag, rel, ref.energy_bound(want["gating_above_relative"]))
    d_lra = abs(float(got["loudness_range_lu"]) - float(want["loudness_range_lu"]))
    assert d_lra <= hr.LRA_BOUND_LU, (tag, d_lra)
    if want["short_term_above_relative"]:   # each range end is the mean of the bin that holds the stored mode's rank element
        for f in ("lra_low_energy", "lra_high_energy"):
            assert hr.bin_of(np.array([got[f]]), B)[0] == hr.bin_of(np.array([want[f]]), B)[0], (tag, f)
    measured["integrated_energy, relative"] = max(measured.get("integrated_energy, relative", 0.0), rel)
    measured["loudness_range_lu"] = max(measured.get("loudness_range_lu", 0.0), d_lra)


@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_restatement_is_pinned_to_the_stored_restatement_seeded(oracle, B, fs, ch, seeds):
    """measured: loudness range at most 0.040 LU from the stored mode's (44.1 kHz, 6 ch, seed 2), integrated energy <= 3.1e-16 relative"""
    measured = {}
    for seed in seeds:
        pin(energies(oracle, ref.programme(seed, fs, ch, ref.SEEDED_SECONDS), fs), B, (fs, ch, seed), measured)
    print(fs, ch, {k: f"{v:.3e}" for k, v in measured.items()})


def test_restatement_is_pinned_to_the_stored_restatement_edges_and_ebu(oracle, B):
    """every 8 kHz input of the GPU file and the two EBU cases that go through the product.  Measured: loudness range at most 0.034 LU
    apart, integrated energy <= 6.4e-14 relative (3000 equal blocks in one bin; its bound is 3.4e-13)"""
    measured = {}
    for tag, x in hr.edge_inputs():
        pin(energies(oracle, x, hr.EDGE_RATE), B, tag, measured)
    for name, spans, _ in ref.EBU_3341 + ref.EBU_3342:
        if name in hr.EBU_THROUGH_THE_PRODUCT:
            pin(energies(oracle, ref.tone_programme(FS, spans), FS), B, name, measured)
    print({k: f"{v:.3e}" for k, v in measured.items()})


@pytest.mark.parametrize("kind", ["tone", "steps"])
def test_restatement_is_pinned_to_the_stored_restatement_long(oracle, B, kind):
    """12 000 segments.  Measured: loudness range 0.0 LU (tone) and 0.024 LU (steps) apart, integrated energy <= 6.9e-14 relative"""
    measured = {}
    e = energies(oracle, hr.long_programme(kind), ref.HOUR_RATE)
    assert len(e) == 12000
    pin(e, B, ("long", kind), measured)
    print(kind, {k: f"{v:.3e}" for k, v in measured.items()})


def test_range_programmes_fill_the_bins_they_are_meant_to(oracle, B):
    progs = hr.range_programmes()
    h = {name: hr.histogram(energies(oracle, x, hr.EDGE_RATE), B) for name, x in progs.items()}
    top = h["top bin"]
    assert top["gating_count"][999] == 47 and top["gating_count"].sum() == 47 and top["short_term_count"][999] == 21
    assert h["below the gate"]["gating_count"].sum() == 0 and h["below the gate"]["short_term_count"].sum() == 0
    eq = h["equal blocks"]
    assert eq["gating_count"].max() >= 2990 and eq["short_term_count"].max() >= 2960
    quiet = h["silence, then a tone"]
    assert 0 < quiet["gating_count"].sum() < 97


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_its_structure_has_its_size_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "omx/program_histogram.h"\nint main(void) { static omx_program_histogram h; h.tail_count = 0; '
                   'return (int)h.tail_count + (int)sizeof(h) - 32248 + (int)offsetof(omx_program_histogram, tail) - 32000 + '
                   '(int)offsetof(omx_program_histogram, segments) - 32232 + OMX_PROGRAM_HISTOGRAM_BINS - 1000 + OMX_PROGRAM_HISTOGRAM_TAIL - 29; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "use")], check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "use")]).returncode == 0
    import openmeters_amd
    assert C.sizeof(openmeters_amd.CProgramHistogram) == 32248
    assert openmeters_amd.CProgramHistogram.tail.offset == 32000 and openmeters_amd.CProgramHistogram.segments.offset == 32232
    syms = declared(os.path.join(INCLUDE, "program_histogram.h"))
    assert syms == ["omx_program_histogram_boundaries", "omx_program_loudness_bank_create_bounded", "omx_program_loudness_bank_fetch_histogram",
                    "omx_program_loudness_bank_is_bounded"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_histogram.h but not exported: {s}"
    assert len(declared(os.path.join(INCLUDE, "program_loudness.h"))) == 10
    assert len(declared(os.path.join(INCLUDE, "program_peaks.h"))) == 3
    assert len(declared(os.path.join(INCLUDE, "program_timeline.h"))) == 4


def build_demo(tmp_path):
    """tests/c_abi/program_histogram_demo.c: a plain C99 host of a bounded bank next to a stored one that overflows"""
    out = str(tmp_path / "program_histogram_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_histogram_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


def test_create_bounded_without_a_device_is_an_error(omx):
    import openmeters_amd
    from openmeters_amd.program_loudness import ProgramLoudnessBank
    with pytest.raises(ValueError):
        ProgramLoudnessBank(omx, LoudnessConfig(), 2, 2, storage="ring")
    if openmeters_amd.device_available():
        bank = ProgramLoudnessBank(omx, LoudnessConfig(), 2, 2, storage="histogram")    # (on a GPU host: the handle exists and is empty)
        assert bank.is_bounded() and bank.fetch(0).segments == 0 and bank.fetch_histogram(1).segments == 0
        return
    with pytest.raises(capi.OmxError) as e:
        ProgramLoudnessBank(omx, LoudnessConfig(), 4, 2, storage="histogram")
    assert e.value.status == capi.ERR_NO_DEVICE

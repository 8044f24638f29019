"""Programme bank timeline and intervals (include/omx/program_timeline.h), CPU side: the numpy restatement
(tests/program_timeline_ref.py) pinned to program_loudness_ref.results, the EBU known answers through it, the new header, its
structures and exports, and the conditions the inputs of tests/test_gpu_program_timeline.py have to meet."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_loudness_ref as ref
import program_timeline_ref as tl
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omx", "program_timeline.h")
FLOOR = -99.9
FS = 48000.0
RESULT_FIELDS = tl.RECORD_ENERGIES + tl.RECORD_COUNTS + tl.RECORD_LEVELS


def coefficients(oracle, fs):
    return oracle.k_weighting_coefficients(ref.sanitize_rate(fs))


def energies(oracle, x, fs):
    return ref.segment_energies(x, fs, capi.positions_fallback(x.shape[1]), coefficients(oracle, fs))


def same(a, b):
    """equal as numbers of the same type (the restatement forms the same numpy operations on the same array contents)"""
    return type(a) is type(b) and a == b if isinstance(a, np.floating) else float(a) == float(b)


def pin(e):
    """timeline(e)[j] is results(e[:j + 1]) field for field, the margin included, and intervals(e, a, c) is results(e[a:a + c])"""
    e = np.asarray(e, np.float64)
    got, p = tl.timeline(e, floor=FLOOR), tl.Prefixes(e)
    assert len(got) == len(e)
    for j in range(len(e)):
        want = ref.results(e[:j + 1], FLOOR)
        for f in ("integrated_energy", "relative_threshold_energy", "momentary_lufs", "short_term_lufs", "integrated_lufs",
                  "gating_above_absolute", "gating_above_relative"):
            assert float(got[j][f]) == float(want[f]), (j, f, got[j][f], want[f])
        assert got[j]["valid"] == 1 and p.margin(j) == want["gate_margin"], (j, p.margin(j), want["gate_margin"])
    rng = np.random.default_rng(len(e))
    for _ in range(40):
        c = int(rng.integers(0, len(e) + 1))
        a = int(rng.integers(0, len(e) - c + 1))
        got_i, want = tl.intervals(e, a, c, 4800, FLOOR), ref.results(e[a:a + c], FLOOR)
        for f in RESULT_FIELDS + ("gate_margin",):
            assert float(got_i[f]) == float(want[f]), (a, c, f, got_i[f], want[f])
        assert got_i["frames"] == c * 4800 and got_i["overflow"] == 0 and got_i["max_true_peak_db"] == np.float32(FLOOR)


@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_restatement_is_pinned_to_the_result_pass_restatement_seeded(oracle, fs, ch, seeds):
    for seed in seeds:
        pin(energies(oracle, ref.programme(seed, fs, ch, ref.SEEDED_SECONDS), fs))


def test_restatement_is_pinned_to_the_result_pass_restatement_ebu_and_hard_inputs(oracle):
    for name, spans, _ in ref.EBU_3341 + ref.EBU_3342:
        pin(energies(oracle, ref.tone_programme(FS, spans), FS))
    for kind in ref.HARD_KINDS:
        pin(energies(oracle, ref.hard_input(kind, FS, 2), FS))
    e = energies(oracle, ref.programme(1, FS, 2, 5.0), FS)
    beyond = tl.timeline(e, first=len(e) - 2, stride=3, count=3, floor=FLOOR)
    assert beyond[0]["valid"] == 1 and beyond[1] == tl.empty_row(FLOOR) and beyond[2] == tl.empty_row(FLOOR)
    assert tl.timeline(e, 5, 7, 4, FLOOR).tobytes() == tl.timeline(e, floor=FLOOR)[5:5 + 7 * 4:7].tobytes()


def test_known_answers_through_the_restatement(oracle):
    """EBU Tech 3341 #3 and #4: -36.0 LUFS at the end of the first -36 dBFS span, -23.0 LUFS at the end; #4's middle minute alone
    -23.0 LUFS; Tech 3342 #1: its halves read -20 and -30 LUFS with a range below 1 LU each, the whole has a range of 10 LU"""
    cases = {name: spans for name, spans, _ in ref.EBU_3341 + ref.EBU_3342}
    for name, span_end in (("3341-3", 100), ("3341-4", 200)):
        e = energies(oracle, ref.tone_programme(FS, cases[name]), FS)
        rows, whole = tl.timeline(e, floor=FLOOR), ref.results(e, FLOOR)
        print(name, "running integrated at the end of the first -36 dBFS span:", rows[span_end - 1]["integrated_lufs"], "at the end:",
              rows[-1]["integrated_lufs"])
        assert abs(float(rows[span_end - 1]["integrated_lufs"]) + 36.0) <= 0.1
        assert abs(float(rows[-1]["integrated_lufs"]) + 23.0) <= 0.1
        assert rows[-1]["gating_above_absolute"] == whole["gating_above_absolute"] and rows[-1]["gating_above_relative"] == whole["gating_above_relative"]
        assert rows[-1]["relative_threshold_energy"] == whole["relative_threshold_energy"]
    e = energies(oracle, ref.tone_programme(FS, cases["3341-4"]), FS)
    middle = tl.intervals(e, 200, 600, 4800, FLOOR)
    assert abs(float(middle["integrated_lufs"]) + 23.0) <= 0.1, middle["integrated_lufs"]
    e = energies(oracle, ref.tone_programme(FS, cases["3342-1"]), FS)
    first, second, whole = tl.intervals(e, 0, 200, 4800, FLOOR), tl.intervals(e, 200, 200, 4800, FLOOR), tl.intervals(e, 0, 400, 4800, FLOOR)
    print("3342-1 halves:", first["integrated_lufs"], first["loudness_range_lu"], second["integrated_lufs"], second["loudness_range_lu"],
          "whole LRA", whole["loudness_range_lu"])
    assert abs(float(first["integrated_lufs"]) + 20.0) <= 0.1 and abs(float(second["integrated_lufs"]) + 30.0) <= 0.2
    assert float(first["loudness_range_lu"]) < 1.0 and float(second["loudness_range_lu"]) < 1.0
    assert abs(float(whole["loudness_range_lu"]) - 10.0) <= 1.0


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_its_structures_have_their_sizes_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text('#include "omx/program_timeline.h"\nint main(void) { omx_program_timeline_row r; omx_program_interval i; r.valid = 0; '
                   'i.stream = 0; return (int)r.valid + (int)i.stream + (int)sizeof(r) - 40 + (int)sizeof(i) - 24 + '
                   '(int)sizeof(omx_program_loudness_record) - 168; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "use")], check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "use")]).returncode == 0
    import openmeters_amd
    from openmeters_amd.program_loudness import INTERVAL_DTYPE, RECORD_DTYPE, TIMELINE_ROW_DTYPE, CProgramLoudnessRecord
    assert C.sizeof(openmeters_amd.CProgramTimelineRow) == 40 and C.sizeof(openmeters_amd.CProgramInterval) == 24
    assert TIMELINE_ROW_DTYPE == tl.ROW_DTYPE and INTERVAL_DTYPE.itemsize == 24
    for dtype, struct in ((TIMELINE_ROW_DTYPE, openmeters_amd.CProgramTimelineRow), (INTERVAL_DTYPE, openmeters_amd.CProgramInterval),
                          (RECORD_DTYPE, CProgramLoudnessRecord)):
        assert [(n, dtype.fields[n][1]) for n in dtype.names] == [(n, getattr(struct, n).offset) for n, _ in struct._fields_]
    syms = declared(HEADER)
    assert syms == ["omx_program_loudness_bank_fetch_intervals", "omx_program_loudness_bank_fetch_timeline",
                    "omx_program_loudness_bank_measure_intervals", "omx_program_loudness_bank_timeline"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_timeline.h but not exported: {s}"
    assert len(declared(os.path.join(ROOT, "include", "omx", "program_loudness.h"))) == 10
    assert len(declared(os.path.join(ROOT, "include", "omx", "program_peaks.h"))) == 3


def build_demo(tmp_path):
    """tests/c_abi/program_timeline_demo.c: a plain C99 host of the timeline and the intervals"""
    out = str(tmp_path / "program_timeline_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_timeline_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


# ---------------------------------------------------------------- conditions on the inputs of the GPU tests
def assert_cap(e, tag, first=0, stride=1):
    clean = tl.clean_rows(e, first, stride)
    unclean = int((~clean).sum())
    print(f"{tag}: {unclean} rows of {len(clean)} within {ref.RESULT_PASS_MARGIN_MIN} LU of a gate")
    assert unclean <= tl.UNCLEAN_SHARE_MAX * len(clean), (tag, unclean, len(clean))


@pytest.mark.parametrize("fs,ch,seeds", ref.SEEDED_CASES)
def test_seeded_programmes_have_clean_rows(oracle, fs, ch, seeds):
    for seed in seeds:
        assert_cap(energies(oracle, ref.programme(seed, fs, ch, ref.SEEDED_SECONDS), fs), (fs, ch, seed))


def test_edge_and_ebu_programmes_have_clean_rows(oracle):
    for s, x in enumerate(tl.edge_programmes(65)):
        e = energies(oracle, x, tl.EDGE_RATE)
        if len(e):
            assert_cap(e, ("edges", s))
    for name, spans, _ in ref.EBU_3341 + ref.EBU_3342:
        if name in tl.EBU_THROUGH_THE_PRODUCT:
            assert_cap(energies(oracle, ref.tone_programme(FS, spans), FS), name)


@pytest.mark.parametrize("kind", ["tone", "steps"])
def test_hour_programmes_have_clean_rows(oracle, kind):
    e = energies(oracle, ref.hour_programme(kind), ref.HOUR_RATE)
    assert len(e) == 36000
    assert_cap(e, ("one hour", kind), stride=tl.HOUR_STRIDE)
    p = tl.Prefixes(e)
    for j in (3, 29, 30, 5000, 35999):   # the prefix form of the margin is the result restatement's own
        assert p.margin(j) == ref.results(e[:j + 1])["gate_margin"]


def test_four_hour_programme_has_clean_rows(oracle):
    x = ref.hour_programme("steps", seconds=ref.FOUR_HOURS_SECONDS, seed=ref.FOUR_HOURS_SEED)
    e = ref.segment_energies_long(x, ref.HOUR_RATE, capi.positions_fallback(1), coefficients(oracle, ref.HOUR_RATE))
    assert len(e) == 144000
    assert_cap(e, "four hours", stride=tl.FOUR_HOURS_STRIDE)


def test_every_drawn_interval_keeps_its_distance_from_the_gates(oracle):
    es = [energies(oracle, tl.interval_bank_programme(s), tl.INTERVAL_RATE) for s in range(tl.INTERVAL_STREAMS)]
    drawn = tl.draw_intervals([len(e) for e in es])
    worst = min(tl.intervals(es[s], a, c)["gate_margin"] for s, a, c in drawn)
    lengths = {c for _, _, c in drawn}
    print(f"{len(drawn)} intervals over {len(es)} streams of {min(map(len, es))} .. {max(map(len, es))} segments: smallest margin {worst:.2e} LU")
    assert 3900 <= len(drawn) <= 4100 and set(tl.EDGE_LENGTHS) <= lengths
    assert any(a == 0 and c > 30 for _, a, c in drawn) and any(a + c == len(es[s]) and a > 0 for s, a, c in drawn)
    assert worst >= ref.RESULT_PASS_MARGIN_MIN

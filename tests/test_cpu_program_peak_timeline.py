"""Programme bank peak timeline (include/omx/program_peak_timeline.h), CPU side: the numpy restatement
(tests/program_peak_timeline_ref.py) against a case written out by hand and against the whole-programme restatement of
tests/program_peaks_ref.py; the new header, its two structures and its exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_peak_timeline_ref as ref
import program_peaks_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omx", "program_peak_timeline.h")
FLOOR = -99.9
EXPORTS = ["omx_program_loudness_bank_fetch_group_peaks", "omx_program_loudness_bank_fetch_interval_peaks",
           "omx_program_loudness_bank_fetch_peak_rows", "omx_program_loudness_bank_measure_group_peaks",
           "omx_program_loudness_bank_measure_interval_peaks", "omx_program_loudness_bank_peak_rows",
           "omx_program_loudness_bank_plan_part_gains", "omx_program_loudness_bank_set_peak_timeline"]


def test_hand_case_impulse_on_the_last_frame_of_a_segment():
    """3364 Hz: L = 336, three segments of silence with one sample of 0.5 on frame 335, the last of segment 0.  The 4x interpolator's
    output of frame 335 + i is 0.5 * fir4[i][p]; its largest tap, 0.8964651 = fir4[5][2] = fir4[6][0] (j = 23 and j = 25 of the
    48-tap windowed sinc), sits 5 and 6 frames behind the impulse.  So segment 0 holds the sample itself (every interpolated value in
    it is 0.5 * fir4[0][p] <= 0.5 * 0.0012), segment 1 holds the tail: true peak 0.5 * 0.8964651 = 0.44823256 at its frame 4 (340 of
    the programme; frame 341 has the same value and loses the tie), sample peak 0; segment 2 holds nothing."""
    coeffs = ref.coefficients()
    assert coeffs[0][5][2] == coeffs[0][6][0] == np.float32(0.8964651) and ref.segment_frames(3364.0) == 336
    x = np.zeros((1008, 1), np.float32)
    x[335, 0] = 0.5
    sp = ref.segment_peaks(x, 3364.0, coeffs)
    assert sp["L"] == 336 and sp["frames"] == 1008 and len(sp["true_peak"]) == 3
    assert sp["true_peak"][:, 0].tolist() == [0.5, float(np.float32(0.44823256)), 0.0]
    assert sp["true_offset"][:, 0].tolist() == [335, 4, 0]
    assert sp["sample_peak"][:, 0].tolist() == [0.5, 0.0, 0.0]
    assert sp["sample_offset"][:, 0].tolist() == [335, 0, 0]
    # rows: one per segment; one over all three (the earlier, larger peak); one that starts at segment 1 and runs past the end
    one = ref.rows(sp, 0, 1, 4)
    assert one["valid"].tolist() == [1, 1, 1, 0] and one["frames"].tolist() == [336, 336, 336, 0]
    assert one["true_peak"][:, 0].tolist() == [0.5, float(np.float32(0.44823256)), 0.0, 0.0]
    assert one["true_peak_offset"][:, 0].tolist() == [335, 4, 0, 0] and one["sample_peak_offset"][:, 0].tolist() == [335, 0, 0, 0]
    assert not one["true_peak"][:, 1:].any() and one[3].tobytes() == bytes(136)
    whole = ref.rows(sp, 0, 3, 1)[0]
    assert whole["true_peak"][0] == 0.5 and whole["true_peak_offset"][0] == 335 and whole["frames"] == 1008
    tail = ref.rows(sp, 1, 5, 1)[0]
    assert tail["true_peak"][0] == np.float32(0.44823256) and tail["true_peak_offset"][0] == 4 and tail["sample_peak"][0] == 0
    assert tail["frames"] == 672 and tail["valid"] == 1
    # parts: the tail is the peak of the programme DURING segment 1, with frames counted from the reset
    part = ref.part_peaks([sp], [(0, 1, 2), (0, 0, ref.TO_END)], None, FLOOR)
    assert part[0]["true_peak"][0] == np.float32(0.44823256) and part[0]["true_peak_frame"][0] == 340 and part[0]["sample_peak"][0] == 0
    assert part[0]["frames"] == 672 and part[0]["channels"] == 1 and part[0]["sample_peak_db"][0] == np.float32(FLOOR)
    assert abs(float(part[0]["max_true_peak_db"]) - 20 * np.log10(0.44823256)) < 1e-5
    assert part[1]["true_peak_frame"][0] == 335 and part[1]["frames"] == 1008 and part[1]["true_peak"][0] == 0.5


def test_the_formula_coefficients_are_the_oracles(oracle):
    fir4, fir2 = ref.coefficients()
    o4, o2 = pref.coefficients(oracle)
    assert fir4.tobytes() == o4.tobytes() and fir2.tobytes() == o2.tobytes()


@pytest.mark.parametrize("fs,ch,frames", [(3364.0, 1, 2000), (8000.0, 3, 4001), (48000.0, 2, 10001), (96000.0, 2, 20000), (192000.0, 1, 40000)])
def test_identity_the_maximum_of_all_rows_is_the_whole_programmes_peak(fs, ch, frames):
    """value and frame of every channel, on programmes with NaN, infinities, -0.0 and denormals; and the interval over the complete
    segments joined with the open row likewise"""
    coeffs = ref.coefficients()
    x = ref.hard_programme(int(fs) % 97, frames, ch)
    want = pref.restate(x, fs, coeffs, FLOOR)
    sp = ref.segment_peaks(x, fs, coeffs)
    L, segs = sp["L"], len(sp["true_peak"])
    assert segs == -(-frames // L)
    everything = ref.rows(sp, 0, segs, 1)[0]
    part = ref.part_peaks([sp], [(0, 0, ref.TO_END)], None, FLOOR)[0]
    open_row = ref.rows(sp, frames // L, 1, 1)[0]
    for c in range(ch):
        for kind in ("true_peak", "sample_peak"):
            assert everything[kind][c].tobytes() == want[kind][c].tobytes(), (c, kind)
            assert everything[kind + "_offset"][c] == want[kind + "_frame"][c], (c, kind)
            value, frame = part[kind][c], int(part[kind + "_frame"][c])
            if open_row["valid"] and open_row[kind][c] > value:
                value, frame = open_row[kind][c], (frames // L) * L + int(open_row[kind + "_offset"][c])
            assert value.tobytes() == want[kind][c].tobytes() and frame == want[kind + "_frame"][c], (c, kind)
    assert everything["frames"] == frames and part["frames"] == (frames // L) * L


def test_group_rules_of_the_restatement():
    """equal peaks in two members: the first member in table order wins, also when it lies later in the stream; an empty group"""
    coeffs = ref.coefficients()
    x = np.zeros((336 * 4, 2), np.float32)
    x[100, 0] = x[336 * 2 + 7, 0] = 0.25
    x[336 * 3 + 1, 1] = -0.125
    sp = ref.segment_peaks(x, 3364.0, coeffs)
    members = [(0, 2, 1), (0, 0, 1), (0, 3, 1)]
    got = ref.part_peaks([sp], members, [(0, 2), (1, 2), (0, 0), (0, 3)], FLOOR)
    assert got[0]["sample_peak_member"][0] == 0 and got[0]["sample_peak_frame"][0] == 336 * 2 + 7 and got[0]["sample_peak"][0] == 0.25
    assert got[1]["sample_peak_member"][0] == 0 and got[1]["sample_peak_frame"][0] == 100
    assert got[1]["sample_peak_member"][1] == 1 and got[1]["sample_peak_frame"][1] == 336 * 3 + 1 and got[1]["sample_peak"][1] == 0.125
    assert got[2]["frames"] == 0 and got[2]["channels"] == 0 and got[2]["max_true_peak_db"] == np.float32(FLOOR) and not got[2]["true_peak"].any()
    assert got[3]["frames"] == 336 * 3 and got[3]["max_true_peak_channel"] == 0 and got[3]["channels"] == 2
    single = ref.part_peaks([sp], members[:1], [(0, 1)], FLOOR)
    assert single.tobytes() == ref.part_peaks([sp], members[:1], None, FLOOR).tobytes()


def commented_offsets(struct):
    """{field: offset} from the `offset N` comments of one structure of the header (a line that declares two fields names two offsets)"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/" % (struct, struct), text, re.S)
    out = {}
    for line in body.group(1).splitlines():
        m = re.match(r"\s*\w+ ([^;]+);\s*/\* offset\s+([\d, ]+)", line)
        if m:
            names = [n.strip().split("[")[0] for n in m.group(1).split(",")]
            for name, offset in zip(names, [int(v) for v in m.group(2).split(",")]):
                out[name] = offset
    return out, int(body.group(2))


def test_structures_have_the_sizes_and_offsets_the_header_states():
    from openmeters_amd.program_loudness import PART_PEAK_DTYPE, PEAK_ROW_DTYPE, CProgramPartPeak, CProgramPeakRow
    for struct, ctype, dtype, size in (("omx_program_peak_row", CProgramPeakRow, PEAK_ROW_DTYPE, 136),
                                       ("omx_program_part_peak", CProgramPartPeak, PART_PEAK_DTYPE, 344)):
        offsets, stated = commented_offsets(struct)
        assert stated == size == C.sizeof(ctype) == dtype.itemsize, struct
        assert set(offsets) == {n for n, _ in ctype._fields_} == set(dtype.names), (struct, offsets)
        for name, offset in offsets.items():
            assert getattr(ctype, name).offset == offset == dtype.fields[name][1], (struct, name)
    assert ref.PEAK_ROW_DTYPE == PEAK_ROW_DTYPE and ref.PART_PEAK_DTYPE == PART_PEAK_DTYPE


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_function_is_exported(omx):
    assert declared(HEADER) == EXPORTS
    for s in EXPORTS:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_peak_timeline.h but not exported: {s}"


def test_header_compiles_as_c99_and_as_cxx_with_the_stated_sizes(tmp_path):
    body = ('#include <stddef.h>\n#include "omx/program_peak_timeline.h"\n'
            "int main(void) { omx_program_peak_row r; omx_program_part_peak p; r.valid = 0; p.channels = 0;\n"
            "  return (int)r.valid + (int)p.channels + (int)sizeof(r) - 136 + (int)sizeof(p) - 344 + (int)offsetof(omx_program_peak_row, frames) - 128\n"
            "    + (int)offsetof(omx_program_part_peak, true_peak) - 200 + (int)offsetof(omx_program_part_peak, max_true_peak_channel) - 336; }\n")
    for compiler, std, name in (("gcc", "-std=c99", "use.c"), ("g++", "-std=c++11", "use.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".out"))
        subprocess.run([compiler, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       check=True, capture_output=True)
        assert subprocess.run([exe]).returncode == 0, compiler


def build_demo(tmp_path):
    """tests/c_abi/program_peak_timeline_demo.c: a plain C99 host of the peak timeline (needs the HIP runtime for its device buffer)"""
    out = str(tmp_path / "program_peak_timeline_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_peak_timeline_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib",
           "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))

"""Programme bank dynamics stage (include/omx/program_dynamics.h), CPU side: the header as C99, its structures' sizes and offsets, the
exported functions and the Python surface; the LOG and EXP literals (in the restatement and as the library exports them) against
exact values from Python integers; the restatement (tests/program_dynamics_ref.py) against itself: the fast form against a
frame-by-frame evaluation, pieces against the whole, the bound E[j] <= Gt[t] 2^16, exact settling, pass-through bits; design, points,
gain, time, frames, latency and plan against the restatement, every refusal of the host-only functions with the outputs still holding
their sentinels; the stand-alone check program under the sanitizers.

Bars.  Everything is equal on bits except design and from_points against the restatement: both run the same f64 operations and
floor(), no libm function, so every table entry is expected equal; the bar is +-1 unit of 2^-16 octave, what a platform whose
floor(v + 0.5) meets a rounding tie differently could move.  The test prints what it measures (0 here)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import program_dynamics_ref as dr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
#        threshold, ratio, knee, expander threshold, expander ratio, range, make-up
SPECS = [(-20.0, 4.0, 0.0, -60.0, 1.0, math.inf, 0.0), (-20.0, 4.0, 6.0, -60.0, 2.0, 24.0, 3.0), (-30.0, math.inf, 12.0, -70.0, 1.0, 0.0, 0.0),
         (-3.0, 1.5, 0.0, -40.0, 10.0, math.inf, -2.5), (12.0, 20.0, 24.0, -90.0, 4.0, 60.0, 40.0), (-240.0, 8.0, 1.0, 48.0, 1.5, 300.0, 250.0),
         (0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0)]
POINT_SETS = [[(-70.0, -90.0), (-40.0, -40.0), (-20.0, -20.0), (0.0, -10.0)], [(-20.0, -20.0)], [(-300.0, -10.0), (100.0, -10.0)],
              [(-96.0 + 6.0 * i, -96.0 + 6.0 * i + (7.0 * i * i) % 11 - 5) for i in range(16)]]


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def last_error(omx):
    return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")


def noise_with_bursts(seed, n, ch):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, ch)) * 0.002).astype(np.float32)      # about -54 dB: under the knee of the curves below
    for b in range(100, n, 300):
        x[b:b + 50 + 7 * seed] *= np.float32(150.0)
    return x


# ---------------------------------------------------------------- the tables
def test_log_and_exp_literals_are_the_exact_integers(omx):
    import openmeters_amd as oa
    log_exact = [((256 + i) ** 65536).bit_length() - 1 - 8 * 65536 for i in range(257)]

    def exp_exact(i):
        v = 1 << (256 * 40 + i)
        for _ in range(8):
            v = math.isqrt(v)
        return v

    exp_exact = [exp_exact(i) for i in range(257)]
    assert dr.LOG == log_exact and dr.EXP == exp_exact
    lg, ex = oa.dynamics_tables(omx)
    assert lg.dtype == np.int32 and ex.dtype == np.uint64
    assert lg.tolist() == log_exact and [int(v) for v in ex] == exp_exact
    # what the issue's prototype found: floor of the double results at all 257 entries, level and factor close to log2 and exp2
    assert all(dr.LOG[i] == math.floor(65536.0 * math.log2(1.0 + i / 256.0)) for i in range(257))
    assert all(dr.EXP[i] == math.floor(2.0 ** (40.0 + i / 256.0)) for i in range(257))
    a = np.exp2(np.linspace(-39.9, 7.99, 20001)).astype(np.float32)
    L = dr.level(a[:, None], 1)
    assert np.abs(L / 65536.0 - np.log2(a.astype(np.float64))).max() <= 2.5e-5
    E = np.linspace(-40 * 2 ** 32, 40 * 2 ** 32, 20001).astype(np.int64)
    assert np.abs(dr.factor(E) / np.exp2(E / 2.0 ** 32) - 1.0).max() <= 1e-6


def test_level_at_its_ends_and_on_hard_values():
    f = np.float32
    key = np.array([[0.0], [-0.0], [1e-45], [2.0 ** -41], [2.0 ** -40], [1.0], [-1.0], [1.5], [255.99998], [256.0], [3e38], [np.inf], [-np.inf], [np.nan]], f)
    L = dr.level(key, 1).tolist()
    assert L[:4] == [dr.L_MIN] * 4 and L[4] == dr.L_MIN and L[5] == L[6] == 0 and L[7] == dr.LOG[128]
    assert dr.L_MAX - 1 <= L[8] <= dr.L_MAX and L[9:13] == [dr.L_MAX] * 4 and L[13] == dr.L_MIN
    # fmaxf semantics: a NaN channel is ignored beside a number; the mask leaves channels out
    two = np.array([[np.nan, 0.5], [0.25, np.nan], [1.0, 0.001]], f)
    assert dr.level(two, 3).tolist() == [-65536, -2 * 65536, 0] and dr.level(two, 2).tolist()[2] < -9 * 65536
    assert dr.level(two, 1).tolist()[0] == dr.L_MIN


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("A,H,d", [(1, 0, 1), (1, 0, dr.MAX_STEP), (16, 5, 1 << 27), (7, 0, 1 << 30), (33, 100, 1 << 25), (64, 3, 1 << 28)])
def test_fast_form_equals_the_frame_by_frame_form_and_keeps_the_bound(A, H, d):
    T = dr.design(-30.0, 4.0, 6.0)
    x = noise_with_bursts(A % 5, 700, 2)
    c = dr.Curve(T, 3, A, H, d)
    _out, _tr, E = dr.render(c, x)
    slow, Gt = dr.render_slow(c, x)
    assert (E == slow).all()
    t0 = int(T[0])
    for j in range(len(E)):      # E[j] <= Gt[t] 2^16 for every t in [j - H, j]
        window = [Gt[t] if t >= 0 else t0 for t in range(j - H, j + 1)]
        assert int(E[j]) <= min(window) << 16, j
    assert (E < 0).any() and ((E == 0).any() or d == 1)


def test_the_prototypes_burst_input_has_reduced_and_unity_frames():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3000, 1)) * 0.003).astype(np.float32)
    for b in range(300, 3000, 700):
        x[b:b + 120] *= np.float32(100.0)
    c = dr.Curve(dr.design(-20.0, 4.0), 1, 16, 40, int(60.0 / dr.OCTAVE_DB * 2 ** 32 / 48000.0))
    E = dr.render(c, x)[2]
    assert (E < 0).sum() > 100 and (E == 0).sum() > 100 and (E <= 0).all()


@pytest.mark.parametrize("A,H", [(1, 0), (2, 0), (16, 9), (40, 0)])
def test_any_cut_of_a_programme_gives_the_bytes_of_the_whole(A, H):
    n, ch = 400, 3
    x = noise_with_bursts(3, n, ch)
    key = noise_with_bursts(4, n, ch)
    x[7, 0], x[20, 1], x[33, 2], x[40, 0] = np.inf, np.nan, -0.0, -np.inf
    key[50, :], key[60, 1] = np.nan, np.inf
    c = dr.Curve(dr.design(-30.0, 3.0, 4.0, -45.0, 2.0, 20.0, 2.0), 0b101, A, H, 1 << 26)
    for k in (None, key):
        want, trace, E = dr.render(c, x, k)
        assert want.shape == (n, ch) and len(trace) == n
        for cuts, own_flush in (([n], True), ([0, 1, 0, max(A - 2, 0), 2, 0, 3], False), ([1] * 9 + [130], True), ([199, 0, 201], False)):
            st = dr.Stream(c, ch)
            if sum(cuts) != n:
                cuts = cuts + [n - sum(cuts)]
            out, tr, at = [], [], 0
            for i, f in enumerate(cuts):
                before = (st.n, st.e)
                last = i == len(cuts) - 1
                o, t, _e = st.push(x[at:at + f], None if k is None else k[at:at + f], flush=last and not own_flush)
                assert len(o) == dr.emitted(c.latency, before[0] + f, before[1], last and not own_flush) - before[1]
                out.append(o)
                tr.append(t)
                at += f
            if own_flush:
                o, t, _e = st.push(x[:0], None if k is None else k[:0], flush=True)
                out.append(o)
                tr.append(t)
            got = np.concatenate(out)
            nan = np.isnan(want)
            assert got.shape == want.shape and np.isnan(got[nan]).all()
            assert got.view(np.uint32)[~nan].tobytes() == want.view(np.uint32)[~nan].tobytes(), (A, H, cuts)
            assert np.concatenate(tr).tobytes() == trace.tobytes() and st.E_all == E.tolist() and st.e == st.n == n


def test_a_constant_level_settles_to_the_curves_value_exactly():
    """what the issue's prototype found: a 4:1 compressor at -20 dB settles a 0.5 DC input to exactly the curve's -10.4845 dB"""
    T = dr.design(-20.0, 4.0)
    c = dr.Curve(T, 1, 48, 480, 891723)
    x = np.full((3000, 1), 0.5, np.float32)
    out, tr, E = dr.render(c, x)
    Gt = int(dr.curve_at(T, dr.level(x[:1], 1))[0])
    assert Gt == int(dr.curve_at(T, -65536)) and (E[:2000] == Gt << 16).all()
    assert abs(float(tr[100]) - -10.4845) <= 5e-5 and tr[100] == np.float32(dr.gain_db(T, 20.0 * math.log10(0.5)))
    assert len(set(out[:2000, 0].tolist())) == 1 and abs(out[0, 0] / 0.5 - 10.0 ** (tr[100] / 20.0)) <= 1e-6
    # the silence behind a flushed programme is never reached: the window of A frames ends inside the programme for every r a frame sums
    assert (E == Gt << 16).all()


def test_a_curve_of_zeros_passes_the_bits_through():
    x = noise_with_bursts(1, 300, 2)
    x.view(np.uint32)[5, 0], x[6, 1], x[7, 0], x[8, 1] = 0x7FA12345, -0.0, np.inf, 1e-45
    c = dr.Curve(np.zeros(dr.POINTS, np.int64), 3, 33, 7, 12345)
    out, tr, E = dr.render(c, x)
    assert out.tobytes() == x.tobytes() and not E.any() and not tr.any()
    st = dr.Stream(c, 2)
    a = st.push(x[:100])[0]
    assert len(a) == 100 - 32 and a.tobytes() == x[:68].tobytes()      # a plain delayed copy


# ---------------------------------------------------------------- the header
C99_USE = r'''
#include <stddef.h>
#include "omx/program_dynamics.h"
typedef char curve_is_3096_bytes[sizeof(omx_program_dynamics_curve) == 3096 ? 1 : -1];
typedef char spec_is_56_bytes[sizeof(omx_program_dynamics_spec) == 56 ? 1 : -1];
typedef char point_is_16_bytes[sizeof(omx_program_dynamics_point) == 16 ? 1 : -1];
typedef char info_is_32_bytes[sizeof(omx_program_dynamics_info) == 32 ? 1 : -1];
typedef char record_is_104_bytes[sizeof(omx_program_dynamics_record) == 104 ? 1 : -1];
int main(void) {
    return (int)offsetof(omx_program_dynamics_curve, detector_mask) - 3076 + (int)offsetof(omx_program_dynamics_curve, attack_frames) - 3080
        + (int)offsetof(omx_program_dynamics_curve, hold_frames) - 3084 + (int)offsetof(omx_program_dynamics_curve, release_step) - 3088
        + (int)offsetof(omx_program_dynamics_spec, ratio) - 8 + (int)offsetof(omx_program_dynamics_spec, makeup_db) - 48
        + (int)offsetof(omx_program_dynamics_point, out_db) - 8
        + (int)offsetof(omx_program_dynamics_info, smooth_tile) - 16 + (int)offsetof(omx_program_dynamics_info, channels) - 24
        + (int)offsetof(omx_program_dynamics_record, frames_reduced) - 24 + (int)offsetof(omx_program_dynamics_record, samples_nonfinite) - 48
        + (int)offsetof(omx_program_dynamics_record, min_gain) - 56 + (int)offsetof(omx_program_dynamics_record, min_gain_db) - 72
        + (int)offsetof(omx_program_dynamics_record, out_sample_peak) - 80 + (int)offsetof(omx_program_dynamics_record, state) - 88
        + (int)offsetof(omx_program_dynamics_record, curve_index) - 96
        + (int)(OMX_DYNAMICS_CURVE_POINTS - 769u) + (int)(OMX_DYNAMICS_TABLE_ENTRIES - 257u) + (int)(OMX_DYNAMICS_MAX_CURVES - 64u)
        + (int)(OMX_DYNAMICS_MAX_POINTS - 16u) + (OMX_DYNAMICS_BYPASS == 0xFFFFFFFFu ? 0 : 1) + (OMX_DYNAMICS_L_MIN + 40 * 65536)
        + (OMX_DYNAMICS_L_MAX - 8 * 65536) + (OMX_DYNAMICS_MAX_GAIN - 40 * 65536) + (OMX_DYNAMICS_MAX_STEP == 40ll * 4294967296ll ? 0 : 1)
        + (int)(OMX_DYNAMICS_IDLE + OMX_DYNAMICS_RUNNING + OMX_DYNAMICS_FLUSHED - 3u);
}
'''


def test_header_is_c99_its_structures_have_their_sizes_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text(C99_USE)
    exe = tmp_path / "use"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    assert subprocess.run([str(exe)]).returncode == 0
    import openmeters_amd as oa
    header = open(os.path.join(INCLUDE, "program_dynamics.h")).read()
    assert '#include "program_convolve.h"' in header
    sizes = {"omx_program_dynamics_curve": (oa.CProgramDynamicsCurve, 3096), "omx_program_dynamics_spec": (oa.CProgramDynamicsSpec, 56),
             "omx_program_dynamics_point": (oa.CProgramDynamicsPoint, 16), "omx_program_dynamics_info": (oa.CProgramDynamicsInfo, 32),
             "omx_program_dynamics_record": (oa.CProgramDynamicsRecord, 104)}
    for name, (struct, size) in sizes.items():
        assert C.sizeof(struct) == size
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), (name, "the header's comment does not give this size")
    for dtype, struct in ((oa.DYNAMICS_RECORD_DTYPE, oa.CProgramDynamicsRecord), (oa.DYNAMICS_INFO_DTYPE, oa.CProgramDynamicsInfo)):
        assert dtype.itemsize == C.sizeof(struct)
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [getattr(oa.CProgramDynamicsRecord, f).offset for f in oa.DYNAMICS_RECORD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80,
                                                                                                      84, 88, 92, 96, 100]
    assert oa.CProgramDynamicsCurve.release_step.offset == 3088
    syms = declared(os.path.join(INCLUDE, "program_dynamics.h"))
    assert syms == ["omx_program_dynamics_check", "omx_program_dynamics_design", "omx_program_dynamics_frames", "omx_program_dynamics_from_points",
                    "omx_program_dynamics_gain_db", "omx_program_dynamics_latency", "omx_program_dynamics_plan", "omx_program_dynamics_tables",
                    "omx_program_dynamics_time", "omx_program_loudness_bank_dynamics", "omx_program_loudness_bank_dynamics_configure",
                    "omx_program_loudness_bank_dynamics_reset", "omx_program_loudness_bank_fetch_dynamics"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_dynamics.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h or in an earlier header
    assert "program_dynamics" not in open(os.path.join(ROOT, "include", "omx.h")).read()
    assert "dynamics" not in open(os.path.join(INCLUDE, "program_convolve.h")).read()
    for name in ("DynamicsSpec", "DynamicsCurve", "DYNAMICS_RECORD_DTYPE", "DYNAMICS_INFO_DTYPE", "dynamics_plan", "dynamics_design",
                 "dynamics_from_points", "dynamics_check", "dynamics_gain_db", "dynamics_time", "dynamics_frames", "dynamics_latency",
                 "dynamics_tables", "DYNAMICS_BYPASS"):
        assert hasattr(oa, name), name
    assert (oa.DYNAMICS_L_MIN, oa.DYNAMICS_L_MAX, oa.DYNAMICS_MAX_GAIN, oa.DYNAMICS_MAX_STEP, oa.DYNAMICS_BYPASS, oa.DYNAMICS_CURVE_POINTS) == (
        dr.L_MIN, dr.L_MAX, dr.MAX_GAIN, dr.MAX_STEP, dr.BYPASS, dr.POINTS)
    assert oa.DYNAMICS_OCTAVE_DB == dr.OCTAVE_DB == 20.0 * math.log10(2.0)
    assert (oa.DYNAMICS_IDLE, oa.DYNAMICS_RUNNING, oa.DYNAMICS_FLUSHED) == (0, 1, 2)
    for name in ("configure_dynamics", "dynamics", "reset_dynamics", "fetch_dynamics"):
        assert hasattr(oa.ProgramLoudnessBank, name), name


def build_demo(tmp_path):
    """tests/c_abi/program_dynamics_demo.c: a plain C99 host that designs a compressor and settles a DC input"""
    out = str(tmp_path / "program_dynamics_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_dynamics_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


def test_check_program_is_clean_under_the_sanitizers(tmp_path):
    """tools/dynamics_design_check.cpp, a stand-alone host program with its own main, under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "dynamics_design_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "dynamics_design_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


# ---------------------------------------------------------------- plan, frames, latency, time
def test_plan_frames_latency_and_time(omx):
    import openmeters_amd as oa
    plan = omx.fn("program_dynamics_plan", C.c_int, [C.c_uint32, C.c_void_p])
    for ch in range(1, 9):
        info = oa.dynamics_plan(omx, ch)
        assert int(info["channels"]) == ch and all(int(info[k]) >= 256 and int(info[k]) % 64 == 0 for k in info.dtype.names[:6])
        assert int(info["hold_max_window"]) < dr.MAX_GAIN and oa.DYNAMICS_MAX_ATTACK + oa.DYNAMICS_MAX_HOLD > int(info["hold_max_window"])
    for ch in (0, 9, 2 ** 32 - 1):
        buf = np.full((32,), 0xAB, np.uint8)
        assert plan(ch, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all()
        assert last_error(omx).startswith("program loudness dynamics plan: ")
    assert plan(2, None) == capi.ERR_INVALID
    for latency in (0, 1, 63, 4095):
        n = e = 0
        for f, flush in ((0, False), (1, False), (5, False), (latency, False), (5000, False), (0, False), (2, True), (0, True)):
            got = oa.dynamics_frames(omx, latency, n, e, f, flush)
            assert got == dr.emitted(latency, n + f, e, flush) - e, (latency, n, e, f, flush)
            n, e = n + f, e + got
        assert e == n
    fn = omx.fn("program_dynamics_frames", C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])
    out = np.full((1,), 0xABABABABABABABAB, np.uint64)
    for args in ((4096, 0, 0, 1, 0), (1, 2 ** 63 + 1, 0, 0, 0), (1, 2 ** 62, 0, 2 ** 63, 0), (1, 5, 6, 1, 0)):
        assert fn(*args, out.ctypes.data) == capi.ERR_INVALID and out[0] == 0xABABABABABABABAB, args
        assert last_error(omx).startswith("program loudness dynamics frames: ")
    assert fn(1, 0, 0, 1, 0, None) == capi.ERR_INVALID
    # time
    for fs, a, h, rate in ((48000.0, 1.0, 10.0, 60.0), (44100.0, 0.0, 0.0, math.inf), (96000.0, 42.6, 170.6, 3.0), (8000.0, 5.0, 0.06, 1e-9),
                           (48000.0, 0.01, 341.33, 1e9)):
        assert oa.dynamics_time(omx, fs, a, h, rate) == dr.time(fs, a, h, rate), (fs, a, h, rate)
    assert oa.dynamics_time(omx, 48000.0, 1.0, 10.0, 60.0) == (48, 480, 891723)
    assert oa.dynamics_time(omx, 44100.0, 0.0, 0.0, math.inf) == (1, 0, dr.MAX_STEP) and oa.dynamics_time(omx, 8000.0, 5.0, 0.06, 1e-9)[2] == 1
    time = omx.fn("program_dynamics_time", C.c_int, [C.c_double] * 4 + [C.c_void_p] * 3)
    res = np.full((4,), 0xABABABAB, np.uint32)
    for args in ((0.0, 1, 1, 1), (math.nan, 1, 1, 1), (math.inf, 1, 1, 1), (48000, -1, 1, 1), (48000, math.nan, 1, 1), (48000, 1, -1, 1),
                 (48000, 1, math.inf, 1), (48000, 85.4, 1, 1), (48000, 1, 341.4, 1), (48000, 1, 1, 0), (48000, 1, 1, -3), (48000, 1, 1, math.nan)):
        assert time(*args, res.ctypes.data, res.ctypes.data + 4, res.ctypes.data + 8) == capi.ERR_INVALID and (res == 0xABABABAB).all(), args
        assert last_error(omx).startswith("program loudness dynamics time: ")
    assert time(48000.0, 1.0, 1.0, 1.0, None, None, None) == 0      # any result pointer may be null
    # latency
    T = np.zeros(dr.POINTS, np.int32)
    assert [oa.dynamics_latency(omx, oa.DynamicsCurve(T, 1, a, 0, 1)) for a in (1, 2, 4096)] == [0, 1, 4095]


# ---------------------------------------------------------------- check, design, points, gain
def test_check_takes_what_the_bank_takes_and_refuses_the_rest(omx):
    import openmeters_amd as oa
    check = omx.fn("program_dynamics_check", C.c_int, [C.c_void_p])
    latency = omx.fn("program_dynamics_latency", C.c_int, [C.c_void_p, C.c_void_p])
    T = np.zeros(dr.POINTS, np.int32)
    T[0], T[768], T[300] = dr.MAX_GAIN, -dr.MAX_GAIN, 12345
    assert oa.dynamics_check(omx, oa.DynamicsCurve(T, 1, 1, 0, 1)) == 0
    assert oa.dynamics_check(omx, oa.DynamicsCurve(T, 255, 4096, 16384, dr.MAX_STEP)) == 0
    over, under = T.copy(), T.copy()
    over[768], under[0] = dr.MAX_GAIN + 1, -dr.MAX_GAIN - 1
    out = np.full((1,), 0xABABABAB, np.uint32)
    for bad in (oa.DynamicsCurve(over), oa.DynamicsCurve(under), oa.DynamicsCurve(T, 0), oa.DynamicsCurve(T, 256), oa.DynamicsCurve(T, 1, 0),
                oa.DynamicsCurve(T, 1, 4097), oa.DynamicsCurve(T, 1, 1, 16385), oa.DynamicsCurve(T, 1, 1, 0, 0), oa.DynamicsCurve(T, 1, 1, 0, -5),
                oa.DynamicsCurve(T, 1, 1, 0, dr.MAX_STEP + 1)):
        c = bad.to_c()
        assert check(C.byref(c)) == capi.ERR_INVALID
        assert last_error(omx).startswith("program loudness dynamics check: ")
        assert latency(C.byref(c), out.ctypes.data) == capi.ERR_INVALID and out[0] == 0xABABABAB
        assert last_error(omx).startswith("program loudness dynamics latency: ")
    assert check(None) == capi.ERR_INVALID and latency(None, out.ctypes.data) == capi.ERR_INVALID
    assert latency(C.byref(oa.DynamicsCurve(T).to_c()), None) == capi.ERR_INVALID


def test_design_and_points_against_the_restatement(omx):
    """the module's docstring gives the bar and what was measured"""
    import openmeters_amd as oa
    worst = 0
    for spec in SPECS:
        T = oa.dynamics_design(omx, oa.DynamicsSpec(*spec))
        want = dr.design(*spec)
        assert T.dtype == np.int32 and T.shape == (dr.POINTS,) and np.abs(T).max() <= dr.MAX_GAIN
        diff = int(np.abs(T.astype(np.int64) - want).max())
        print(f"dynamics design {spec}: max |library - restatement| = {diff} units of 2^-16 octave")
        worst = max(worst, diff)
        assert diff <= 1, spec
        assert oa.dynamics_check(omx, oa.DynamicsCurve(T)) == 0
    for pts in POINT_SETS:
        T = oa.dynamics_from_points(omx, pts)
        diff = int(np.abs(T.astype(np.int64) - dr.from_points(pts)).max())
        print(f"dynamics points {len(pts)}: max |library - restatement| = {diff} units")
        worst = max(worst, diff)
        assert diff <= 1, pts
    print(f"dynamics design and points: the largest difference is {worst} units")
    # shapes by hand: 4:1 at -20 dB gives -15 dB at 0 dB and nothing below the threshold; sox-style points keep slope 1 outside
    T = oa.dynamics_design(omx, oa.DynamicsSpec(-20.0, 4.0))
    assert abs(oa.dynamics_gain_db(omx, T, 0.0) - -15.0) <= 1e-4 and oa.dynamics_gain_db(omx, T, -20.5) == 0.0
    T = oa.dynamics_design(omx, oa.DynamicsSpec(-20.0, 4.0, 10.0))
    # the middle of the knee: (1/R - 1) (K/2)^2 / (2K).  The table is linear between entries h = 0.376 dB apart; on the quadratic, whose
    # second derivative is (1/R - 1) / K = 0.075 per dB^2, that is off by at most h^2 / 8 * 0.075 = 1.4e-3 dB
    assert abs(oa.dynamics_gain_db(omx, T, -20.0) - -0.75 * 25.0 / 20.0) <= 1.4e-3 + 1e-4
    T = oa.dynamics_design(omx, oa.DynamicsSpec(0.0, 1.0, 0.0, -40.0, 2.0, 12.0, 0.0))
    assert abs(oa.dynamics_gain_db(omx, T, -45.0) - -5.0) <= 1e-4 and abs(oa.dynamics_gain_db(omx, T, -80.0) - -12.0) <= 1e-4
    T = oa.dynamics_from_points(omx, POINT_SETS[0])
    for level, gain in ((-100.0, -20.0), (-55.0, -10.0), (-30.0, 0.0), (-10.0, -5.0), (20.0, -10.0)):
        assert abs(oa.dynamics_gain_db(omx, T, level) - gain) <= 1e-4, (level, gain)


def test_gain_db_matches_the_restatement_exactly(omx):
    import openmeters_amd as oa
    rng = np.random.default_rng(5)
    T = oa.dynamics_design(omx, oa.DynamicsSpec(*SPECS[1]))
    levels = [-math.inf, -1000.0, -240.83, -240.8239965311849, -100.3, -20.0, -6.02, 0.0, 3.0, 48.16, 48.2, 1000.0, math.inf] + list(rng.uniform(-250, 50, 500))
    for level in levels:
        assert oa.dynamics_gain_db(omx, T, level) == dr.gain_db(T, level), level
    rnd = rng.integers(-dr.MAX_GAIN, dr.MAX_GAIN + 1, dr.POINTS).astype(np.int32)
    for level in rng.uniform(-245, 50, 500):
        assert oa.dynamics_gain_db(omx, rnd, level) == dr.gain_db(rnd, level), level
    fn = omx.fn("program_dynamics_gain_db", C.c_int, [C.c_void_p, C.c_double, C.c_void_p])
    out = np.full((1,), 777.25, np.float64)
    c = oa.DynamicsCurve(rnd).to_c()
    assert fn(C.byref(c), math.nan, out.ctypes.data) == capi.ERR_INVALID and out[0] == 777.25
    assert last_error(omx).startswith("program loudness dynamics gain: ")
    rnd[700] = dr.MAX_GAIN + 1
    c = oa.DynamicsCurve(rnd).to_c()
    assert fn(C.byref(c), 0.0, out.ctypes.data) == capi.ERR_INVALID and out[0] == 777.25
    assert fn(None, 0.0, out.ctypes.data) == capi.ERR_INVALID and fn(C.byref(c), 0.0, None) == capi.ERR_INVALID


def test_design_and_points_refuse_and_write_nothing(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_dynamics_design", C.c_int, [C.c_void_p, C.c_void_p])
    good = dict(threshold_db=-20.0, ratio=4.0, knee_db=6.0, expander_threshold_db=-60.0, expander_ratio=2.0, range_db=24.0, makeup_db=0.0)
    bad = [dict(threshold_db=math.nan), dict(threshold_db=48.5), dict(threshold_db=-241.0), dict(ratio=0.99), dict(ratio=math.nan),
           dict(knee_db=-0.1), dict(knee_db=math.inf), dict(expander_ratio=0.5), dict(expander_ratio=math.inf), dict(expander_ratio=math.nan),
           dict(expander_threshold_db=math.nan), dict(expander_threshold_db=49.0), dict(range_db=-1.0), dict(range_db=math.nan),
           dict(makeup_db=math.inf), dict(makeup_db=math.nan)]
    for change in bad:
        spec = oa.DynamicsSpec(**{**good, **change}).to_c()
        buf = np.full((3096,), 0xAB, np.uint8)
        assert fn(C.byref(spec), buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), change
        assert last_error(omx).startswith("program loudness dynamics design: "), change
    spec = oa.DynamicsSpec(**good).to_c()
    assert fn(None, np.zeros(3096, np.uint8).ctypes.data) == capi.ERR_INVALID and fn(C.byref(spec), None) == capi.ERR_INVALID
    # the design writes the table and nothing else of the curve
    buf = np.full((3096,), 0xAB, np.uint8)
    assert fn(C.byref(spec), buf.ctypes.data) == 0 and (buf[3076:] == 0xAB).all() and not (buf[:3076] == 0xAB).all()
    # an expander threshold is not looked at without an expander
    assert oa.dynamics_design(omx, oa.DynamicsSpec(-20.0, 4.0, 0.0, math.nan, 1.0)).shape == (dr.POINTS,)
    pts = omx.fn("program_dynamics_from_points", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p])
    two = (oa.CProgramDynamicsPoint * 17)(*[oa.CProgramDynamicsPoint(-90.0 + 5 * i, -90.0 + 4 * i) for i in range(17)])
    for n in (0, 17, 2 ** 32 - 1):
        buf = np.full((3096,), 0xAB, np.uint8)
        assert pts(two, n, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), n
        assert last_error(omx).startswith("program loudness dynamics points: ")
    for i, v in ((1, (-90.0, 0.0)), (1, (-95.0, 0.0)), (0, (math.nan, 0.0)), (1, (-80.0, math.inf))):
        arr = (oa.CProgramDynamicsPoint * 2)(oa.CProgramDynamicsPoint(-90.0, -90.0), oa.CProgramDynamicsPoint(-20.0, -30.0))
        arr[i] = oa.CProgramDynamicsPoint(*v)
        buf = np.full((3096,), 0xAB, np.uint8)
        assert pts(arr, 2, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), (i, v)
    assert pts(None, 2, buf.ctypes.data) == capi.ERR_INVALID and pts(two, 2, None) == capi.ERR_INVALID


def test_bank_calls_with_null_handles_are_refused(omx):
    """what needs no device: a null bank is refused by every bank function of the header"""
    rec = np.zeros((104,), np.uint8)
    assert omx.fn("program_loudness_bank_dynamics_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])(
        None, 2, None, 1, None) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_dynamics_reset", C.c_int, [C.c_void_p, C.c_void_p])(None, None) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_fetch_dynamics", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(None, 0, rec.ctypes.data) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_dynamics", C.c_int, [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3)(
        None, None, None, 0, None, None, None, 0, None, None, None) == capi.ERR_INVALID

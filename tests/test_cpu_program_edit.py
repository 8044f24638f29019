"""Programme bank edit pass (include/omx/program_edit.h), CPU side: the numpy restatement (tests/program_edit_ref.py) pinned by a
hand-written case; the library's gain function against the restatement on bits; the curve tables; the header as C99, its structures'
sizes and offsets, the exported functions, the Python surface; extent and trim against the restatement, and every refusal of the
host-only functions with the output buffers still holding their sentinels.

Bars.  Everything is equal on bits but two things: the curve tables lie within 1 ulp of numpy's double-precision curve rounded to f32
(the host's libm against numpy's on the same doubles), and out_sample_peak_db lies within the family's 1e-4 dB."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_edit_ref as er
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
Q = 2.0 ** -24


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def last_error(omx):
    return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")


# ---------------------------------------------------------------- the restatement, by hand
def test_restatement_gives_the_hand_written_output_of_two_clips():
    """An 8-frame stereo source.  Clip A: source frames 1 .. 6 at output frame 2, gain 0.5, linear fade-in of 2.  Clip B: source frames
    0 .. 3 at output frame 6, gain 1, linear fade-out of 3.  Output frames 0 1 are pads, 2 3 A's fade-in (0.5 * 1/4 and 0.5 * 3/4),
    4 5 A at 0.5, 6 A at 0.5 plus B copied, 7 A at 0.5 plus B under the fade-out's third step from the end, 8 9 B alone.  The phase of a
    fade of 3: M = (2^63 - 2) / 3, p = 2796202, 8388607, 13981013 for i = 0, 1, 2 (one below 2^24 / 6, 2^24 / 2 and 5 * 2^24 / 6
    rounded down), and a linear table gives g = p / 2^24 exactly.  Every sample is a power of two or a small dyadic number, so every
    product and sum below is exact in f32."""
    src = np.array([(1.0, -1.0), (1.0, 1.0), (0.5, 0.25), (-0.25, 2.0), (0.75, -0.0), (0.25, 0.5), (0.25, -1.5), (9.0, 9.0)], np.float32)
    a = er.Clip(src_first=1, dst_first=2, frames=6, gain=0.5, fade_in_frames=2)
    b = er.Clip(src_first=0, dst_first=6, frames=4, gain=1.0, fade_out_frames=3)
    assert [int(v) for v in er.phase(3, [0, 1, 2])] == [2796202, 8388607, 13981013]
    assert [int(v) for v in er.phase(2, [0, 1])] == [1 << 22, 3 << 22]
    g0, g1, g2 = 2796202 * Q, 8388607 * Q, 13981013 * Q
    want = np.array([(0.0, 0.0), (0.0, 0.0), (0.125, 0.125), (0.1875, 0.09375), (-0.125, 1.0), (0.375, -0.0), (1.125, -0.75),
                     (0.125 + g2, -0.75 + g2), (0.5 * g1, 0.25 * g1), (-0.25 * g0, 2.0 * g0)], np.float64)
    assert (want.astype(np.float32).astype(np.float64) == want).all(), "the hand-written figures are not f32 values"
    (y,), (rec,) = er.render([src], [a, b], [10], 2, er.analytic_tables())
    assert y.tobytes() == want.astype(np.float32).tobytes(), (y, want)
    assert np.signbit(y[5, 1]) and not np.signbit(y[:2]).any()      # -0.0 * 0.5 is -0.0; the pads are +0.0
    fields = {"out_first": 0, "frames": 10, "silent_frames": 2, "faded_frames": 5, "mixed_frames": 2, "samples_over": 1, "clips": 2, "_pad": 0}
    assert {f: int(rec[f]) for f in fields} == fields
    assert float(rec["out_sample_peak"]) == 1.125 and abs(float(rec["out_sample_peak_db"]) - 20 * np.log10(1.125)) <= 1e-4
    # the same frames through windows: pieces of the whole, counts that add up
    parts = [er.render([src], [a, b], [n], 2, er.analytic_tables(), out_first=[f]) for f, n in ((0, 3), (3, 4), (7, 3))]
    assert b"".join(p[0][0].tobytes() for p in parts) == y.tobytes()
    for f in er.COUNT_FIELDS:
        assert sum(int(p[1][0][f]) for p in parts) == int(rec[f]), f
    assert [int(p[1][0]["clips"]) for p in parts] == [1, 2, 2] and max(float(p[1][0]["out_sample_peak"]) for p in parts) == 1.125
    # B alone, gain 1: frame 6 is its source's bits
    (yb,), _ = er.render([src], [b], [10], 2, er.analytic_tables())
    assert yb[6].tobytes() == src[0].tobytes() and not yb[:6].any()


def test_restatement_copies_hard_values_and_sums_in_table_order():
    x = np.array([[np.nan], [np.inf], [-np.inf], [-0.0], [1e-45], [3.0]], np.float32)
    x.view(np.uint32)[0] = 0x7FA00001      # a signalling NaN with a payload
    tabs = er.analytic_tables()
    (y,), (rec,) = er.render([x], [er.Clip(frames=6, dst_first=1)], [8], 1, tabs)
    assert y[1:7].tobytes() == x.tobytes() and y[0].tobytes() == y[7].tobytes() == np.float32(0).tobytes()
    assert int(rec["samples_over"]) == 3 and np.isinf(rec["out_sample_peak"]) and int(rec["silent_frames"]) == 2
    (y,), _ = er.render([x], [er.Clip(frames=1, src_first=3), er.Clip(frames=1, src_first=3, gain=0.5)], [1], 1, tabs)
    assert y.tobytes() == np.float32(-0.0).tobytes()      # the copied -0.0 plus 0.5 * -0.0
    with pytest.raises(er.Invalid):
        er.render([x], [er.Clip(frames=2), er.Clip(frames=2), er.Clip(frames=2, dst_first=1)], [3], 1, tabs)


# ---------------------------------------------------------------- gain and curves
@pytest.mark.parametrize("curve", er.CURVES)
def test_gain_function_equals_the_restatement_on_bits(omx, curve):
    import openmeters_amd as oa
    tab = oa.edit_curve(omx, curve)
    fn = omx.fn("program_edit_gain", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
    out = C.c_float()
    rng = np.random.default_rng(11 + curve)
    cases = [(f, np.arange(f)) for f in (1, 2, 3, 5, 63, 64, 65, 1000)]
    cases += [(f, np.unique(np.concatenate([[0, f - 1], rng.integers(0, f, 10000)]))) for f in (48000, 2 ** 24 - 1, 2 ** 24)]
    for f, idx in cases:
        want = er.gain(tab, f, idx)
        got = np.zeros(len(idx), np.float32)
        for n, i in enumerate(idx):
            assert fn(curve, f, int(i), C.byref(out)) == 0
            got[n] = out.value
        assert got.tobytes() == want.tobytes(), (curve, f, np.flatnonzero(got != want)[:5])
        # monotone and inside [0, 1].  0 itself only where (i + 1/2) / F lies below 2^-24, that is beyond F = 2^23; 1 itself only where
        # the curve is flat to f32 (the last steps of a long equal-power or raised-cosine fade), never on the linear curve
        assert (got >= 0).all() and (got <= 1).all() and (np.diff(got) >= 0).all(), (curve, f)
        assert (f > 2 ** 23 or (got > 0).all()) and (curve != er.CURVE_LINEAR or (got < 1).all()), (curve, f)
        p = er.phase(f, idx)
        assert int(p.max()) < 2 ** 24 and (np.abs(p.astype(np.float64) * Q - (idx + 0.5) / f) <= Q).all(), f
    assert float(oa.edit_gain(omx, curve, 3, 1)) == float(er.gain(tab, 3, [1])[0])
    # at F = 777 the function lies within 1.4e-7 of the analytic curve
    i = np.arange(777)
    x = (i + 0.5) / 777
    exact = x if curve == er.CURVE_LINEAR else (np.sin(np.pi / 2 * x) if curve == er.CURVE_EQUAL_POWER else 0.5 - 0.5 * np.cos(np.pi * x))
    assert np.abs(er.gain(tab, 777, i).astype(np.float64) - exact).max() <= 1.4e-7
    for args in ((3, 1, 0), (curve, 0, 0), (curve, 2 ** 24 + 1, 0), (curve, 5, 5)):
        out.value = 7.0
        assert fn(*args, C.byref(out)) == capi.ERR_INVALID and out.value == 7.0, args
    assert fn(curve, 5, 0, None) == capi.ERR_INVALID


@pytest.mark.parametrize("curve", er.CURVES)
def test_curve_tables(omx, curve):
    import openmeters_amd as oa
    tab = oa.edit_curve(omx, curve)
    assert tab.dtype == np.float32 and tab.shape == (4097,)
    assert tab[0].tobytes() == np.float32(0).tobytes() and tab[4096].tobytes() == np.float32(1).tobytes()
    assert (np.diff(tab) >= 0).all() and (np.diff(tab[::64]) > 0).all()
    want = er.analytic_curve(curve).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -126)))
    assert (np.abs(tab.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    if curve == er.CURVE_LINEAR:
        assert tab.tobytes() == want.tobytes()
    fn = omx.fn("program_edit_curve", C.c_int, [C.c_uint32, C.c_void_p])
    buf = np.full((4097,), 7.0, np.float32)
    assert fn(3, buf.ctypes.data) == capi.ERR_INVALID and (buf == 7.0).all()
    assert fn(curve, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- the header
C99_USE = r'''
#include <stddef.h>
#include "omx/program_edit.h"
typedef char clip_is_48_bytes[sizeof(omx_program_edit_clip) == 48 ? 1 : -1];
typedef char info_is_16_bytes[sizeof(omx_program_edit_info) == 16 ? 1 : -1];
typedef char rule_is_48_bytes[sizeof(omx_program_trim_rule) == 48 ? 1 : -1];
typedef char record_is_64_bytes[sizeof(omx_program_edit_record) == 64 ? 1 : -1];
int main(void) {
    return (int)offsetof(omx_program_edit_clip, src_first) - 8 + (int)offsetof(omx_program_edit_clip, frames) - 24
        + (int)offsetof(omx_program_edit_clip, fade_out_frames) - 36 + (int)offsetof(omx_program_edit_clip, fade_in_curve) - 40
        + (int)offsetof(omx_program_edit_clip, flags) - 42 + (int)offsetof(omx_program_edit_clip, gain) - 44
        + (int)offsetof(omx_program_trim_rule, fade_in_frames) - 32 + (int)offsetof(omx_program_trim_rule, flags) - 42
        + (int)offsetof(omx_program_edit_record, samples_over) - 40 + (int)offsetof(omx_program_edit_record, out_sample_peak) - 48
        + (int)offsetof(omx_program_edit_record, clips) - 56
        + (int)(OMX_EDIT_CURVE_RAISED_COSINE - 2u) + (int)(OMX_EDIT_CURVE_POINTS - 4097u) + (OMX_EDIT_MAX_POSITION == (1ull << 40) ? 0 : 1);
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
    header = open(os.path.join(INCLUDE, "program_edit.h")).read()
    sizes = {"omx_program_edit_clip": (oa.CProgramEditClip, 48), "omx_program_edit_info": (oa.CProgramEditInfo, 16),
             "omx_program_trim_rule": (oa.CProgramTrimRule, 48), "omx_program_edit_record": (oa.CProgramEditRecord, 64)}
    for name, (struct, size) in sizes.items():
        assert C.sizeof(struct) == size
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), (name, "the header's comment does not give this size")
    assert oa.EDIT_RECORD_DTYPE == er.RECORD_DTYPE
    for dtype, struct in ((oa.EDIT_RECORD_DTYPE, oa.CProgramEditRecord), (oa.EDIT_CLIP_DTYPE, oa.CProgramEditClip),
                          (oa.EDIT_INFO_DTYPE, oa.CProgramEditInfo)):
        assert dtype.itemsize == C.sizeof(struct)
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [getattr(oa.CProgramEditClip, f).offset for f in oa.EDIT_CLIP_DTYPE.names] == [0, 4, 8, 16, 24, 32, 36, 40, 41, 42, 44]
    assert [getattr(oa.CProgramEditRecord, f).offset for f in er.RECORD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert [f for f, _ in oa.CProgramTrimRule._fields_][:9] == list(er.Trim.__dataclass_fields__)
    assert [getattr(oa.CProgramTrimRule, f).offset for f, _ in oa.CProgramTrimRule._fields_] == [0, 8, 16, 24, 32, 36, 40, 41, 42, 44]
    syms = declared(os.path.join(INCLUDE, "program_edit.h"))
    assert syms == ["omx_program_edit_curve", "omx_program_edit_extent", "omx_program_edit_gain", "omx_program_edit_plan",
                    "omx_program_edit_trim", "omx_program_loudness_bank_edit", "omx_program_loudness_bank_edit_configure",
                    "omx_program_loudness_bank_fetch_edited"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_edit.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_edit" not in open(os.path.join(ROOT, "include", "omx.h")).read()
    for name in ("EditClip", "TrimRule", "EDIT_RECORD_DTYPE", "EDIT_CURVE_LINEAR", "EDIT_CURVE_EQUAL_POWER", "EDIT_CURVE_RAISED_COSINE",
                 "edit_plan", "edit_curve", "edit_gain", "edit_extent", "edit_trim"):
        assert hasattr(oa, name), name
    assert (oa.EDIT_CURVE_LINEAR, oa.EDIT_CURVE_EQUAL_POWER, oa.EDIT_CURVE_RAISED_COSINE) == er.CURVES
    for name in ("configure_edit", "edit", "fetch_edited"):
        assert hasattr(oa.ProgramLoudnessBank, name), name


def build_demo(tmp_path):
    """tests/c_abi/program_edit_demo.c: a plain C99 host that inspects two tracks, trims both where the silence lies and joins them
    with a crossfade"""
    out = str(tmp_path / "program_edit_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_edit_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


def test_plan(omx):
    import openmeters_amd as oa
    plan = omx.fn("program_edit_plan", C.c_int, [C.c_uint32, C.c_void_p])
    for ch in range(1, 9):
        info = oa.edit_plan(omx, ch)
        t = int(info["tile_frames"])
        assert int(info["channels"]) == ch and t >= 64 and t % 64 == 0 and not info["_pad"].any()
    for ch in (0, 9, 2 ** 32 - 1):
        buf = np.full((16,), 0xAB, np.uint8)
        assert plan(ch, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), ch
    assert plan(2, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- extent
def to_api(clips):
    import openmeters_amd as oa
    return [oa.EditClip(**c.__dict__) for c in clips]


def test_extent_equals_the_restatement(omx):
    import openmeters_amd as oa
    rng = np.random.default_rng(21)
    for trial in range(200):
        n_in, n_out = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        frames_in = [int(v) for v in rng.integers(0, 60, n_in)]
        clips = []
        for o in range(n_out):
            at, mine = 0, []
            for _ in range(int(rng.integers(0, 5))):
                s = int(rng.integers(0, n_in))
                n = int(rng.integers(0, frames_in[s] + 1))
                at = max(0, at + int(rng.integers(-6, 10)))
                mine.append(er.Clip(s, o, int(rng.integers(0, frames_in[s] - n + 1)), at, n, int(rng.integers(0, n + 1)),
                                    int(rng.integers(0, n + 1)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), 0, 0.5))
            if trial % 7:      # (every seventh table keeps its disorder)
                mine.sort(key=lambda c: c.dst_first)
            clips += mine
        try:
            want = er.extent(clips, frames_in, n_out)
        except er.Invalid:
            want = None
        if want is None:
            with pytest.raises(capi.OmxError) as err:
                oa.edit_extent(omx, to_api(clips), frames_in, n_out)
            assert err.value.status == capi.ERR_INVALID
        else:
            assert [int(v) for v in oa.edit_extent(omx, to_api(clips), frames_in, n_out)] == want, (trial, clips)
    # zero frames: a clip of none, a table of none, a zero-frame clip between two that would otherwise be a triple
    assert list(oa.edit_extent(omx, [oa.EditClip(frames=0, dst_first=5)], [0], 2)) == [0, 0]
    assert list(oa.edit_extent(omx, [], [3], 1)) == [0]
    table = [er.Clip(frames=4), er.Clip(frames=0, dst_first=1), er.Clip(frames=4, dst_first=2), er.Clip(frames=3, dst_first=4)]
    assert list(oa.edit_extent(omx, to_api(table), [4], 1)) == er.extent(table, [4], 1) == [7]
    assert list(oa.edit_extent(omx, [oa.EditClip(frames=2 ** 32 - 1, dst_first=2 ** 40 - 2 ** 32 + 1)], [2 ** 32 - 1], 1)) == [2 ** 40]


def test_extent_refuses_bad_tables_and_writes_nothing(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_edit_extent", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
    frames_in = np.array([100, 50], np.uint32)
    good = [er.Clip(0, 0, 0, 0, 40, 10, 10), er.Clip(1, 0, 0, 30, 50, 10, 0), er.Clip(0, 1, 60, 5, 40)]
    assert list(oa.edit_extent(omx, to_api(good), frames_in, 2)) == er.extent(good, list(frames_in), 2) == [80, 45]

    def refused(clips, tag, n_in=2, n_out=2):
        table = oa.edit_table(to_api(clips))
        out = np.full((max(n_out, 1),), 0xABABABABABABABAB, np.uint64)
        assert fn(table.ctypes.data, table.size, n_in, frames_in.ctypes.data, n_out, out.ctypes.data) == capi.ERR_INVALID, tag
        assert (out == 0xABABABABABABABAB).all(), (tag, "out_frames was written")
        assert last_error(omx).startswith("program loudness edit extent: "), (tag, last_error(omx))
        with pytest.raises(er.Invalid):
            er.extent(clips, list(frames_in[:n_in]), n_out)

    def with_(k, **kw):
        clips = [er.Clip(**c.__dict__) for c in good]
        for f, v in kw.items():
            setattr(clips[k], f, v)
        return clips

    refused([good[1], good[0], good[2]], "unsorted by dst_first")
    refused([good[2], good[0], good[1]], "unsorted by dst_stream")
    refused(good[:2] + [er.Clip(0, 0, 0, 35, 10), good[2]], "triple overlap")
    refused(with_(0, src_first=61), "a clip beyond frames_in")
    refused(with_(1, frames=51, fade_in_frames=0), "a clip longer than frames_in")
    refused(with_(0, fade_in_curve=3), "bad fade-in curve")
    refused(with_(0, fade_out_curve=255), "bad fade-out curve")
    refused(with_(2, flags=1), "non-zero flags")
    refused(with_(1, gain=float("nan")), "NaN gain")
    refused(with_(1, gain=float("inf")), "infinite gain")
    refused(with_(0, fade_in_frames=41), "fade-in longer than the clip")
    refused(with_(0, fade_out_frames=41), "fade-out longer than the clip")
    refused(with_(0, src_stream=2), "src_stream out of range")
    refused(with_(2, dst_stream=2), "dst_stream out of range")
    refused(with_(2, dst_first=2 ** 40 - 39), "dst_first + frames beyond 2^40")
    # a fade longer than 2^24 (inside a clip that is long enough: the input stream would have to hold it)
    big_in = np.array([2 ** 25], np.uint32)
    table = oa.edit_table([oa.EditClip(frames=2 ** 25, fade_in_frames=2 ** 24 + 1)])
    out = np.full((1,), 7, np.uint64)
    assert fn(table.ctypes.data, 1, 1, big_in.ctypes.data, 1, out.ctypes.data) == capi.ERR_INVALID and out[0] == 7
    table["fade_in_frames"] = 2 ** 24
    assert fn(table.ctypes.data, 1, 1, big_in.ctypes.data, 1, out.ctypes.data) == 0 and out[0] == 2 ** 25
    # null pointers
    table = oa.edit_table(to_api(good))
    out = np.full((2,), 7, np.uint64)
    assert fn(None, 3, 2, frames_in.ctypes.data, 2, out.ctypes.data) == capi.ERR_INVALID
    assert fn(table.ctypes.data, 3, 2, None, 2, out.ctypes.data) == capi.ERR_INVALID
    assert fn(table.ctypes.data, 3, 2, frames_in.ctypes.data, 2, None) == capi.ERR_INVALID
    assert (out == 7).all()


# ---------------------------------------------------------------- trim
def inspect_record(frames, lead, trail):
    import openmeters_amd as oa
    rec = np.zeros((), oa.INSPECT_RECORD_DTYPE)
    rec["frames"], rec["leading_silence"], rec["trailing_silence"], rec["channels"] = frames, lead, trail, 2
    return rec


def test_trim_equals_the_restatement(omx):
    import openmeters_amd as oa
    cases = {"plain": ((1000, 100, 50), er.Trim()),
             "silent end to end": ((480, 480, 480), er.Trim(pad_head=24000, pad_tail=96000, fade_in_frames=10, keep_head=5)),
             "no frames": ((0, 0, 0), er.Trim(pad_head=3, pad_tail=4, fade_out_frames=9)),
             "keep larger than the silence found": ((1000, 100, 50), er.Trim(keep_head=101, keep_tail=2 ** 40)),
             "keep some": ((1000, 100, 50), er.Trim(keep_head=30, keep_tail=50, pad_head=7, pad_tail=9)),
             "fades longer than what is kept": ((1000, 600, 390), er.Trim(fade_in_frames=480, fade_out_frames=2 ** 24, fade_in_curve=1, fade_out_curve=2)),
             "one frame kept": ((1000, 999, 0), er.Trim(fade_in_frames=1, fade_out_frames=5)),
             "no silence": ((77, 0, 0), er.Trim(fade_in_frames=480, fade_out_frames=48, pad_head=2 ** 39)),
             "a full row": ((2 ** 32 - 1, 1, 1), er.Trim())}
    for tag, ((n, lead, trail), rule) in cases.items():
        rec = inspect_record(n, lead, trail)
        want_clip, want_total = er.trim(rec, rule, 3, 5)
        got_clip, got_total = oa.edit_trim(omx, rec, oa.TrimRule(**rule.__dict__), 3, 5)
        assert got_clip.__dict__ == want_clip.__dict__ and got_total == want_total, (tag, got_clip, want_clip, got_total, want_total)
        assert got_clip.gain == 1.0 and got_clip.fade_in_frames <= got_clip.frames and got_clip.fade_out_frames <= got_clip.frames
        # the clip is one the table check accepts
        assert int(oa.edit_extent(omx, [got_clip], [0, 0, 0, n], 6)[5]) == (want_clip.dst_first + want_clip.frames if want_clip.frames else 0)
    clip, total = oa.edit_trim(omx, inspect_record(480, 480, 480), oa.TrimRule(pad_head=24000, pad_tail=96000))
    assert clip.frames == 0 and total == 120000
    clip, total = oa.edit_trim(omx, inspect_record(1000, 100, 50), oa.TrimRule())
    assert (clip.src_first, clip.frames, clip.dst_first, total) == (100, 850, 0, 850)
    clip, total = oa.edit_trim(omx, inspect_record(1000, 600, 390), oa.TrimRule(fade_in_frames=480, fade_out_frames=480))
    assert (clip.frames, clip.fade_in_frames, clip.fade_out_frames) == (10, 10, 10)


def test_trim_refuses_bad_arguments_and_writes_nothing(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_edit_trim", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    good_rec = np.ascontiguousarray(inspect_record(1000, 100, 50).reshape(1))
    good_rule = oa.TrimRule().to_c()

    def refused(rec, rule, tag):
        clip, total = np.full((48,), 0xAB, np.uint8), np.full((1,), 7, np.uint64)
        rc = fn(rec.ctypes.data if rec is not None else None, C.byref(rule) if rule is not None else None, 0, 0, clip.ctypes.data, total.ctypes.data)
        assert rc == capi.ERR_INVALID and (clip == 0xAB).all() and total[0] == 7, tag
        assert last_error(omx).startswith("program loudness edit trim: "), tag

    refused(None, good_rule, "null record")
    refused(good_rec, None, "null rule")
    total = np.zeros((1,), np.uint64)
    clip = np.zeros((48,), np.uint8)
    assert fn(good_rec.ctypes.data, C.byref(good_rule), 0, 0, None, total.ctypes.data) == capi.ERR_INVALID
    assert fn(good_rec.ctypes.data, C.byref(good_rule), 0, 0, clip.ctypes.data, None) == capi.ERR_INVALID and not clip.any()
    for kw in (dict(fade_in_curve=3), dict(fade_out_curve=3), dict(flags=1), dict(fade_in_frames=2 ** 24 + 1), dict(fade_out_frames=2 ** 24 + 1),
               dict(pad_head=2 ** 40), dict(pad_tail=2 ** 40 - 849), dict(pad_head=2 ** 63, pad_tail=2 ** 63)):
        refused(good_rec, oa.TrimRule(**kw).to_c(), kw)
        with pytest.raises(er.Invalid):
            er.trim(good_rec[0], er.Trim(**kw))
    padded = oa.TrimRule().to_c()
    padded._pad = 1
    refused(good_rec, padded, "padding set")
    for shape in ((10, 11, 0), (10, 0, 11), (10, 6, 5), (2 ** 32, 0, 0)):
        rec = np.ascontiguousarray(inspect_record(*shape).reshape(1))
        refused(rec, good_rule, shape)
        with pytest.raises(er.Invalid):
            er.trim(rec[0], er.Trim())
    assert fn(good_rec.ctypes.data, C.byref(oa.TrimRule(pad_tail=2 ** 40 - 850).to_c()), 0, 0, clip.ctypes.data, total.ctypes.data) == 0
    assert int(total[0]) == 2 ** 40

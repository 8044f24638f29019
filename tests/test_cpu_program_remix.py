"""Programme bank channel remix (include/omx/program_remix.h), CPU side: the header as C99, its structures' sizes and offsets, the
exported functions, the Python surface; the two preset builders of the library against the numpy restatement
(tests/program_remix_ref.py) byte for byte, and against the hand-written BS.775 table; every invalid argument of the host-only functions
with the output buffers still holding their sentinel; and the restatement against what the header's DEFINITION says follows from it.

Bars.  Matrices, positions and masks: equal on bytes.  Normalised rows: 1 + 2^-23 (each weight is one f32 division, the sum of up to
eight of them each within half an ulp of at most 1), and the ratio of two weights of a row within one ulp of f32 (numerator and
denominator are each within half an ulp of the exact quotient)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import program_remix_ref as mr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
C_LEVEL = np.float32(0.70710678)
ODD_LAYOUT = [mr.POS_FL, mr.POS_UNKNOWN, mr.POS_AUX0 + 1, mr.POS_FC, mr.POS_FC, mr.POS_FL, mr.POS_SR, mr.POS_MONO]      # duplicates included


def layouts():
    return [(ch, capi.positions_fallback(ch)) for ch in range(1, 9)] + [(8, ODD_LAYOUT), (5, ODD_LAYOUT)]


# ---------------------------------------------------------------- the header
def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


C99_USE = r'''
#include <stddef.h>
#include "omx/program_remix.h"
typedef char remix_info_is_16_bytes[sizeof(omx_program_remix_info) == 16 ? 1 : -1];
typedef char downmix_rule_is_20_bytes[sizeof(omx_program_downmix_rule) == 20 ? 1 : -1];
typedef char remix_record_is_32_bytes[sizeof(omx_program_remix_record) == 32 ? 1 : -1];
int main(void) {
    omx_program_downmix_rule rule;
    rule.kind = OMX_REMIX_KIND_MONO; rule.center_level = OMX_REMIX_DEFAULT_CENTER; rule.surround_level = OMX_REMIX_DEFAULT_SURROUND;
    rule.lfe_level = OMX_REMIX_DEFAULT_LFE; rule.flags = OMX_REMIX_NORMALIZE;
    return (int)offsetof(omx_program_remix_info, channels_in) - 4 + (int)offsetof(omx_program_remix_info, channels_out) - 8
        + (int)offsetof(omx_program_downmix_rule, center_level) - 4 + (int)offsetof(omx_program_downmix_rule, surround_level) - 8
        + (int)offsetof(omx_program_downmix_rule, lfe_level) - 12 + (int)offsetof(omx_program_downmix_rule, flags) - 16
        + (int)offsetof(omx_program_remix_record, samples_over) - 8 + (int)offsetof(omx_program_remix_record, out_sample_peak) - 16
        + (int)offsetof(omx_program_remix_record, out_sample_peak_db) - 20 + (int)offsetof(omx_program_remix_record, matrix_index) - 24
        + (int)offsetof(omx_program_remix_record, terms) - 28
        + (int)OMX_REMIX_KIND_STEREO + (int)rule.kind - 1 + (int)rule.flags - 1 + (int)(OMX_REMIX_MAX_MATRICES - 65536u)
        + (rule.center_level == 0.70710678f ? 0 : 1) + (rule.surround_level == rule.center_level ? 0 : 1) + (rule.lfe_level == 0.0f ? 0 : 1);
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
    assert C.sizeof(oa.CProgramRemixInfo) == 16 and C.sizeof(oa.CProgramDownmixRule) == 20 and C.sizeof(oa.CProgramRemixRecord) == 32
    assert oa.REMIX_RECORD_DTYPE.itemsize == 32 and oa.REMIX_RECORD_DTYPE.names == mr.RECORD_FIELDS and oa.REMIX_INFO_DTYPE.itemsize == 16
    for dtype, struct in ((oa.REMIX_RECORD_DTYPE, oa.CProgramRemixRecord), (oa.REMIX_INFO_DTYPE, oa.CProgramRemixInfo)):
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [getattr(oa.CProgramRemixRecord, f).offset for f in mr.RECORD_FIELDS] == [0, 8, 16, 20, 24, 28]
    assert [getattr(oa.CProgramDownmixRule, f).offset for f in ("kind", "center_level", "surround_level", "lfe_level", "flags")] == [0, 4, 8, 12, 16]
    syms = declared(os.path.join(INCLUDE, "program_remix.h"))
    assert syms == ["omx_program_loudness_bank_fetch_remixed", "omx_program_loudness_bank_remix", "omx_program_loudness_bank_remix_configure",
                    "omx_program_remix_downmix", "omx_program_remix_plan", "omx_program_remix_select"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_remix.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_remix" not in open(os.path.join(ROOT, "include", "omx.h")).read()


def test_python_surface(omx):
    import openmeters_amd as oa
    for name in ("configure_remix", "remix", "fetch_remixed"):
        assert callable(getattr(oa.ProgramLoudnessBank, name)), name
    c = oa.DownmixRule().to_c()
    assert (c.kind, c.flags) == (mr.KIND_STEREO, 0)
    assert (np.float32(c.center_level), np.float32(c.surround_level), np.float32(c.lfe_level)) == (mr.DEFAULT_CENTER, mr.DEFAULT_SURROUND, mr.DEFAULT_LFE)
    assert (oa.REMIX_KIND_STEREO, oa.REMIX_KIND_MONO, oa.REMIX_NORMALIZE, oa.REMIX_MAX_MATRICES) == (mr.KIND_STEREO, mr.KIND_MONO, mr.NORMALIZE, mr.MAX_MATRICES)
    for ci, co in itertools.product(range(1, 9), repeat=2):
        info = oa.remix_plan(omx, ci, co)
        assert (int(info["channels_in"]), int(info["channels_out"])) == (ci, co) and int(info["tile_frames"]) >= 4 and int(info["_pad"]) == 0


# ---------------------------------------------------------------- the presets
def test_the_restated_5_1_fold_is_the_bs775_table():
    c = s = C_LEVEL
    m, pos = mr.downmix(6, capi.positions_fallback(6))
    table = np.array([[1, 0, c, 0, s, 0], [0, 1, c, 0, 0, s]], np.float32)
    assert m.dtype == np.float32 and m.tobytes() == table.tobytes()
    assert pos == [mr.POS_FL, mr.POS_FR] + [mr.POS_UNKNOWN] * 6
    mono, pos = mr.downmix(6, capi.positions_fallback(6), kind=mr.KIND_MONO)
    assert mono.tobytes() == (np.float32(0.5) * (table[0] + table[1]))[None].tobytes() and pos[0] == mr.POS_MONO


def test_the_normalised_fold_cannot_exceed_full_scale_and_keeps_the_balance():
    plain, _ = mr.downmix(6, capi.positions_fallback(6))
    m, _ = mr.downmix(6, capi.positions_fallback(6), flags=mr.NORMALIZE)
    sums = np.abs(m.astype(np.float64)).sum(axis=1)
    print(f"normalised 5.1 fold: rows sum to {sums[0]:.9f} and {sums[1]:.9f} (bar {1 + 2.0 ** -23:.9f})")
    assert (sums <= 1.0 + 2.0 ** -23).all() and (sums > 0.99).all()
    before, after = np.float32(plain[0, 0] / plain[0, 2]), np.float32(m[0, 0] / m[0, 2])
    assert abs(float(after) - float(before)) <= float(np.spacing(before)), (before, after)
    # a full-scale input of any signs stays within full scale (one more rounding per term: 6 terms, 2^-24 each)
    worst = mr.remix(m, np.sign(m[0] + m[1])[None] * np.float32(1.0))
    assert np.abs(worst).max() <= 1.0 + 6 * 2.0 ** -24
    # nothing to normalise: the flag leaves a stereo layout alone
    assert mr.downmix(2, capi.positions_fallback(2), flags=mr.NORMALIZE)[0].tobytes() == np.eye(2, dtype=np.float32).tobytes()


LEVELS = [(0.0, 0.0, 0.0), (float(mr.DEFAULT_CENTER), float(mr.DEFAULT_SURROUND), float(mr.DEFAULT_LFE)), (2.0, 2.0, 2.0), (0.5, 1.0, 0.31622776)]


def test_library_presets_equal_the_restatement_on_bytes(omx):
    import openmeters_amd as oa
    cases = 0
    for (ch, pos), kind, flags, (c, s, l) in itertools.product(layouts(), (mr.KIND_STEREO, mr.KIND_MONO), (0, mr.NORMALIZE), LEVELS):
        want, want_pos = mr.downmix(ch, pos, kind, c, s, l, flags)
        got, got_pos = oa.remix_downmix(omx, oa.DownmixRule(kind, c, s, l, flags), ch, pos)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (ch, pos, kind, flags, c, s, l, got, want)
        assert got_pos == want_pos
        cases += 1
    assert cases == 10 * 2 * 2 * 4
    targets = [(2, [mr.POS_FL, mr.POS_FR]), (2, [mr.POS_SL, mr.POS_SR]), (6, [mr.POS_FL, mr.POS_FR, mr.POS_RL, mr.POS_RR, mr.POS_FC, mr.POS_LFE]),
               (1, [mr.POS_MONO]), (8, list(reversed(capi.positions_fallback(8)))), (3, [mr.POS_FC, mr.POS_FC, mr.POS_AUX0 + 1]), (8, ODD_LAYOUT)]
    for (ch, pos), (co, out_pos) in itertools.product(layouts(), targets):
        want, want_missing = mr.select(ch, pos, co, out_pos)
        got, got_missing = oa.remix_select(omx, ch, pos, co, out_pos)
        assert got.shape == (co, ch) and got.tobytes() == want.tobytes() and got_missing == want_missing, (ch, pos, co, out_pos)
    # the film order C L R Ls Rs LFE back to L R C LFE Ls Rs: a permutation, nothing missing
    film = [mr.POS_FC, mr.POS_FL, mr.POS_FR, mr.POS_RL, mr.POS_RR, mr.POS_LFE]
    m, missing = oa.remix_select(omx, 6, film, 6, capi.positions_fallback(6))
    assert missing == 0 and (m.sum(axis=0) == 1).all() and (m.sum(axis=1) == 1).all() and m[0, 1] == 1 and m[3, 5] == 1
    # the lowest of two equal positions is taken, an absent one is reported
    m, missing = oa.remix_select(omx, 8, ODD_LAYOUT, 3, [mr.POS_FC, mr.POS_FL, mr.POS_RR])
    assert missing == 0b100 and m[0, 3] == 1 and m[0, 4] == 0 and m[1, 0] == 1 and m[1, 5] == 0 and not m[2].any()


def test_every_invalid_argument_is_refused_with_nothing_written(omx):
    import openmeters_amd as oa
    plan_fn = omx.fn("program_remix_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p])
    down_fn = omx.fn("program_remix_downmix", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    sel_fn = omx.fn("program_remix_select", C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    u8x8 = C.c_uint8 * 8
    pos = u8x8(*capi.positions_fallback(6))

    for ci, co in ((0, 2), (9, 2), (2, 0), (2, 9), (2 ** 32 - 1, 1)):
        info = np.full((4,), 0xA5A5A5A5, np.uint32)
        assert plan_fn(ci, co, info.ctypes.data) == capi.ERR_INVALID and (info == 0xA5A5A5A5).all(), (ci, co)
    assert plan_fn(2, 2, None) == capi.ERR_INVALID

    def downmix(rule, ch=6, null=None):
        matrix, n_out, pos_out = np.full((16,), 7.25, np.float32), C.c_uint32(99), u8x8(*[0xA5] * 8)
        c = rule.to_c()
        args = dict(rule=C.byref(c), pos=pos, matrix=matrix.ctypes.data, n_out=C.byref(n_out), pos_out=pos_out)
        if null:
            args[null] = None
        rc = down_fn(args["rule"], ch, args["pos"], args["matrix"], args["n_out"], args["pos_out"])
        return rc, (matrix == 7.25).all() and n_out.value == 99 and list(pos_out) == [0xA5] * 8

    bad_rules = [dict(kind=2), dict(kind=2 ** 31), dict(flags=2), dict(flags=3), dict(flags=2 ** 31)]
    for field in ("center_level", "surround_level", "lfe_level"):
        bad_rules += [{field: v} for v in (-0.001, 2.001, float("nan"), float("inf"), float("-inf"))]
    for bad in bad_rules:
        rule = oa.DownmixRule(**bad)
        with pytest.raises(mr.Invalid):
            mr.downmix(6, capi.positions_fallback(6), rule.kind, rule.center_level, rule.surround_level, rule.lfe_level, rule.flags)
        rc, untouched = downmix(rule)
        assert rc == capi.ERR_INVALID and untouched, bad
    for ch in (0, 9, 2 ** 32 - 1):
        rc, untouched = downmix(oa.DownmixRule(), ch)
        assert rc == capi.ERR_INVALID and untouched, ch
    for null in ("rule", "pos", "matrix", "n_out", "pos_out"):
        rc, untouched = downmix(oa.DownmixRule(), 6, null)
        assert rc == capi.ERR_INVALID and untouched, null
    for good in (dict(center_level=0.0), dict(center_level=2.0), dict(lfe_level=2.0), dict(surround_level=0.0), dict(flags=1, kind=1)):      # the limits themselves
        rc, untouched = downmix(oa.DownmixRule(**good))
        assert rc == 0 and not untouched, good

    def select(ci=6, co=2, null=None):
        matrix, missing = np.full((64,), 7.25, np.float32), C.c_uint32(99)
        args = dict(pos_in=pos, pos_out=u8x8(*capi.positions_fallback(2)), matrix=matrix.ctypes.data, missing=C.byref(missing))
        if null:
            args[null] = None
        rc = sel_fn(ci, args["pos_in"], co, args["pos_out"], args["matrix"], args["missing"])
        return rc, (matrix == 7.25).all() and missing.value == 99

    for ci, co in ((0, 2), (9, 2), (6, 0), (6, 9)):
        rc, untouched = select(ci, co)
        assert rc == capi.ERR_INVALID and untouched, (ci, co)
        with pytest.raises(mr.Invalid):
            mr.select(ci, capi.positions_fallback(6), co, capi.positions_fallback(2))
    for null in ("pos_in", "pos_out", "matrix", "missing"):
        rc, untouched = select(null=null)
        assert rc == capi.ERR_INVALID and untouched, null
    rc, untouched = select()
    assert rc == 0 and not untouched


# ---------------------------------------------------------------- what follows from the DEFINITION, on the restatement
def special_rows(channels):
    x = mr.noise(11, 64, channels)
    x[3, 0], x[5, 1 % channels], x[7, channels - 1], x[9, 0] = np.nan, np.inf, -np.inf, -0.0
    x[11] = -0.0
    return x


def test_a_permutation_is_a_byte_copy():
    x = special_rows(6)
    perm = [2, 0, 1, 5, 3, 4]
    m = np.zeros((6, 6), np.float32)
    m[np.arange(6), perm] = 1.0
    assert mr.remix(m, x).tobytes() == x[:, perm].tobytes()
    assert np.signbit(mr.remix(m, x)[11]).all()      # -0.0f stays -0.0f: the first term is a product, not a sum with +0
    m[m == 0] = -0.0      # a zero of either sign is skipped
    assert mr.remix(m, x).tobytes() == x[:, perm].tobytes()
    sel, missing = mr.select(6, capi.positions_fallback(6), 6, [capi.positions_fallback(6)[p] for p in perm])
    assert missing == 0 and sel.tobytes() == np.abs(m).tobytes()


def test_a_dropped_channel_does_not_reach_the_output():
    fold, _ = mr.downmix(6, capi.positions_fallback(6))
    x = mr.noise(12, 32, 6, 0.25)
    x[4, 3], x[5, 3], x[6, 3] = np.inf, -np.inf, np.nan      # in the LFE, level 0
    y = mr.remix(fold, x)
    assert np.isfinite(y).all()
    clean = x.copy()
    clean[:, 3] = 0
    assert y.tobytes() == mr.remix(fold, clean).tobytes()
    rec = mr.record(y, fold)
    assert rec["terms"] == 6 and rec["samples_over"] == 0 and rec["frames"] == 32


def test_infinities_of_opposite_sign_give_nan_and_an_antiphase_pair_folds_to_plus_zero():
    m = np.array([[1.0, -1.0]], np.float32)
    y = mr.remix(m, np.array([[np.inf, np.inf], [1.0, 2.0]], np.float32))
    assert np.isnan(y[0, 0]) and y[1, 0] == -1.0
    mono, _ = mr.downmix(2, capi.positions_fallback(2), kind=mr.KIND_MONO)
    assert mono.tobytes() == np.array([[0.5, 0.5]], np.float32).tobytes()
    left = mr.noise(13, 200, 1)
    y = mr.remix(mono, np.concatenate([left, -left], axis=1))
    assert y.tobytes() == np.zeros((200, 1), np.float32).tobytes()      # x + (-x) is +0.0f in round-to-nearest, never -0.0f
    empty = mr.remix(np.zeros((2, 3), np.float32), special_rows(3))
    assert empty.tobytes() == np.zeros((64, 2), np.float32).tobytes()      # a row without a term: +0.0f whatever the input holds
    rec = mr.record(mr.remix(np.array([[1.0, 1.0]], np.float32), np.array([[0.75, 0.5], [np.nan, 0.0], [-np.inf, 1.0]], np.float32)), m)
    assert rec["samples_over"] == 2 and rec["out_sample_peak"] == np.inf and rec["out_sample_peak_db"] == np.inf


# ---------------------------------------------------------------- the C99 host
def build_demo(tmp_path):
    """tests/c_abi/program_remix_demo.c: a plain C99 host that takes one 5.1 S24 programme through import, the fold-down to Lo/Ro,
    process, plan_gains, apply_limited and the export as S16 stereo"""
    out = str(tmp_path / "program_remix_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_remix_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))

"""Programme bank signal QC (include/omx/program_inspect.h), CPU side: the header as C99, its structures' sizes and offsets, the exported
functions, the Python surface; the numpy restatement (tests/program_inspect_ref.py) pinned by hand-computed cases; the host-only
functions of the library (rule_default, plan, summarize) against the restatement and every invalid argument of theirs with the output
buffer still holding its sentinel.

Bars.  Verdict bits and integers: equal.  Linear floats (dc_offset, correlation): 1e-6 relative, host libm against numpy on the same
doubles, each then rounded to f32 (half an ulp, 6e-8).  dB values: 1e-4 dB, the family's bar."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_inspect_ref as ir
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
DB_BAR = 1e-4


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------- the restatement, by hand
def twelve_frames():
    nan = np.nan
    return np.array([(0, 0), (0, -0.0), (0.5, 0.25), (0.75, -0.5), (-1.0, 0.25), (0.25, nan), (0, 0), (0.25, 0.5), (0.5, 1.0), (0.5, -2.0),
                     (0, 0), (0, 0)], np.float32)


TWELVE_RULE = dict(clip_level=0.5, clip_min_run=2, silence_level=0.0, silence_min_run=2)


def test_restatement_gives_the_hand_computed_record_of_twelve_stereo_frames():
    """left is hot at frames 2 3 4 and 8 9, right at 3 and 7 8 9; frames 0 1, 6 and 10 11 are quiet (-0.0 is zero); frame 5 has a NaN on
    the right.  Sums: left 1.75, right -0.5 (the NaN gives 0); products ab -0.875, aa 2.4375, bb 0.0625 + 0.25 + 0.0625 + 0.25 + 1 +
    1 (4.0 clamped to 1) = 2.625 (the NaN frame gives 0 to ab and bb, 0.0625 to aa)."""
    rec = ir.record(twelve_frames(), 2, ir.Rule(**TWELVE_RULE), [(0, 1)])
    stream = {"frames": 12, "silent_frames": 5, "silent_runs": 2, "longest_silent_run": 2, "longest_silent_start": 0, "leading_silence": 2,
              "trailing_silence": 2, "channels": 2, "n_pairs": 1}
    left = {"dc_sum": 469762048, "nan_samples": 0, "clipped_samples": 5, "clip_runs": 2, "longest_clip_run": 3, "longest_clip_start": 2,
            "open_clip_run": 0, "_pad": 0}
    right = {"dc_sum": -134217728, "nan_samples": 1, "clipped_samples": 4, "clip_runs": 1, "longest_clip_run": 3, "longest_clip_start": 7,
             "open_clip_run": 0, "_pad": 0}
    pair = {"sum_ab": -939524096, "sum_aa": 2617245696, "sum_bb": 2818572288, "a": 0, "b": 1}
    assert {f: int(rec[f]) for f in stream} == stream
    assert {f: int(rec["channel"][0][f]) for f in left} == left
    assert {f: int(rec["channel"][1][f]) for f in right} == right
    assert {f: int(rec["pair"][0][f]) for f in pair} == pair
    assert not rec["channel"][2:].tobytes().strip(b"\0") and not rec["pair"][1:].tobytes().strip(b"\0")      # the rest is zero
    s = ir.summarize(ir.Rule(**TWELVE_RULE), rec)
    assert s["verdict"] == ir.NAN | ir.CLIPPED | ir.DC | ir.ANTIPHASE and s["interior_silent_runs"] == 0
    assert s["dc_offset"][0] == float(np.float32(1.75 / 12)) and s["dc_offset"][1] == float(np.float32(-0.5 / 12))
    assert abs(s["correlation"][0] - (-0.875 / np.sqrt(2.4375 * 2.625))) < 1e-7 and s["correlation_valid"] == [1, 0, 0, 0]


def test_restatement_runs_by_hand():
    f = ir.run_figures
    assert f([], 1) == (0, 0, 0, 0, 0)
    assert f([0, 0, 0], 1) == (0, 0, 0, 0, 0)
    assert f([1, 1, 1], 1) == (3, 1, 3, 0, 3) and f([1, 1, 1], 3) == (3, 1, 3, 0, 3) and f([1, 1, 1], 4) == (3, 0, 3, 0, 3)
    assert f([1, 0, 1, 1, 0, 1, 1, 0], 2) == (5, 2, 2, 2, 0)       # two longest runs: the earlier start
    assert f([0, 1, 1, 1, 0, 1], 1) == (4, 2, 3, 1, 1)
    assert list(ir.run_lengths([1, 1, 0, 1])) == [1, 2, 0, 1]


def test_restatement_hard_values_by_hand():
    rule = ir.Rule(clip_level=1.0, clip_min_run=1, silence_level=1e-4, silence_min_run=1)
    level = np.float32(1e-4)
    x = np.array([[np.inf], [-np.inf], [np.nan], [5.0], [-0.0], [1e-45], [level], [np.nextafter(level, np.float32(1))],
                  [np.nextafter(np.float32(1), np.float32(0))], [1.0]], np.float32)
    rec = ir.record(x, 1, rule)
    ch = rec["channel"][0]
    assert int(ch["nan_samples"]) == 1 and int(ch["clipped_samples"]) == 4 and int(ch["clip_runs"]) == 3      # inf -inf | 5.0 | 1.0
    assert int(rec["silent_frames"]) == 3 and int(rec["leading_silence"]) == 0 and int(rec["trailing_silence"]) == 0
    # inf and 5.0 clamp to 4, -inf to -4, NaN gives 0; 1e-45 and 1e-4 * 2^28 round to 0 and 26844 (26843.5456, and one ulp above)
    tail = int(np.rint(np.float32(np.nextafter(np.float32(1), np.float32(0))) * np.float32(2 ** 28))) + 2 ** 28
    assert int(ch["dc_sum"]) == 4 * 2 ** 28 + 2 * 26844 + tail
    assert list(ir.fixed([0.5 * 2.0 ** -28, 1.5 * 2.0 ** -28, 2.5 * 2.0 ** -28, -0.5 * 2.0 ** -28], 4.0, 2.0 ** 28)) == [0, 2, 2, 0]      # ties to even
    assert list(ir.fixed([2.25, -9.0, np.nan, np.inf], 1.0, 2.0 ** 30)) == [2 ** 30, -2 ** 30, 0, 2 ** 30]


# ---------------------------------------------------------------- the header
C99_USE = r'''
#include <stddef.h>
#include "omx/program_inspect.h"
typedef char rule_is_28_bytes[sizeof(omx_program_inspect_rule) == 28 ? 1 : -1];
typedef char info_is_16_bytes[sizeof(omx_program_inspect_info) == 16 ? 1 : -1];
typedef char channel_is_64_bytes[sizeof(omx_program_inspect_channel) == 64 ? 1 : -1];
typedef char pair_is_32_bytes[sizeof(omx_program_inspect_pair) == 32 ? 1 : -1];
typedef char record_is_704_bytes[sizeof(omx_program_inspect_record) == 704 ? 1 : -1];
typedef char summary_is_120_bytes[sizeof(omx_program_inspect_summary) == 120 ? 1 : -1];
int main(void) {
    return (int)offsetof(omx_program_inspect_rule, flags) - 24 + (int)offsetof(omx_program_inspect_record, trailing_silence) - 48
        + (int)offsetof(omx_program_inspect_record, channels) - 56 + (int)offsetof(omx_program_inspect_record, n_pairs) - 60
        + (int)offsetof(omx_program_inspect_record, channel) - 64 + (int)offsetof(omx_program_inspect_record, pair) - 576
        + (int)offsetof(omx_program_inspect_channel, open_clip_run) - 48 + (int)offsetof(omx_program_inspect_pair, a) - 24
        + (int)offsetof(omx_program_inspect_summary, interior_silent_runs) - 16 + (int)offsetof(omx_program_inspect_summary, dc_offset) - 24
        + (int)offsetof(omx_program_inspect_summary, correlation) - 88 + (int)offsetof(omx_program_inspect_summary, correlation_valid) - 104
        + (int)(OMX_INSPECT_MAX_PAIRS - 4u) + (int)(OMX_INSPECT_ANTIPHASE - 32u) + (OMX_INSPECT_DEFAULT_CLIP_LEVEL == 32767.0f / 32768.0f ? 0 : 1);
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
    sizes = {oa.CProgramInspectRule: 28, oa.CProgramInspectInfo: 16, oa.CProgramInspectChannel: 64, oa.CProgramInspectPair: 32,
             oa.CProgramInspectRecord: 704, oa.CProgramInspectSummary: 120}
    header = open(os.path.join(INCLUDE, "program_inspect.h")).read()
    for struct, size in sizes.items():
        assert C.sizeof(struct) == size
        name = "omx_program_inspect_" + struct.__name__[len("CProgramInspect"):].lower()
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), (name, "the header's comment does not give this size")
    assert oa.INSPECT_RECORD_DTYPE == ir.RECORD_DTYPE and oa.INSPECT_RECORD_DTYPE.itemsize == 704
    for dtype, struct in ((oa.INSPECT_RECORD_DTYPE, oa.CProgramInspectRecord), (oa.INSPECT_SUMMARY_DTYPE, oa.CProgramInspectSummary),
                          (oa.INSPECT_INFO_DTYPE, oa.CProgramInspectInfo)):
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [getattr(oa.CProgramInspectRecord, f).offset for f in ir.STREAM_FIELDS + ("channels", "n_pairs", "channel", "pair")] == [
        0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 576]
    assert [getattr(oa.CProgramInspectChannel, f).offset for f in ir.CHANNEL_FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56]
    assert [getattr(oa.CProgramInspectPair, f).offset for f in ir.PAIR_FIELDS] == [0, 8, 16, 24, 28]
    assert [getattr(oa.CProgramInspectRule, f).offset for f in ("clip_level", "clip_min_run", "silence_level", "silence_min_run", "dc_limit",
                                                                "correlation_min", "flags")] == [0, 4, 8, 12, 16, 20, 24]
    syms = declared(os.path.join(INCLUDE, "program_inspect.h"))
    assert syms == ["omx_program_inspect_plan", "omx_program_inspect_rule_default", "omx_program_inspect_summarize",
                    "omx_program_loudness_bank_fetch_inspected", "omx_program_loudness_bank_inspect",
                    "omx_program_loudness_bank_inspect_configure", "omx_program_loudness_bank_inspect_reset"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_inspect.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_inspect" not in open(os.path.join(ROOT, "include", "omx.h")).read()
    for name in ("InspectRule", "inspect_plan", "inspect_summarize", "INSPECT_RECORD_DTYPE"):
        assert hasattr(oa, name), name
    for name in ("configure_inspect", "reset_inspect", "inspect", "fetch_inspected"):
        assert hasattr(oa.ProgramLoudnessBank, name), name


def build_demo(tmp_path):
    """tests/c_abi/program_inspect_demo.c: a plain C99 host that inspects a stereo programme with a clipped passage, a dropout and an
    inverted right channel"""
    out = str(tmp_path / "program_inspect_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_inspect_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


# ---------------------------------------------------------------- rule_default, plan
def test_rule_default_and_plan(omx):
    import openmeters_amd as oa
    rule = oa.inspect_rule_default(omx)
    assert rule == oa.InspectRule(float(np.float32(32767.0 / 32768.0)), 3, 0.0, 480, float(np.float32(1e-3)), float(np.float32(-0.2)), 0)
    assert ir.Rule().valid() and np.float32(rule.clip_level) == ir.Rule().clip_level
    assert omx.fn("program_inspect_rule_default", C.c_int, [C.c_void_p])(None) == capi.ERR_INVALID
    plan = omx.fn("program_inspect_plan", C.c_int, [C.c_uint32, C.c_void_p])
    for ch in range(1, 9):
        info = oa.inspect_plan(omx, ch)
        t = int(info["tile_frames"])
        assert int(info["channels"]) == ch and t >= 64 and t % 64 == 0 and not info["_pad"].any()
    sentinel = np.full((1,), 0xAB, np.uint8).repeat(16)
    for ch in (0, 9, 2 ** 32 - 1):
        buf = sentinel.copy()
        assert plan(ch, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), ch
    assert plan(2, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- summarize
def summarize_both(omx, rule_kw, rec):
    import openmeters_amd as oa
    got = oa.inspect_summarize(omx, oa.InspectRule(**rule_kw), rec)
    want = ir.summarize(ir.Rule(**rule_kw), rec)
    for f in ("verdict", "channels", "n_pairs", "interior_silent_runs"):
        assert int(got[f]) == want[f], (f, got[f], want[f])
    assert list(got["correlation_valid"]) == want["correlation_valid"]
    for f in ("dc_offset", "correlation"):
        for g, w in zip(got[f], want[f]):
            assert abs(float(g) - w) <= 1e-6 * abs(w), (f, g, w)
    for g, w in zip(got["dc_offset_db"][:want["channels"]], want["dc_offset_db"]):
        assert abs(float(g) - w) <= DB_BAR, ("dc_offset_db", g, w)
    assert not got["dc_offset_db"][want["channels"]:].any() and int(got["_pad"]) == 0
    return got


def test_summarize_equals_the_restatement(omx):
    got = summarize_both(omx, TWELVE_RULE, ir.record(twelve_frames(), 2, ir.Rule(**TWELVE_RULE), [(0, 1)]))
    assert int(got["verdict"]) == ir.NAN | ir.CLIPPED | ir.DC | ir.ANTIPHASE
    rng = np.random.default_rng(3)
    seen = 0
    for i in range(40):
        ch = 1 + i % 8
        kw = dict(clip_level=float(rng.choice([0.5, 0.99996948, 1.0])), clip_min_run=int(rng.integers(1, 5)), silence_level=float(rng.choice([0.0, 1e-3])),
                  silence_min_run=int(rng.integers(1, 6)), dc_limit=float(rng.choice([0.0, 1e-3, 0.1])), correlation_min=float(rng.choice([-1.0, -0.2, 0.5, 1.0])))
        x = ir.noise(500 + i, int(rng.integers(0, 400)), ch, float(rng.choice([0.3, 1.2])), int(rng.integers(2, 9)))
        if i % 3 == 0 and len(x):
            x += np.float32(0.05)
        if i % 5 == 0 and len(x) > 8:
            x[:7] = 0
            x[8, 0] = np.nan
        pairs = [] if ch == 1 else [(0, ch - 1), (ch - 1, 0)][:1 + i % 2]
        seen |= int(summarize_both(omx, kw, ir.record(x, ch, ir.Rule(**kw), pairs))["verdict"])
    assert (seen | ir.ALL_SILENT) == 63, "the random records do not raise every verdict bit but ALL_SILENT (the edge cases below raise it)"
    # sums at the far end of their range: 2^32 - 1 frames at +4 in one channel and -4 in the other, a pair at full correlation
    rec = np.zeros((), ir.RECORD_DTYPE)
    rec["frames"], rec["channels"], rec["n_pairs"] = 2 ** 32 - 1, 2, 2
    rec["channel"][0]["dc_sum"], rec["channel"][1]["dc_sum"] = (2 ** 32 - 1) * 2 ** 30, -(2 ** 32 - 1) * 2 ** 30
    rec["pair"][0]["sum_ab"], rec["pair"][0]["sum_aa"], rec["pair"][0]["sum_bb"] = -(2 ** 32 - 1) * 2 ** 30, (2 ** 32 - 1) * 2 ** 30, (2 ** 32 - 1) * 2 ** 30
    rec["pair"][1]["sum_ab"], rec["pair"][1]["sum_aa"], rec["pair"][1]["sum_bb"], rec["pair"][1]["a"] = 5, 3, 0, 1
    got = summarize_both(omx, {}, rec)
    assert float(got["dc_offset"][0]) == 4.0 and float(got["dc_offset"][1]) == -4.0 and float(got["correlation"][0]) == -1.0
    assert list(got["correlation_valid"]) == [1, 0, 0, 0] and float(got["correlation"][1]) == 0.0


def test_interior_silent_runs_at_the_edges(omx):
    kw = dict(silence_min_run=2, dc_limit=4.0)      # (no offset exceeds 4: the DC bit stays out of the way)
    rule = ir.Rule(**kw)
    loud = np.float32(0.5)
    cases = {"all silent": ([0, 0, 0, 0, 0], 0, ir.ALL_SILENT),       # the leading run is also the trailing run: counted once
             "leading only": ([0, 0, loud, loud], 0, 0),
             "trailing only": ([loud, 0, 0], 0, 0),
             "leading, interior, trailing": ([0, 0, loud, 0, 0, loud, 0, 0], 1, ir.DROPOUT),
             "a short leading run and an interior one": ([0, loud, 0, 0, loud], 1, ir.DROPOUT),
             "a short trailing run and an interior one": ([loud, 0, 0, 0, loud, 0], 1, ir.DROPOUT),
             "one silent frame": ([0], 0, ir.ALL_SILENT),
             "no frames": ([], 0, 0),
             "runs below the minimum": ([0, loud, 0, loud, 0], 0, 0)}
    for tag, (samples, interior, verdict) in cases.items():
        rec = ir.record(np.array(samples, np.float32).reshape(-1, 1), 1, rule)
        got = summarize_both(omx, kw, rec)
        assert int(got["interior_silent_runs"]) == interior and int(got["verdict"]) == verdict, (tag, got)


def test_summarize_refuses_bad_arguments(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_inspect_summarize", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    rec = np.zeros((1,), oa.INSPECT_RECORD_DTYPE)
    rec["channels"] = 2
    good = oa.InspectRule().to_c()
    out = np.full((120,), 0xAB, np.uint8)
    assert fn(C.byref(good), rec.ctypes.data, out.ctypes.data) == 0 and not (out == 0xAB).all()

    def refused(rule, record, tag):
        buf = np.full((120,), 0xAB, np.uint8)
        assert fn(C.byref(rule) if rule is not None else None, record.ctypes.data if record is not None else None, buf.ctypes.data) == capi.ERR_INVALID, tag
        assert (buf == 0xAB).all(), (tag, "the summary was written")

    refused(None, rec, "null rule")
    refused(good, None, "null record")
    assert fn(C.byref(good), rec.ctypes.data, None) == capi.ERR_INVALID
    bad_rules = [dict(clip_level=0.0), dict(clip_level=-1.0), dict(clip_level=np.nan), dict(clip_level=np.inf), dict(clip_min_run=0),
                 dict(clip_min_run=65536), dict(silence_level=-1e-9), dict(silence_level=np.nan), dict(silence_level=np.inf),
                 dict(silence_min_run=0), dict(silence_min_run=2 ** 24 + 1), dict(dc_limit=-1.0), dict(dc_limit=np.nan), dict(dc_limit=np.inf),
                 dict(correlation_min=-1.5), dict(correlation_min=1.5), dict(correlation_min=np.nan), dict(flags=1)]
    for kw in bad_rules:
        refused(oa.InspectRule(**kw).to_c(), rec, kw)
        assert not ir.Rule(**kw).valid(), kw
    for kw in (dict(clip_min_run=65535), dict(silence_min_run=2 ** 24), dict(correlation_min=-1.0), dict(correlation_min=1.0), dict(dc_limit=0.0)):
        assert fn(C.byref(oa.InspectRule(**kw).to_c()), rec.ctypes.data, out.ctypes.data) == 0 and ir.Rule(**kw).valid(), kw
    for channels, n_pairs in ((0, 0), (9, 0), (2, 5)):
        bad = rec.copy()
        bad["channels"], bad["n_pairs"] = channels, n_pairs
        refused(good, bad, (channels, n_pairs))
        with pytest.raises(ir.Invalid):
            ir.summarize(ir.Rule(), bad[0])

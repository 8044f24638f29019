"""Programme bank PCM formats (include/omx/program_pcm.h), CPU side: the header as C99, its structures' sizes and offsets, the exported
functions, omx_pcm_format_bytes and every invalid rule, omx_program_dither_evaluate against the restatement bit for bit; and the numpy
restatement (tests/program_pcm_ref.py) against the definition's own properties: the dither's statistics, the error bound, a sine
below one LSB, exact round trips, the rounding of halves, the clamp, and pieces with carried position against the whole.

Bars.  Dither statistics over N = 2^20 draws, each five standard errors of an ideal triangular density on (-1, 1): mean
5 sqrt(1 / 6N); variance 5 sqrt((1/15 - 1/36) / N) (fourth moment 1/15); every correlation 5 / sqrt(N).  Error bound: |d| < 1 and the
rounding moves by at most 1/2, so |y - sv| < 1.5.  The sine: a signal of variance A^2 / 2 under a total error of variance 1/4 that is
uncorrelated with it (what TPDF dither gives) correlates at rho = sqrt(A^2/2 / (A^2/2 + 1/4)); bar five standard errors
(1 - rho^2) / sqrt(N) of a sample correlation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_pcm_ref as pr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
FORMATS = (pr.S16, pr.S24, pr.S32)


# ---------------------------------------------------------------- the header
def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


C99_USE = r'''
#include <stddef.h>
#include "omx/program_pcm.h"
typedef char export_rule_is_24_bytes[sizeof(omx_program_export_rule) == 24 ? 1 : -1];
typedef char export_record_is_48_bytes[sizeof(omx_program_export_record) == 48 ? 1 : -1];
int main(void) {
    omx_program_export_rule rule;
    rule.format = OMX_PCM_S24; rule.dither = OMX_DITHER_TPDF; rule.seed = 1; rule.flags = 0; rule._pad = 0;
    return (int)sizeof(rule) - 24 + (int)offsetof(omx_program_export_rule, seed) - 8 + (int)offsetof(omx_program_export_rule, flags) - 16
        + (int)offsetof(omx_program_export_record, samples_nan) - 24 + (int)offsetof(omx_program_export_record, out_peak) - 32
        + (int)offsetof(omx_program_export_record, dither) - 44 + (int)(OMX_PCM_S16 + OMX_PCM_S24 + OMX_PCM_S32) - 6
        + (int)(OMX_DITHER_NONE + OMX_DITHER_TPDF) - 1 + (int)rule.flags;
}
'''


def test_header_is_c99_its_structures_have_their_sizes_and_every_function_is_exported(tmp_path, omx):
    src = tmp_path / "use.c"
    src.write_text(C99_USE)
    exe = tmp_path / "use"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    assert subprocess.run([str(exe)]).returncode == 0
    import openmeters_amd
    assert C.sizeof(openmeters_amd.CProgramExportRule) == 24 and C.sizeof(openmeters_amd.CProgramExportRecord) == 48
    assert openmeters_amd.EXPORT_RECORD_DTYPE.itemsize == 48 and openmeters_amd.EXPORT_RECORD_DTYPE.names == pr.RECORD_FIELDS
    for f in openmeters_amd.EXPORT_RECORD_DTYPE.names:
        assert openmeters_amd.EXPORT_RECORD_DTYPE.fields[f][1] == getattr(openmeters_amd.CProgramExportRecord, f).offset, f
    assert [getattr(openmeters_amd.CProgramExportRecord, f).offset for f in pr.RECORD_FIELDS] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert [getattr(openmeters_amd.CProgramExportRule, f).offset for f in ("format", "dither", "seed", "flags")] == [0, 4, 8, 16]
    syms = declared(os.path.join(INCLUDE, "program_pcm.h"))
    assert syms == ["omx_pcm_format_bytes", "omx_program_dither_evaluate", "omx_program_loudness_bank_export_configure",
                    "omx_program_loudness_bank_export_pcm", "omx_program_loudness_bank_export_reset",
                    "omx_program_loudness_bank_fetch_exported", "omx_program_loudness_bank_import_pcm"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_pcm.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_pcm" not in open(os.path.join(ROOT, "include", "omx.h")).read()


def test_python_surface():
    import openmeters_amd
    for name in ("import_pcm", "configure_export", "reset_export", "export_pcm", "fetch_exported"):
        assert callable(getattr(openmeters_amd.ProgramLoudnessBank, name)), name
    assert (openmeters_amd.PCM_S16, openmeters_amd.PCM_S24, openmeters_amd.PCM_S32) == (pr.S16, pr.S24, pr.S32) == (1, 2, 3)
    assert (openmeters_amd.DITHER_NONE, openmeters_amd.DITHER_TPDF) == (pr.NONE, pr.TPDF) == (0, 1)
    c = openmeters_amd.ExportRule(pr.S24, pr.TPDF, 2 ** 64 - 3).to_c()
    assert (c.format, c.dither, c.seed, c.flags) == (2, 1, 2 ** 64 - 3, 0)
    assert callable(openmeters_amd.pcm_format_bytes) and callable(openmeters_amd.dither_value)


def test_format_bytes_and_every_invalid_rule_is_refused_with_nothing_written(omx):
    import openmeters_amd
    fn = omx.fn("pcm_format_bytes", C.c_int, [C.c_uint32, C.c_void_p])
    out = C.c_uint32(0xA5A5A5A5)
    for fmt in (0, 4, 5, 2 ** 32 - 1):
        assert fn(fmt, C.byref(out)) == capi.ERR_INVALID and out.value == 0xA5A5A5A5, fmt
    for fmt in FORMATS:
        assert fn(fmt, None) == capi.ERR_INVALID
        assert openmeters_amd.pcm_format_bytes(omx, fmt) == pr.BYTES[fmt]
    ev = omx.fn("program_dither_evaluate", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])
    d = C.c_double(123.25)
    for bad in ((0, 1, 1, 0), (4, 1, 1, 0), (2 ** 32 - 1, 0, 1, 0), (1, 2, 1, 0), (1, 2 ** 32 - 1, 1, 0), (1, 1, 1, 1), (3, 0, 1, 2 ** 31)):
        assert not pr.rule_valid(bad), bad
        c = openmeters_amd.ExportRule(*bad).to_c()
        assert ev(C.byref(c), 0, 0, 0, C.byref(d)) == capi.ERR_INVALID and d.value == 123.25, bad
        with pytest.raises(capi.OmxError) as err:
            openmeters_amd.dither_value(omx, openmeters_amd.ExportRule(*bad), 0, 0, 0)
        assert err.value.status == capi.ERR_INVALID
    good = openmeters_amd.ExportRule(pr.S16, pr.TPDF, 1).to_c()
    assert ev(None, 0, 0, 0, C.byref(d)) == capi.ERR_INVALID and ev(C.byref(good), 0, 0, 0, None) == capi.ERR_INVALID
    assert ev(C.byref(good), 0, 0, 8, C.byref(d)) == capi.ERR_INVALID and d.value == 123.25
    for fmt in FORMATS:
        assert openmeters_amd.dither_value(omx, openmeters_amd.ExportRule(fmt, pr.NONE, 7), 3, 5, 1) == 0.0


def test_dither_evaluate_equals_the_restatement_bit_for_bit(omx):
    import openmeters_amd
    frames = [0, 1, 2, 7, 1000, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 61 - 1, 2 ** 64 - 1]
    for seed in (0, 1, 2, 0xDEADBEEF, 2 ** 63, 2 ** 64 - 1):
        for stream in (0, 1, 2, 1023, 2 ** 32 - 1, 2 ** 40):
            rule = openmeters_amd.ExportRule(pr.S16, pr.TPDF, seed)
            for c in range(8):
                want = pr.dither(seed, stream, frames, c)
                got = np.array([openmeters_amd.dither_value(omx, rule, stream, f, c) for f in frames])
                assert got.tobytes() == want.tobytes(), (seed, stream, c)
                assert (np.abs(want) < 1.0).all()


# ---------------------------------------------------------------- the dither's statistics
def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_dither_statistics():
    N = 2 ** 20
    n = np.arange(N, dtype=np.uint64)
    d0, d1, other = pr.dither(1, 0, n, 0), pr.dither(1, 0, n, 1), pr.dither(1, 1, n, 0)
    se = 1.0 / np.sqrt(N)
    figures = {"mean": (d0.mean(), 0.0, 5.0 * np.sqrt(1.0 / 6.0 / N)),
               "variance": (d0.var(), 1.0 / 6.0, 5.0 * np.sqrt((1.0 / 15.0 - 1.0 / 36.0) / N)),
               "lag-1 correlation": (corr(d0[:-1], d0[1:]), 0.0, 5.0 * se),
               "correlation between channels 0 and 1": (corr(d0, d1), 0.0, 5.0 * se),
               "correlation between streams 0 and 1": (corr(d0, other), 0.0, 5.0 * se)}
    for name, (got, want, bar) in figures.items():
        print(f"dither {name}: {got:.6e} (expected {want:.6e}, bar {bar:.3e})")
    for name, (got, want, bar) in figures.items():
        assert abs(got - want) <= bar, (name, got, want, bar)
    assert d0.min() > -1.0 and d0.max() < 1.0 and d0.min() < -0.97 and d0.max() > 0.97
    assert (pr.dither(2, 0, n[:1000], 0) != d0[:1000]).any()


def test_error_stays_below_one_and_a_half_lsb():
    for fmt in FORMATS:
        x = pr.noise(3, 20000, 2, 0.9)
        y, clipped, nan, sv = pr.quantise(x, pr.dither_block((fmt, pr.TPDF, 5), 2, 10 ** 9, 20000, 2), fmt)
        assert not clipped.any() and not nan.any()
        worst = float(np.abs(y - sv).max())
        print(f"format {fmt}: largest |y - sv| = {worst:.4f} LSB")
        assert worst < 1.5


def test_a_sine_below_one_lsb_survives_only_with_dither():
    N, A = 2 ** 16, 0.4
    for fmt in (pr.S16, pr.S24):
        x = pr.low_sine(N, 1, fmt, A)
        raw, counts = pr.export_pcm(x, (fmt, pr.NONE, 0), 0, 0)
        assert raw == bytes(len(raw)) and counts == {"samples_clipped": 0, "samples_nan": 0, "out_peak": 0}
        raw, _ = pr.export_pcm(x, (fmt, pr.TPDF, 1), 0, 0)
        y = pr.unpack(raw, fmt).astype(np.float64)
        s = x[:, 0].astype(np.float64) * 2.0 ** (pr.BITS[fmt] - 1)
        rho = np.sqrt(A * A / 2.0 / (A * A / 2.0 + 0.25))
        got, bar = corr(y, s), 5.0 * (1.0 - rho * rho) / np.sqrt(N)
        print(f"format {fmt}: correlation {got:.4f} (expected {rho:.4f}, bar {bar:.4f}), error variance {np.var(y - s):.4f} (expected 0.25)")
        assert abs(got - rho) <= bar


# ---------------------------------------------------------------- exactness
def round_trip(values, fmt):
    raw = pr.pack(values, fmt)
    x = pr.import_pcm(raw, fmt, 1)
    back, counts = pr.export_pcm(x, (fmt, pr.NONE, 0), 0, 0)
    return raw, back, counts, x


def test_export_of_import_is_the_identity():
    raw, back, counts, x = round_trip(np.arange(-32768, 32768), pr.S16)
    assert back == raw and counts["samples_clipped"] == 0 and counts["out_peak"] == 32768
    assert x[0, 0] == -1.0 and x[-1, 0] == np.float32(32767.0 / 32768.0)
    rng = np.random.default_rng(11)
    v24 = np.concatenate([[-2 ** 23, 2 ** 23 - 1, 0, -1, 1], rng.integers(-2 ** 23, 2 ** 23, 10000)])
    raw, back, counts, _ = round_trip(v24, pr.S24)
    assert back == raw and counts["samples_clipped"] == 0 and counts["out_peak"] == 2 ** 23
    v32 = np.concatenate([[-2 ** 31, 2 ** 31 - 128, 0, -1, 1], rng.integers(-2 ** 23, 2 ** 23, 10000) << rng.integers(0, 9, 10000)])
    assert (v32.astype(np.float32).astype(np.int64) == v32).all()      # only values that are exact in f32 take part: 24 bits, shifted
    raw, back, counts, _ = round_trip(v32, pr.S32)
    assert back == raw and counts["samples_clipped"] == 0 and counts["out_peak"] == 2 ** 31


def test_halves_round_up_and_full_scale_clips():
    for fmt in (pr.S16, pr.S24):
        full = 2.0 ** (pr.BITS[fmt] - 1)
        ks = np.array([-5, -2, -1, 0, 1, 2, 1000, -1001], np.int64)
        x = ((ks + 0.5) / full).astype(np.float32).reshape(-1, 1)
        raw, counts = pr.export_pcm(x, (fmt, pr.NONE, 0), 0, 0)
        assert (pr.unpack(raw, fmt) == ks + 1).all() and counts["samples_clipped"] == 0
    for fmt in FORMATS:
        hi, lo = 2 ** (pr.BITS[fmt] - 1) - 1, -2 ** (pr.BITS[fmt] - 1)
        x = np.array([[1.0], [-1.0], [np.inf], [-np.inf], [np.nan], [2.0], [-2.0]], np.float32)
        raw, counts = pr.export_pcm(x, (fmt, pr.NONE, 0), 0, 0)
        assert list(pr.unpack(raw, fmt)) == [hi, lo, hi, lo, 0, hi, lo]
        assert counts == {"samples_clipped": 5, "samples_nan": 1, "out_peak": -lo}      # +1.0 is counted, -1.0 is not
        raw, counts = pr.export_pcm(x[:1], (fmt, pr.NONE, 0), 0, 0)
        assert counts["samples_clipped"] == 1
        raw, counts = pr.export_pcm(x[1:2], (fmt, pr.NONE, 0), 0, 0)
        assert counts["samples_clipped"] == 0 and list(pr.unpack(raw, fmt)) == [lo]
    assert pr.import_pcm(pr.pack([2 ** 31 - 1], pr.S32), pr.S32, 1)[0, 0] == np.float32(1.0)
    assert pr.import_pcm(pr.pack([2 ** 24 + 1, 2 ** 24 + 3], pr.S32), pr.S32, 1).reshape(-1).tolist() == [2.0 ** -7, (2.0 ** 24 + 4) * 2.0 ** -31]
    assert pr.peak_db(2 ** 15, pr.S16, -99.9) == 0.0 and pr.peak_db(0, pr.S16, -99.9) == -99.9


def test_pieces_with_carried_position_equal_the_whole():
    for fmt in FORMATS:
        for ch in (1, 3):
            x = pr.hard(20 + ch, 3000, ch, fmt)
            rule = (fmt, pr.TPDF, 99)
            whole, counts = pr.export_pcm(x, rule, 4, 0)
            for cuts in ([3000], [0, 1, 7, 1000, 0, 1992], [1] * 20 + [2980]):
                ex, parts, at = pr.Exporter(rule, 4), [], 0
                for f in cuts:
                    parts.append(ex.feed(x[at:at + f]))
                    at += f
                rec = ex.record()
                assert b"".join(parts) == whole, (fmt, ch, cuts[:3])
                assert (rec["samples_clipped"], rec["samples_nan"], rec["out_peak"]) == tuple(counts[k] for k in ("samples_clipped", "samples_nan", "out_peak"))
                assert rec["frames_out"] == 3000 and rec["frames_written"] == cuts[-1]
            other, _ = pr.export_pcm(x, rule, 5, 0)
            shifted, _ = pr.export_pcm(x, rule, 4, 1)
            assert other != whole and shifted != whole


# ---------------------------------------------------------------- the C99 host
def build_demo(tmp_path):
    """tests/c_abi/program_pcm_demo.c: a plain C99 host that takes one S16 programme through import, process, plan_gains, apply_limited
    and the export as S16 with TPDF dither"""
    out = str(tmp_path / "program_pcm_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_pcm_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))

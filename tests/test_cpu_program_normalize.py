"""Programme bank normalisation (include/omx/program_normalize.h), CPU side: omx_program_gain_evaluate, the host twin of the plan
kernels (one inline function serves both), against the numpy restatement (tests/program_normalize_ref.py) on a grid that crosses
every branch; every invalid rule; the header as C99 and its structures' sizes; and the known answers, from the restatements alone,
that make the inputs of the GPU round trip (tests/test_gpu_program_normalize.py) fair: every known programme keeps its gate counts
and its gate margin when it is scaled by its gain, and lands on the predicted loudness within the project's LUFS bar.

Bars: gain_db, predicted_*, limited_by and peak_known equal bits; `gain` within 1 f32 ulp: pow is the only step whose f64 result may
differ between libraries, and one f64 ulp moves the f32 rounding by at most one."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import program_groups_ref as gr
import program_loudness_ref as ref
import program_normalize_ref as nr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
FLOOR = -99.9
LUFS_BAR = 1e-4


def rule_of(t):
    import openmeters_amd
    return openmeters_amd.GainRule(*t)


def evaluate(omx, rule, I, n, P, F=FLOOR):
    import openmeters_amd
    return openmeters_amd.evaluate_gain(omx, rule_of(rule), I, n, P, F)


# ---------------------------------------------------------------- the grid
RULES = [(-23.0, -1.0, -60.0, 60.0, 0),                      # target only
         (-23.0, -1.0, -60.0, 60.0, nr.LIMIT_PEAK),          # the EBU pair
         (-14.0, -1.0, -60.0, 60.0, nr.LIMIT_PEAK),          # a louder target: the peak limit binds often
         (-23.0, -25.0, -60.0, 60.0, nr.LIMIT_PEAK),
         (-23.0, -25.0, -1.5, 5.0, nr.LIMIT_PEAK),           # both clamps; the minimum overrides the peak limit
         (-23.0, -1.0, 2.0, 2.0, 0),                         # min == max
         (-23.0, np.nan, -6.0, 6.0, 0),                      # a ceiling that is not in use may be anything
         (-23.1, -0.3, -12.34, 12.34, nr.LIMIT_PEAK),        # values that are no short binary fractions
         (-0.0, 0.0, -0.0, 0.0, nr.LIMIT_PEAK),              # negative zeros
         (0.0, -0.0, 0.0, 0.0, 0)]
LOUDNESS = [-23.0, -29.0, -50.0, -20.0, -30.0, -29.3337, -1.2345678, -23.000002, -70.0, -5.5, 0.0, -0.0, FLOOR]
COUNTS = [0, 1, 197, 2 ** 40]
PEAKS = [FLOOR, -99.8, -50.0, -29.01, -23.0, -3.0, -1.0, -0.99, 0.0, -0.0, 3.2, np.inf]


def test_evaluate_equals_the_restatement_on_every_branch(omx):
    seen, n = set(), 0
    for rule, I, count, P in itertools.product(RULES, LOUDNESS, COUNTS, PEAKS):
        got, want = evaluate(omx, rule, I, count, P), nr.gain(rule, I, count, P, FLOOR)
        nr.check_record(got, want, (rule, I, count, P))
        overrides = (want["limited_by"] == nr.BY_MIN_GAIN and (rule[4] & nr.LIMIT_PEAK) and want["peak_known"]
                     and float(want["predicted_peak_db"]) > rule[1])
        seen.add((int(want["limited_by"]), int(want["peak_known"]), bool(rule[4] & nr.LIMIT_PEAK), bool(overrides)))
        n += 1
    # every branch was crossed: each limit with the peak known and unknown, with and without LIMIT_PEAK, and the override
    for by in (nr.BY_TARGET, nr.BY_MAX_GAIN, nr.BY_MIN_GAIN, nr.BY_NO_MEASUREMENT):
        for known, limit in itertools.product((0, 1), (False, True)):
            assert any(s[:3] == (by, known, limit) for s in seen), (by, known, limit)
    assert any(s[0] == nr.BY_PEAK and s[1] == 1 and s[2] for s in seen)
    assert not any(s[0] == nr.BY_PEAK and (s[1] == 0 or not s[2]) for s in seen)       # no peak limit without a known peak or the flag
    assert any(s[3] for s in seen), "the minimum clamp never overrode the peak limit"
    print(n, "evaluations,", len(seen), "distinct branch signatures")


def test_evaluate_particular_answers(omx):
    """readable cases next to the grid: what a host expects from the names"""
    r = evaluate(omx, (-23.0, -1.0, -60.0, 60.0, nr.LIMIT_PEAK), -29.0, 10, -3.0)
    assert (r["gain_db"], r["limited_by"], r["predicted_lufs"], r["predicted_peak_db"]) == (2.0, nr.BY_PEAK, -27.0, -1.0)
    r = evaluate(omx, (-23.0, -1.0, -60.0, 60.0, 0), -29.0, 10, -3.0)
    assert (r["gain_db"], r["limited_by"], r["predicted_peak_db"], r["peak_known"]) == (6.0, nr.BY_TARGET, 3.0, 1)
    assert abs(float(r["gain"]) - 10.0 ** 0.3) < 2e-7
    r = evaluate(omx, (-23.0, -1.0, -60.0, 60.0, nr.LIMIT_PEAK), -29.0, 10, FLOOR)     # a peak at the floor limits nothing
    assert (r["gain_db"], r["limited_by"], r["peak_known"]) == (6.0, nr.BY_TARGET, 0) and r["predicted_peak_db"] == np.float32(FLOOR)
    r = evaluate(omx, (-23.0, -1.0, 3.0, 60.0, nr.LIMIT_PEAK), -29.0, 10, -3.0)        # the minimum wins: predicted peak above the ceiling
    assert (r["gain_db"], r["limited_by"], r["predicted_peak_db"]) == (3.0, nr.BY_MIN_GAIN, 0.0)
    r = evaluate(omx, (-23.0, -1.0, -60.0, 60.0, nr.LIMIT_PEAK), FLOOR, 0, -3.0)
    assert (r["gain_db"], r["gain"], r["limited_by"], r["predicted_lufs"], r["predicted_peak_db"]) == (0.0, 1.0, nr.BY_NO_MEASUREMENT, np.float32(FLOOR), -3.0)
    # a gain whose f64 value is no f32: the record holds the rounded one and predicts from it
    I, target = np.float32(-1.2345678), np.float32(-23.1)      # (operands of different exponents: the f64 difference keeps bits an f32 drops)
    g64 = np.float64(target) - np.float64(I)
    assert np.float64(np.float32(g64)) != g64
    r = evaluate(omx, (float(target), -1.0, -60.0, 60.0, 0), float(I), 10, FLOOR)
    assert r["gain_db"] == np.float32(g64) and r["predicted_lufs"] == np.float32(np.float64(I) + np.float64(np.float32(g64)))
    # negative zero survives: -0.0 - 0.0 = -0.0, and no clamp at +0.0 touches it
    r = evaluate(omx, (-0.0, 0.0, 0.0, 0.0, 0), 0.0, 1, FLOOR)
    assert r["gain_db"].tobytes() == np.float32(-0.0).tobytes() and r["gain"] == 1.0 and r["limited_by"] == nr.BY_TARGET


BAD_RULES = [(np.nan, -1.0, -60.0, 60.0, 0), (np.inf, -1.0, -60.0, 60.0, 0), (-np.inf, -1.0, -60.0, 60.0, 0),
             (-23.0, -1.0, np.nan, 60.0, 0), (-23.0, -1.0, -np.inf, 60.0, 0), (-23.0, -1.0, -60.0, np.nan, 0), (-23.0, -1.0, -60.0, np.inf, 0),
             (-23.0, -1.0, 1.0, 0.5, 0), (-23.0, -1.0, 0.0, -0.0001, nr.LIMIT_PEAK),
             (-23.0, np.nan, -60.0, 60.0, nr.LIMIT_PEAK), (-23.0, np.inf, -60.0, 60.0, nr.LIMIT_PEAK), (-23.0, -np.inf, -60.0, 60.0, nr.LIMIT_PEAK),
             (-23.0, -1.0, -60.0, 60.0, 2), (-23.0, -1.0, -60.0, 60.0, 3), (-23.0, -1.0, -60.0, 60.0, 2 ** 31), (-23.0, -1.0, -60.0, 60.0, 2 ** 32 - 1)]


def test_every_invalid_rule_is_refused_and_writes_nothing(omx):
    import openmeters_amd
    fn = omx.fn("program_gain_evaluate", C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_float, C.c_float, C.c_void_p])
    out = np.full((1,), 0xA5, np.uint8).repeat(32).view(openmeters_amd.GAIN_RECORD_DTYPE)
    before = out.tobytes()
    for bad in BAD_RULES:
        c = rule_of(bad).to_c()
        assert fn(C.byref(c), -29.0, 10, -3.0, FLOOR, out.ctypes.data) == capi.ERR_INVALID, bad
        assert out.tobytes() == before, bad
        with pytest.raises(capi.OmxError) as err:
            evaluate(omx, bad, -29.0, 10, -3.0)
        assert err.value.status == capi.ERR_INVALID
    good = rule_of(RULES[0]).to_c()
    assert fn(None, -29.0, 10, -3.0, FLOOR, out.ctypes.data) == capi.ERR_INVALID and out.tobytes() == before
    assert fn(C.byref(good), -29.0, 10, -3.0, FLOOR, None) == capi.ERR_INVALID
    assert fn(C.byref(good), -29.0, 10, -3.0, FLOOR, out.ctypes.data) == 0 and out.tobytes() != before
    assert fn(C.byref(rule_of(RULES[6]).to_c()), -29.0, 10, -3.0, FLOOR, out.ctypes.data) == 0      # a NaN ceiling that is not in use


# ---------------------------------------------------------------- the header
def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


C99_USE = r'''
#include <stddef.h>
#include "omx/program_normalize.h"
typedef char gain_record_is_32_bytes[sizeof(omx_program_gain_record) == 32 ? 1 : -1];
typedef char apply_record_is_32_bytes[sizeof(omx_program_apply_record) == 32 ? 1 : -1];
int main(void) {
    omx_program_gain_rule rule;
    rule.target_lufs = -23.0f; rule.true_peak_ceiling_db = -1.0f; rule.min_gain_db = -60.0f; rule.max_gain_db = 60.0f;
    rule.flags = OMX_GAIN_LIMIT_PEAK; rule._pad = 0;
    return (int)sizeof(rule) - 24 + (int)offsetof(omx_program_gain_record, limited_by) - 24 + (int)offsetof(omx_program_apply_record, gain) - 16
        + (int)offsetof(omx_program_apply_record, gain_index) - 28 + (OMX_PROGRAM_UNITY_GAIN == 4294967295u ? 0 : 1)
        + (int)(OMX_GAIN_BY_TARGET + OMX_GAIN_BY_PEAK + OMX_GAIN_BY_MAX_GAIN + OMX_GAIN_BY_MIN_GAIN + OMX_GAIN_BY_NO_MEASUREMENT) - 10
        + (int)rule.flags - 1;
}
'''
C11_ASSERTS = r'''
#include "omx/program_normalize.h"
_Static_assert(sizeof(omx_program_gain_record) == 32, "omx_program_gain_record is 32 bytes");
_Static_assert(sizeof(omx_program_apply_record) == 32, "omx_program_apply_record is 32 bytes");
_Static_assert(sizeof(omx_program_gain_rule) == 24, "omx_program_gain_rule is 24 bytes");
int main(void) { return 0; }
'''


def test_header_is_c99_its_structures_have_their_sizes_and_every_function_is_exported(tmp_path, omx):
    for name, text, std in (("use.c", C99_USE, "-std=c99"), ("asserts.c", C11_ASSERTS, "-std=c11")):
        src = tmp_path / name
        src.write_text(text)
        exe = tmp_path / name.replace(".c", "")
        subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       check=True, capture_output=True)
        assert subprocess.run([str(exe)]).returncode == 0, name
    import openmeters_amd
    assert C.sizeof(openmeters_amd.CProgramGainRecord) == 32 and C.sizeof(openmeters_amd.CProgramApplyRecord) == 32
    assert C.sizeof(openmeters_amd.CProgramGainRule) == 24
    assert openmeters_amd.GAIN_RECORD_DTYPE.itemsize == 32 and openmeters_amd.APPLY_RECORD_DTYPE.itemsize == 32
    assert openmeters_amd.GAIN_RECORD_DTYPE.names == nr.RECORD_FIELDS and openmeters_amd.UNITY_GAIN == nr.UNITY
    for dtype, struct in ((openmeters_amd.GAIN_RECORD_DTYPE, openmeters_amd.CProgramGainRecord),
                          (openmeters_amd.APPLY_RECORD_DTYPE, openmeters_amd.CProgramApplyRecord)):
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    syms = declared(os.path.join(INCLUDE, "program_normalize.h"))
    assert syms == ["omx_program_gain_evaluate", "omx_program_loudness_bank_apply_gains", "omx_program_loudness_bank_fetch_applied",
                    "omx_program_loudness_bank_fetch_gains", "omx_program_loudness_bank_plan_gains",
                    "omx_program_loudness_bank_plan_group_gains"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_normalize.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_normalize" not in open(os.path.join(ROOT, "include", "omx.h")).read()


def test_python_surface():
    from openmeters_amd.program_loudness import ProgramLoudnessBank
    for name in ("plan_gains", "plan_group_gains", "fetch_gains", "apply_gains", "fetch_applied"):
        assert callable(getattr(ProgramLoudnessBank, name)), name
    c = rule_of((-14.0, -1.0, -3.0, 9.0, nr.LIMIT_PEAK)).to_c()
    assert (c.target_lufs, c.true_peak_ceiling_db, c.min_gain_db, c.max_gain_db, c.flags, c._pad) == (-14.0, -1.0, -3.0, 9.0, 1, 0)


# ---------------------------------------------------------------- the restatement of the pass
def test_apply_restatement_counts_and_peaks():
    x = np.array([0.5, -0.75, np.nan, np.inf, -np.inf, 1e-40, -0.0, 1.0, -1.0], np.float32)
    out, over, peak = nr.apply(x, 2.0)
    assert over == 5 and np.isinf(peak)                       # -1.5, +inf, -inf, 2.0, -2.0; NaN is not counted
    assert out[5] == np.float32(1e-40) * np.float32(2.0) and out[5] != 0.0 and out[6].tobytes() == np.float32(-0.0).tobytes()
    out, over, peak = nr.apply(x[[0, 1, 2, 5, 6]], 1.0)
    assert over == 0 and peak == np.float32(0.75) and np.isnan(out[2])
    assert nr.apply(np.zeros((0,), np.float32), 3.0)[1:] == (0, np.float32(0.0))
    assert nr.apply(np.array([np.nan], np.float32), 3.0)[1:] == (0, np.float32(0.0))
    assert nr.peak_db(0.0, FLOOR) == FLOOR and abs(nr.peak_db(0.5, FLOOR) + 6.0206) < 1e-4 and nr.peak_db(np.inf, FLOOR) == np.inf
    p = nr.planted(nr.noise(1, 40, 3), 1)
    assert np.isnan(p).sum() == 1 and np.isinf(p).sum() == 2
    assert set(nr.APPLY_FRAMES) >= {0, 1, 3, 4, 5, 255, 256, 257, nr.APPLY_CAPACITY} and (nr.APPLY_CAPACITY * 3 * 4) % 16 and (nr.APPLY_CAPACITY * 5 * 4) % 16


# ---------------------------------------------------------------- known answers, from the restatements alone
@pytest.fixture(scope="module")
def known(oracle):
    xs = gr.known_programmes()
    coeffs = oracle.k_weighting_coefficients(ref.sanitize_rate(gr.KNOWN_RATE))
    pos = capi.positions_fallback(2)
    return xs, coeffs, pos, [ref.restate(x, gr.KNOWN_RATE, pos, coeffs, FLOOR) for x in xs]


COUNT_FIELDS = ("gating_above_absolute", "gating_above_relative", "short_term_above_absolute", "short_term_above_relative")


def test_known_track_gains_and_the_scaled_programmes_land_on_the_prediction(known):
    """stereo 1 kHz tones at -23, -29, -50, -20, -30 dBFS to -23 LUFS: 0, +6, +27, -3, +7 dB.  Scaled in numpy by the gain and
    restated, every programme lands on predicted_lufs within 1e-4 LU with the gate counts it had and the gate margin the comparison
    needs, before and after: the proof that the inputs of the GPU round trip are fair"""
    xs, coeffs, pos, before = known
    worst = 0.0
    for s, (x, src) in enumerate(zip(xs, before)):
        assert src["gate_margin"] >= ref.GATE_MARGIN_MIN, (s, src["gate_margin"])
        r = nr.gain(nr.RULE_TARGET, src["integrated_lufs"], src["gating_above_relative"], FLOOR, FLOOR)
        assert r["limited_by"] == nr.BY_TARGET and r["peak_known"] == 0
        assert abs(float(r["gain_db"]) - nr.KNOWN_TRACK_GAINS_DB[s]) <= 0.1, (s, r["gain_db"])
        out, _, _ = nr.apply(x, r["gain"])
        after = ref.restate(out, gr.KNOWN_RATE, pos, coeffs, FLOOR)
        d = abs(float(after["integrated_lufs"]) - float(r["predicted_lufs"]))
        worst = max(worst, d)
        assert d <= LUFS_BAR and abs(float(after["integrated_lufs"]) + 23.0) <= LUFS_BAR, (s, after["integrated_lufs"], r["predicted_lufs"])
        for f in COUNT_FIELDS:
            assert after[f] == src[f], (s, f, after[f], src[f])
        assert after["gate_margin"] >= ref.GATE_MARGIN_MIN, (s, after["gate_margin"])
    print(f"known programmes: scaled and restated at most {worst:.2e} LU from the prediction")


def test_known_album_gain_and_the_scaled_album_lands_on_the_prediction(known):
    xs, coeffs, pos, before = known
    es = [b["e"] for b in before]
    members = gr.KNOWN_MEMBERS[:2]
    album = gr.results(es, members, 4800, FLOOR)
    r = nr.gain(nr.RULE_TARGET, album["integrated_lufs"], album["gating_above_relative"], FLOOR, FLOOR)
    assert abs(float(r["gain_db"]) - (-23.0 - gr.KNOWN_ALBUM_LUFS)) <= 0.1 and abs(float(r["gain_db"]) - 2.04) <= 0.1, r["gain_db"]
    scaled = [ref.restate(nr.apply(xs[s], r["gain"])[0], gr.KNOWN_RATE, pos, coeffs, FLOOR)["e"] for s in (0, 1)]
    after = gr.results(scaled, [(0, 0, gr.TO_END), (1, 0, gr.TO_END)], 4800, FLOOR)
    assert abs(float(after["integrated_lufs"]) - float(r["predicted_lufs"])) <= LUFS_BAR and abs(float(after["integrated_lufs"]) + 23.0) <= LUFS_BAR
    for f in COUNT_FIELDS:
        assert after[f] == album[f], f
    assert album["gate_margin"] >= ref.GATE_MARGIN_MIN and after["gate_margin"] >= ref.GATE_MARGIN_MIN


def test_shared_rules_bind_where_the_gpu_file_says(known):
    """with the tones' true peaks at their levels (within 0.01 dB: the GPU file reads the measured ones), RULE_CEILING is peak-limited
    on every stream and RULE_CLAMPS crosses both clamps and the override"""
    _, _, _, before = known
    peaks = [float(db) for db in gr.KNOWN_LEVELS_DBFS]
    by = [nr.gain(nr.RULE_CEILING, b["integrated_lufs"], b["gating_above_relative"], p, FLOOR)["limited_by"] for b, p in zip(before, peaks)]
    assert by == [nr.BY_PEAK] * 5, by
    recs = [nr.gain(nr.RULE_CLAMPS, b["integrated_lufs"], b["gating_above_relative"], p, FLOOR) for b, p in zip(before, peaks)]
    assert [r["limited_by"] for r in recs] == [nr.BY_MIN_GAIN, nr.BY_PEAK, nr.BY_MAX_GAIN, nr.BY_MIN_GAIN, nr.BY_MAX_GAIN], [r["limited_by"] for r in recs]
    assert float(recs[3]["predicted_peak_db"]) > -25.0        # the minimum clamp overrode the peak limit

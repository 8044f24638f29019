"""Programme bank convolve stage (include/omx/program_convolve.h), CPU side: the numpy restatement (tests/program_convolve_ref.py)
pinned by a hand-written case and by the order and width cases; its streaming rule (any cut of a programme gives the bytes of the
whole); the header as C99, its structures' sizes and offsets, the exported functions, the Python surface; plan, frames, check, design
and response against the restatement, and every refusal of the host-only functions with the output buffers still holding their
sentinels.

Bars.  Everything is equal on bits except:
  - the design against the restatement: libm and numpy may round sin differently, nothing else differs.  Measured here over DESIGNS:
    the largest |library tap - restated tap| is 0.0 (every tap equal on bits on this libm and this numpy), so the bar is
    DESIGN_MEASURED = 0 plus one f32 ulp of the design's largest tap: what another libm's sine can move a tap that lies at a
    rounding boundary.  The test prints what it measures.  Every other test (and every GPU test) feeds the restatement the LIBRARY's
    taps, so none rests on this bar;
  - response against an FFT of the taps: 1e-9 dB at -80 dB and above."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import program_convolve_ref as cr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")
FS = 48000.0
#           kind, taps, f_lo, f_hi, beta
DESIGNS = [(cr.LOWPASS, 3, 0.0, 6000.0, 0.0), (cr.LOWPASS, 15, 0.0, 12000.0, 4.0), (cr.LOWPASS, 255, 0.0, 8000.0, 9.0),
           (cr.LOWPASS, 4095, 0.0, 20000.0, 12.0), (cr.LOWPASS, 1023, 0.0, 40.0, 20.0), (cr.HIGHPASS, 63, 300.0, 0.0, 6.0),
           (cr.HIGHPASS, 511, 20.0, 0.0, 9.0), (cr.BANDPASS, 255, 300.0, 3400.0, 9.0), (cr.BANDPASS, 1025, 997.0, 1003.0, 7.5),
           (cr.BANDSTOP, 127, 45.0, 55.0, 5.0), (cr.BANDSTOP, 2047, 1000.0, 23999.0, 10.0)]
DESIGN_MEASURED = 0.0      # the largest |library - restatement| over DESIGNS, measured on the CPU (the module's docstring)


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def last_error(omx):
    return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")


def bits(v):
    return int(np.float32(v).view(np.uint32))


def spec_of(kind, taps, f_lo, f_hi, beta):
    import openmeters_amd as oa
    return oa.ConvolveSpec(kind, taps, f_lo, f_hi, beta)


# ---------------------------------------------------------------- the restatement, by hand
def test_restatement_gives_the_hand_written_output():
    """Taps (0.5, -1, 0.25) on x = (1, 2, -0.5, 4, 0.25), D = 1, flushed: out[m] = 0.5 x[m+1] - x[m] + 0.25 x[m-1].  Every figure is a
    small dyadic number, so every figure below is exact.  A second channel is bypassed and comes out as it went in, aligned."""
    h = np.array([0.5, -1.0, 0.25], np.float32)
    x = np.array([1.0, 2.0, -0.5, 4.0, 0.25], np.float32)
    want = np.array([0.5 * 2 - 1,                      # m = 0: x[1], x[0], 0
                     0.5 * -0.5 - 2 + 0.25 * 1,        # m = 1
                     0.5 * 4 + 0.5 + 0.25 * 2,         # m = 2
                     0.5 * 0.25 - 4 + 0.25 * -0.5,     # m = 3
                     0.5 * 0 - 0.25 + 0.25 * 4], np.float32)      # m = 4: the zero behind the flush
    assert want.tolist() == [0.0, -2.0, 3.0, -4.0, 0.75]
    st = cr.Stream([h, None], 1, floor=-99.9)
    y = st.feed(np.stack([x, x], axis=1), flush=True)
    assert y[:, 0].tobytes() == want.tobytes() and y[:, 1].tobytes() == x.tobytes(), y
    rec = st.record()
    assert {f: int(rec[f]) for f in ("frames_in", "frames_out", "frames_written", "samples_over", "samples_nonfinite", "state",
                                     "delay_frames", "max_taps")} == {"frames_in": 5, "frames_out": 5, "frames_written": 5,
                                                                      "samples_over": 3 + 2, "samples_nonfinite": 0, "state": cr.FLUSHED,
                                                                      "delay_frames": 1, "max_taps": 3}
    assert float(rec["out_sample_peak"]) == 4.0 and abs(rec["out_sample_peak_db"] - 20 * np.log10(4.0)) <= 1e-4
    # D = 0 is the causal FIR and a flush emits nothing; D = T - 1 is the anti-causal end
    assert cr.convolve([h], 0, x[:, None])[:, 0].tolist() == [0.5, 0.0, -2.0, 3.0, -4.0]
    assert cr.convolve([h], 2, x[:, None])[:, 0].tolist() == [-2.0, 3.0, -4.0, 0.75, 0.0625]


def test_restatement_is_pinned_on_the_order_and_width_cases():
    def fir(taps, xs=None, delay=None):
        taps = np.array(taps, np.float32)
        x = np.ones(len(taps), np.float32) if xs is None else np.array(xs, np.float32)
        y = cr.convolve([taps], 0, x[:, None])
        return bits(y[len(taps) - 1 if delay is None else delay, 0])      # the frame that reads every tap

    assert fir([2.0 ** 60, 1.0, -2.0 ** 60]) == bits(0.0)          # the table's order: (2^60 + 1) rounds to 2^60 in f64
    assert fir([2.0 ** 60, -2.0 ** 60, 1.0]) == bits(1.0)          # the other order
    assert fir([2.0 ** 30, 1.0, -2.0 ** 30]) == bits(1.0)          # an f32 accumulator would give 0.0
    assert np.float32(np.float32(2.0 ** 30) + np.float32(1.0)) - np.float32(2.0 ** 30) == 0.0
    assert fir([1.0] + [2.0 ** -25] * 4) == 0x3F800001             # f32 accumulation stays at 0x3f800000
    acc = np.float32(1.0)
    for _ in range(4):
        acc = np.float32(acc + np.float32(2.0 ** -25))
    assert bits(acc) == 0x3F800000
    # the rounding to f32 is to nearest EVEN and produces denormals
    assert fir([1.0, 2.0 ** -24]) == 0x3F800000 and fir([1.0, 2.0 ** -24, 2.0 ** -24]) == 0x3F800001
    assert fir([1.0, 2.0 ** -23, 2.0 ** -24]) == 0x3F800002      # a tie: up to the even neighbour
    assert fir([2.0 ** -126, -2.0 ** -127]) == 0x00400000          # a denormal comes out
    assert fir([2.0 ** -49], [2.0 ** -100]) == 0x00000001          # the smallest denormal, from one product
    assert fir([2.0 ** -50, 2.0 ** -50], [2.0 ** -100, 2.0 ** -100]) == 0x00000001      # two products of 2^-150 sum to 2^-149
    assert fir([2.0 ** -49, 2.0 ** -50], [2.0 ** -100, 2.0 ** -100]) == 0x00000002      # 1.5 * 2^-149: a tie, up to the even 2
    assert fir([2.0 ** -50], [2.0 ** -100]) == 0x00000000          # 2^-150: a tie between 0 and the odd 1, down to the even 0
    # every tap takes part: an infinity under a zero tap is a NaN; -0.0 keeps its sign under ONE tap only
    assert np.isnan(np.uint32(fir([1.0, 0.0], [np.inf, 1.0])).view(np.float32))
    assert fir([1.0], [-0.0]) == 0x80000000
    y = cr.convolve([np.array([0.0, 1.0], np.float32)], 1, np.array([[-0.0], [3.0]], np.float32))
    assert bits(y[0, 0]) == 0x00000000 and bits(y[1, 0]) == bits(3.0)      # 0 * 3 + 1 * -0.0 = +0.0: the impulse at k = D loses the sign
    z = cr.Stream([None], 1, max_taps=2).feed(np.array([[-0.0], [3.0]], np.float32), flush=True)
    assert bits(z[0, 0]) == 0x80000000                                       # the bypass keeps it
    # a bypass keeps NaN payloads
    nan = np.array([0x7FC12345, 0xFF800001], np.uint32).view(np.float32)
    assert cr.convolve([None], 0, nan[:, None]).tobytes() == nan.tobytes()


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("taps", [1, 2, 5, 16])
def test_any_cut_of_a_programme_gives_the_bytes_of_the_whole(taps):
    """calls of 0 frames and of fewer than T - 1 frames, D in {0, 1, (T-1)/2, T-1}, the flush in the last call or in one of its own,
    a second channel with a shorter FIR and a bypassed third; a reset starts the stream over"""
    n, ch = 61, 3
    x = cr.noise(taps, n, ch)
    x[7, 0], x[20, 1], x[33, 2], x[40, 0] = np.inf, np.nan, -0.0, -np.inf
    firs = [cr.random_taps(taps, taps), cr.random_taps(taps + 50, max(1, taps // 2)), None]
    for delay in sorted({0, min(1, taps - 1), (taps - 1) // 2, taps - 1}):
        whole = cr.Stream(firs, delay)
        want = whole.feed(x, flush=True)
        assert want.shape == (n, ch)
        for cuts, own_flush in (([n], True), ([0, 1, 0, 2, taps, 0, 3], False), ([1] * 9 + [30], True), ([29, 0, 31], False)):
            st = cr.Stream(firs, delay)
            if sum(cuts) != n:
                cuts = cuts + [n - sum(cuts)]
            out, at = [], 0
            for i, f in enumerate(cuts):
                before = (st.n, st.e)
                last = i == len(cuts) - 1
                out.append(st.feed(x[at:at + f], flush=last and not own_flush))
                at += f
                assert len(out[-1]) == cr.emitted(delay, before[0] + f, before[1], last and not own_flush) - before[1]
                if delay == 0:
                    assert len(out[-1]) == f
            if own_flush:
                out.append(st.feed(x[:0], flush=True))
                assert len(out[-1]) == min(delay, n)
            got = np.concatenate(out)
            cr.same_floats(got, want, (taps, delay, cuts))
            assert got[:, 2].tobytes() == x[:, 2].tobytes()      # the bypass, aligned and on bits
            a, b = st.record(), whole.record()
            a["frames_written"] = b["frames_written"] = 0
            assert {k: (float(v) if k.startswith("out") else int(v)) for k, v in a.items()} == \
                {k: (float(v) if k.startswith("out") else int(v)) for k, v in b.items()}
            st.reset()
            assert st.record()["state"] == cr.IDLE and st.record()["frames_in"] == 0
            cr.same_floats(st.feed(x, flush=True), want, (taps, delay, "after a reset"))


def test_frames_is_the_streaming_formula(omx):
    import openmeters_amd as oa
    for delay in (0, 1, 7, 4095):
        n = e = 0
        for f, flush in ((0, False), (1, False), (5, False), (3, False), (5000, False), (0, False), (2, True), (0, True)):
            got = oa.convolve_frames(omx, delay, n, e, f, flush)
            want = cr.emitted(delay, n + f, e, flush) - e
            assert got == want, (delay, n, e, f, flush)
            n, e = n + f, e + got
        assert e == n
    fn = omx.fn("program_convolve_frames", C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p])
    out = np.full((1,), 0xABABABABABABABAB, np.uint64)
    for args in ((4096, 0, 0, 1, 0), (1, 2 ** 63 + 1, 0, 0, 0), (1, 2 ** 62, 0, 2 ** 63, 0), (1, 5, 6, 1, 0)):
        assert fn(*args, out.ctypes.data) == capi.ERR_INVALID and out[0] == 0xABABABABABABABAB, args
        assert last_error(omx).startswith("program loudness convolve frames: ")
    assert fn(1, 0, 0, 1, 0, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- the header
C99_USE = r'''
#include <stddef.h>
#include "omx/program_convolve.h"
typedef char fir_is_16_bytes[sizeof(omx_program_fir) == 16 ? 1 : -1];
typedef char spec_is_32_bytes[sizeof(omx_program_convolve_spec) == 32 ? 1 : -1];
typedef char info_is_16_bytes[sizeof(omx_program_convolve_info) == 16 ? 1 : -1];
typedef char record_is_64_bytes[sizeof(omx_program_convolve_record) == 64 ? 1 : -1];
int main(void) {
    return (int)offsetof(omx_program_fir, n_taps) - 8 + (int)offsetof(omx_program_fir, flags) - 12
        + (int)offsetof(omx_program_convolve_spec, n_taps) - 4 + (int)offsetof(omx_program_convolve_spec, f_lo_hz) - 8
        + (int)offsetof(omx_program_convolve_spec, f_hi_hz) - 16 + (int)offsetof(omx_program_convolve_spec, beta) - 24
        + (int)offsetof(omx_program_convolve_info, frames_per_thread) - 4 + (int)offsetof(omx_program_convolve_info, tap_block) - 8
        + (int)offsetof(omx_program_convolve_info, channels) - 12
        + (int)offsetof(omx_program_convolve_record, frames_written) - 16 + (int)offsetof(omx_program_convolve_record, samples_nonfinite) - 32
        + (int)offsetof(omx_program_convolve_record, out_sample_peak) - 40 + (int)offsetof(omx_program_convolve_record, state) - 48
        + (int)offsetof(omx_program_convolve_record, delay_frames) - 52 + (int)offsetof(omx_program_convolve_record, max_taps) - 56
        + (int)(OMX_CONVOLVE_MAX_TAPS - 4096u) + (int)(OMX_CONVOLVE_MAX_FIRS - 64u) + (OMX_CONVOLVE_BYPASS == 0xFFFFFFFFu ? 0 : 1)
        + (int)(OMX_CONVOLVE_LOWPASS + OMX_CONVOLVE_HIGHPASS + OMX_CONVOLVE_BANDPASS + OMX_CONVOLVE_BANDSTOP - 6u)
        + (int)(OMX_CONVOLVE_IDLE + OMX_CONVOLVE_RUNNING + OMX_CONVOLVE_FLUSHED - 3u);
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
    header = open(os.path.join(INCLUDE, "program_convolve.h")).read()
    assert '#include "program_mix.h"' in header
    sizes = {"omx_program_fir": (oa.CProgramFir, 16), "omx_program_convolve_spec": (oa.CProgramConvolveSpec, 32),
             "omx_program_convolve_info": (oa.CProgramConvolveInfo, 16), "omx_program_convolve_record": (oa.CProgramConvolveRecord, 64)}
    for name, (struct, size) in sizes.items():
        assert C.sizeof(struct) == size
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), (name, "the header's comment does not give this size")
    for dtype, struct in ((oa.CONVOLVE_RECORD_DTYPE, oa.CProgramConvolveRecord), (oa.CONVOLVE_INFO_DTYPE, oa.CProgramConvolveInfo)):
        assert dtype.itemsize == C.sizeof(struct)
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [f for f in oa.CONVOLVE_RECORD_DTYPE.names if f != "_pad"] == list(cr.RECORD_FIELDS)
    assert [getattr(oa.CProgramConvolveRecord, f).offset for f in oa.CONVOLVE_RECORD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    syms = declared(os.path.join(INCLUDE, "program_convolve.h"))
    assert syms == ["omx_program_convolve_check", "omx_program_convolve_design", "omx_program_convolve_frames", "omx_program_convolve_plan",
                    "omx_program_convolve_response", "omx_program_loudness_bank_convolve", "omx_program_loudness_bank_convolve_configure",
                    "omx_program_loudness_bank_convolve_reset", "omx_program_loudness_bank_fetch_convolved"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_convolve.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h or in an earlier header
    assert "program_convolve" not in open(os.path.join(ROOT, "include", "omx.h")).read()
    assert "convolve" not in open(os.path.join(INCLUDE, "program_mix.h")).read()
    for name in ("ConvolveSpec", "CONVOLVE_RECORD_DTYPE", "CONVOLVE_INFO_DTYPE", "convolve_plan", "convolve_design", "convolve_check",
                 "convolve_response", "convolve_frames", "CONVOLVE_BYPASS"):
        assert hasattr(oa, name), name
    assert (oa.CONVOLVE_MAX_TAPS, oa.CONVOLVE_MAX_FIRS, oa.CONVOLVE_BYPASS) == (cr.MAX_TAPS, cr.MAX_FIRS, cr.BYPASS)
    assert (oa.CONVOLVE_LOWPASS, oa.CONVOLVE_HIGHPASS, oa.CONVOLVE_BANDPASS, oa.CONVOLVE_BANDSTOP) == (0, 1, 2, 3)
    assert (oa.CONVOLVE_IDLE, oa.CONVOLVE_RUNNING, oa.CONVOLVE_FLUSHED) == (cr.IDLE, cr.RUNNING, cr.FLUSHED)
    for name in ("configure_convolve", "convolve", "reset_convolve", "fetch_convolved"):
        assert hasattr(oa.ProgramLoudnessBank, name), name


def build_demo(tmp_path):
    """tests/c_abi/program_convolve_demo.c: a plain C99 host that designs a low-pass, prints its response and filters an impulse"""
    out = str(tmp_path / "program_convolve_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_convolve_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


def test_plan(omx):
    import openmeters_amd as oa
    plan = omx.fn("program_convolve_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p])
    for ch in range(1, 9):
        for max_taps in (1, 255, 4096):
            info = oa.convolve_plan(omx, ch, max_taps)
            t, r, kb = int(info["tile_frames"]), int(info["frames_per_thread"]), int(info["tap_block"])
            assert int(info["channels"]) == ch and r >= 2 and t % (64 * r) == 0 and kb % r == 0 and kb >= 2 * r
            assert 2 * kb + 1 <= cr.MAX_TAPS      # the GPU tests' tap counts KB - 1 .. 2 KB + 1 are allowed
            assert (ch * (t + kb) * 4) <= 64 * 1024      # the staging of a tile and a tap block: 4096 taps need no more LDS than 256
    for ch, max_taps in ((0, 1), (9, 1), (2, 0), (2, 4097), (2 ** 32 - 1, 2 ** 32 - 1)):
        buf = np.full((16,), 0xAB, np.uint8)
        assert plan(ch, max_taps, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), (ch, max_taps)
        assert last_error(omx).startswith("program loudness convolve plan: ")
    assert plan(2, 1, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- check, design, response
def test_check_takes_what_the_bank_takes_and_refuses_the_rest(omx):
    import openmeters_amd as oa
    check = omx.fn("program_convolve_check", C.c_int, [C.c_void_p])
    assert oa.convolve_check(omx, [1.0]) == 0 and oa.convolve_check(omx, np.zeros(4096, np.float32)) == 0
    assert oa.convolve_check(omx, [1e-45, -3.4e38, 0.0, -0.0]) == 0
    taps = np.ones(8, np.float32)
    for bad in (oa.CProgramFir(None, 8, 0), oa.CProgramFir(taps.ctypes.data, 0, 0), oa.CProgramFir(taps.ctypes.data, 4097, 0),
                oa.CProgramFir(taps.ctypes.data, 8, 1)):
        assert check(C.byref(bad)) == capi.ERR_INVALID
        assert last_error(omx).startswith("program loudness convolve check: ")
    assert check(None) == capi.ERR_INVALID
    for v in (np.nan, np.inf, -np.inf):
        t = taps.copy()
        t[5] = v
        with pytest.raises(capi.OmxError):
            oa.convolve_check(omx, t)


def test_design_against_the_restatement(omx):
    """the module's docstring gives the bar and what was measured"""
    import openmeters_amd as oa
    worst = 0.0
    for kind, T, f_lo, f_hi, beta in DESIGNS:
        h = oa.convolve_design(omx, spec_of(kind, T, f_lo, f_hi, beta), FS)
        want = cr.design(kind, T, FS, f_lo, f_hi, beta)
        assert h.dtype == np.float32 and h.shape == (T,) and np.isfinite(h).all()
        assert h.tobytes() == h[::-1].tobytes(), "h[k] == h[T-1-k] on bits"
        diff = float(np.abs(h.astype(np.float64) - want.astype(np.float64)).max())
        ulp = float(np.spacing(np.abs(h).max()))
        print(f"convolve design kind {kind} T {T}: max |library - restatement| = {diff:.3e}, one ulp of the largest tap {ulp:.3e}")
        worst = max(worst, diff)
        assert diff <= DESIGN_MEASURED + ulp, (kind, T, diff)
        total = float(np.sum(h.astype(np.float64)))
        bar = T * 2.0 ** -24
        if kind in (cr.LOWPASS, cr.BANDSTOP):
            assert abs(total - 1.0) <= bar, (kind, T, total)
        else:
            assert abs(total) <= bar, (kind, T, total)
        assert oa.convolve_check(omx, h) == 0
    print(f"convolve design: the largest difference over DESIGNS is {worst:.3e}")


def test_design_refuses_and_writes_nothing(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_convolve_design", C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_uint32])
    good = dict(kind=cr.BANDPASS, n_taps=31, f_lo_hz=300.0, f_hi_hz=3400.0, beta=8.0)
    bad = [dict(n_taps=30), dict(n_taps=1), dict(n_taps=4097), dict(n_taps=4096), dict(kind=4), dict(f_lo_hz=0.0), dict(f_lo_hz=-1.0),
           dict(f_hi_hz=24000.0), dict(f_hi_hz=np.nan), dict(f_lo_hz=np.inf), dict(f_lo_hz=3400.0), dict(f_lo_hz=5000.0), dict(beta=-0.5),
           dict(beta=20.5), dict(beta=np.nan), dict(kind=cr.LOWPASS, f_hi_hz=0.0), dict(kind=cr.HIGHPASS, f_lo_hz=24000.0)]
    for change in bad:
        spec = oa.ConvolveSpec(**{**good, **change}).to_c()
        buf = np.full((4100,), 777.25, np.float32)
        assert fn(C.byref(spec), FS, buf.ctypes.data, spec.n_taps) == capi.ERR_INVALID and (buf == 777.25).all(), change
        assert last_error(omx).startswith("program loudness convolve design: "), change
    spec = oa.ConvolveSpec(**good).to_c()
    buf = np.full((64,), 777.25, np.float32)
    for fs, n in ((FS, 30), (FS, 32), (0.0, 31), (-1.0, 31), (np.nan, 31), (np.inf, 31)):
        assert fn(C.byref(spec), fs, buf.ctypes.data, n) == capi.ERR_INVALID and (buf == 777.25).all(), (fs, n)
    assert fn(None, FS, buf.ctypes.data, 31) == capi.ERR_INVALID and fn(C.byref(spec), FS, None, 31) == capi.ERR_INVALID
    # a frequency the kind does not use is not looked at
    assert oa.convolve_design(omx, oa.ConvolveSpec(cr.LOWPASS, 31, np.nan, 1000.0, 8.0), FS).shape == (31,)
    assert oa.convolve_design(omx, oa.ConvolveSpec(cr.HIGHPASS, 31, 1000.0, -5.0, 8.0), FS).shape == (31,)


def test_response_agrees_with_an_fft_of_the_taps(omx):
    import openmeters_amd as oa
    n_fft, total = 1 << 15, 0
    for kind, T, f_lo, f_hi, beta in DESIGNS:
        h = oa.convolve_design(omx, spec_of(kind, T, f_lo, f_hi, beta), FS)
        spectrum = np.fft.rfft(h.astype(np.float64), n_fft)
        checked = 0      # (bins at -80 dB and above: the 6 Hz band-pass has one among these)
        for b in (0, 1, 17, 683, 2048, 5461, 8192, 13653, 16000, n_fft // 2):
            hz = b * FS / n_fft
            mag, ph = oa.convolve_response(omx, h, FS, hz)
            want_mag, want_ph = cr.response(h, FS, hz)
            assert (mag == want_mag or abs(mag - want_mag) <= 1e-9 or want_mag < -250) and (abs(ph - want_ph) <= 1e-6 or want_mag < -120)
            with np.errstate(divide="ignore"):
                fft_db = 20.0 * np.log10(np.abs(spectrum[b]))
            if fft_db >= -80.0:
                assert abs(mag - fft_db) <= 1e-9, (kind, T, hz, mag, fft_db)
                checked += 1
        assert checked >= 1, (kind, T)
        total += checked
    assert total >= 40, total
    # linear phase: a symmetric FIR's phase at a passband frequency is -w (T - 1) / 2, folded into (-pi, pi]
    h = oa.convolve_design(omx, spec_of(cr.LOWPASS, 255, 0.0, 8000.0, 9.0), FS)
    mag, ph = oa.convolve_response(omx, h, FS, 1000.0)
    want = -2.0 * np.pi * 1000.0 / FS * 127.0
    assert abs(mag) <= 1e-3 and abs(np.angle(np.exp(1j * (ph - want)))) <= 1e-9
    # refusals leave the outputs alone
    fn = omx.fn("program_convolve_response", C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p])
    fir = oa.CProgramFir(h.ctypes.data, h.size, 0)
    for fs, hz in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (FS, -1.0), (FS, np.inf), (np.inf, 1.0)):
        out = np.full((2,), 777.25, np.float64)
        assert fn(C.byref(fir), fs, hz, out.ctypes.data, out.ctypes.data + 8) == capi.ERR_INVALID and (out == 777.25).all(), (fs, hz)
        assert last_error(omx).startswith("program loudness convolve response: ")
    out = np.full((2,), 777.25, np.float64)
    for bad in (oa.CProgramFir(None, 8, 0), oa.CProgramFir(h.ctypes.data, 0, 0), oa.CProgramFir(h.ctypes.data, 8, 2)):
        assert fn(C.byref(bad), FS, 1.0, out.ctypes.data, out.ctypes.data + 8) == capi.ERR_INVALID and (out == 777.25).all()
    assert fn(None, FS, 1.0, out.ctypes.data, out.ctypes.data + 8) == capi.ERR_INVALID
    assert fn(C.byref(fir), FS, 1.0, None, None) == 0      # either result pointer may be null


def test_bank_calls_before_configure_and_with_null_handles_are_refused(omx):
    """what needs no device: a null bank is refused by every bank function of the header"""
    rec = np.zeros((64,), np.uint8)
    assert omx.fn("program_loudness_bank_convolve_configure", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])(
        None, 2, None, 1, None, 0) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_convolve_reset", C.c_int, [C.c_void_p, C.c_void_p])(None, None) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_fetch_convolved", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])(None, 0, rec.ctypes.data) == capi.ERR_INVALID
    assert omx.fn("program_loudness_bank_convolve", C.c_int,
                  [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p])(
        None, None, 0, None, None, 0, None, None, None) == capi.ERR_INVALID

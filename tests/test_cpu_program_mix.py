"""Programme bank mix pass (include/omx/program_mix.h), CPU side: the numpy restatement (tests/program_mix_ref.py) pinned by a
hand-written case and by the order and width cases; the header as C99, its structures' sizes and offsets, the exported functions, the
Python surface; extent, plan and mix_null against the restatement, and every refusal of the host-only functions with the output
buffers still holding their sentinels.

Bars.  Everything is equal on bits but out_sample_peak_db, which lies within the family's 1e-4 dB."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import program_mix_ref as mr
from openmeters_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include", "omx")


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(omx_[a-z0-9_]+)\s*\(", text)))


def last_error(omx):
    return omx.fn("last_error", C.c_char_p, [])().decode("utf-8", "replace")


def bits(v):
    return int(np.float32(v).view(np.uint32))


# ---------------------------------------------------------------- the restatement, by hand
def test_restatement_gives_the_hand_written_output_of_three_sends():
    """Two stereo sources of 6 and 4 frames.  Send A: source 0 frames 1 .. 4 at bus frame 2, gain 0.5.  Send B: source 1 frames
    0 .. 3 at bus frame 3, gain -1 (polarity inverted).  Send C: source 0 frames 0 .. 1 at bus frame 4, gain 2.  Bus frames 0 1 are
    under nothing, 2 under A, 3 under A B, 4 5 under A B C, 6 under B, 7 under nothing.  Every sample is a small dyadic number, so
    every figure below is exact."""
    s0 = np.array([(1.0, -1.0), (0.5, 0.25), (-0.25, 2.0), (0.75, -0.0), (0.25, 0.5), (9.0, 9.0)], np.float32)
    s1 = np.array([(0.125, 1.0), (1.0, -0.5), (3.0, 0.25), (-0.5, -0.0)], np.float32)
    a = mr.Send(0, 0, 1, 2, 4, 0.5)
    b = mr.Send(1, 0, 0, 3, 4, -1.0)
    c = mr.Send(0, 0, 0, 4, 2, 2.0)
    want = np.array([(0.0, 0.0), (0.0, 0.0),
                     (0.25, 0.125),                                              # A: 0.5 * (0.5, 0.25)
                     (-0.125 - 0.125, 1.0 - 1.0),                                # A + B: 0.5 * (-0.25, 2) - (0.125, 1)
                     (0.375 - 1.0 + 2.0, -0.0 + 0.5 - 2.0),                      # A + B + C: 0.5 * (0.75, -0) - (1, -0.5) + 2 * (1, -1)
                     (0.125 - 3.0 + 1.0, 0.25 - 0.25 + 0.5),                     # 0.5 * (0.25, 0.5) - (3, 0.25) + 2 * (0.5, 0.25)
                     (0.5, 0.0),                                                 # B: -(-0.5, -0)
                     (0.0, 0.0)], np.float32)
    (y,), (rec,) = mr.render([s0, s1], [a, b, c], [8], 2)
    assert y.tobytes() == want.tobytes(), (y, want)
    assert not np.signbit(y[[0, 1, 7]]).any() and not np.signbit(y[3, 1]) and not np.signbit(y[6, 1])      # 1 - 1 and -(-0) are +0
    fields = {"out_first": 0, "frames": 8, "silent_frames": 3, "mixed_frames": 3, "samples_over": 3, "samples_nonfinite": 0, "sends": 3,
              "max_layers": 3}
    assert {f: int(rec[f]) for f in fields} == fields
    assert float(rec["out_sample_peak"]) == 1.875 and abs(float(rec["out_sample_peak_db"]) - 20 * np.log10(1.875)) <= 1e-4
    # the same frames through windows: pieces of the whole, counts that add up, maxima that are maxima
    parts = [mr.render([s0, s1], [a, b, c], [n], 2, out_first=[f]) for f, n in ((0, 3), (3, 2), (5, 3))]
    assert b"".join(p[0][0].tobytes() for p in parts) == y.tobytes()
    for f in mr.COUNT_FIELDS:
        assert sum(int(p[1][0][f]) for p in parts) == int(rec[f]), f
    assert [int(p[1][0]["sends"]) for p in parts] == [1, 3, 3] and [int(p[1][0]["max_layers"]) for p in parts] == [1, 3, 3]
    # one send of gain 1 keeps the bits of -0.0, a denormal and the infinities
    hard = np.array([[-0.0], [1e-45], [-1e-40], [np.inf], [-np.inf], [3.0]], np.float32)
    (y,), (rec,) = mr.render([hard], [mr.Send(frames=6, dst_first=1)], [8], 1)
    assert y[1:7].tobytes() == hard.tobytes() and y[0].tobytes() == y[7].tobytes() == np.float32(0).tobytes()
    assert int(rec["samples_nonfinite"]) == 2 and int(rec["samples_over"]) == 3 and np.isinf(rec["out_sample_peak"])


def test_restatement_is_pinned_on_the_order_and_width_cases():
    def mix_of(samples, gains=None):
        xs = [np.array([[v]], np.float32) for v in samples]
        sends = [mr.Send(i, 0, 0, 0, 1, 1.0 if gains is None else gains[i]) for i in range(len(xs))]
        (y,), _ = mr.render(xs, sends, [1], 1)
        return bits(y[0, 0])

    assert mix_of([2.0 ** 60, 1.0, -2.0 ** 60]) == bits(0.0)          # the table's order: (2^60 + 1) rounds to 2^60 in f64
    assert mix_of([2.0 ** 60, -2.0 ** 60, 1.0]) == bits(1.0)          # the other order
    assert mix_of([2.0 ** 30, 1.0, -2.0 ** 30]) == bits(1.0)          # an f32 accumulator would give 0.0
    assert np.float32(np.float32(2.0 ** 30) + np.float32(1.0)) - np.float32(2.0 ** 30) == 0.0
    assert mix_of([1.0] + [2.0 ** -25] * 4) == 0x3F800001             # f32 accumulation stays at 0x3f800000
    acc = np.float32(1.0)
    for _ in range(4):
        acc = np.float32(acc + np.float32(2.0 ** -25))
    assert bits(acc) == 0x3F800000
    # a negative gain inverts polarity; the rounding to f32 is to nearest EVEN and produces denormals
    assert mix_of([0.75], [-1.0]) == bits(-0.75)
    assert mix_of([1.0, 2.0 ** -24]) == 0x3F800000 and mix_of([1.0, 2.0 ** -24, 2.0 ** -24]) == 0x3F800001
    assert mix_of([1.0, 2.0 ** -23, 2.0 ** -24]) == 0x3F800002      # a tie: up to the even neighbour
    assert mix_of([2.0 ** -126, -2.0 ** -127]) == 0x00400000          # a denormal comes out
    assert mix_of([2.0 ** -100], [2.0 ** -49]) == 0x00000001          # the smallest denormal, from one product
    assert mix_of([2.0 ** -100, 2.0 ** -100], [2.0 ** -50, 2.0 ** -50]) == 0x00000001      # two products of 2^-150, each below f32, sum to 2^-149


def test_products_of_two_floats_are_exact_in_double():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 2 ** 32, 40000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    raw = raw[np.isfinite(raw)][:20000]
    g, x = raw[:len(raw) // 2], raw[len(raw) // 2:2 * (len(raw) // 2)]
    prod = g.astype(np.float64) * x.astype(np.float64)
    for i in range(0, len(g), 10):      # rational arithmetic on a tenth of them, every exponent among them
        assert Fraction(float(prod[i])) == Fraction(float(g[i])) * Fraction(float(x[i])), (g[i], x[i])
    tiny, huge = np.float32(1e-45), np.float32(3.4028235e38)
    assert Fraction(float(np.float64(tiny) * np.float64(tiny))) == Fraction(float(tiny)) ** 2
    assert Fraction(float(np.float64(huge) * np.float64(huge))) == Fraction(float(huge)) ** 2


# ---------------------------------------------------------------- the header
C99_USE = r'''
#include <stddef.h>
#include "omx/program_mix.h"
typedef char send_is_40_bytes[sizeof(omx_program_mix_send) == 40 ? 1 : -1];
typedef char info_is_16_bytes[sizeof(omx_program_mix_info) == 16 ? 1 : -1];
typedef char record_is_64_bytes[sizeof(omx_program_mix_record) == 64 ? 1 : -1];
int main(void) {
    return (int)offsetof(omx_program_mix_send, dst_bus) - 4 + (int)offsetof(omx_program_mix_send, src_first) - 8
        + (int)offsetof(omx_program_mix_send, dst_first) - 16 + (int)offsetof(omx_program_mix_send, frames) - 24
        + (int)offsetof(omx_program_mix_send, gain) - 32 + (int)offsetof(omx_program_mix_send, flags) - 36
        + (int)offsetof(omx_program_mix_info, layers_per_batch) - 4 + (int)offsetof(omx_program_mix_info, channels) - 8
        + (int)offsetof(omx_program_mix_record, mixed_frames) - 24 + (int)offsetof(omx_program_mix_record, samples_nonfinite) - 40
        + (int)offsetof(omx_program_mix_record, out_sample_peak) - 48 + (int)offsetof(omx_program_mix_record, sends) - 56
        + (int)offsetof(omx_program_mix_record, max_layers) - 60
        + (int)(OMX_MIX_MAX_LAYERS - 64u) + (int)(OMX_MIX_MAX_SENDS - 1048576u) + (OMX_MIX_MAX_POSITION == (1ull << 40) ? 0 : 1);
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
    header = open(os.path.join(INCLUDE, "program_mix.h")).read()
    assert '#include "program_filter.h"' in header
    sizes = {"omx_program_mix_send": (oa.CProgramMixSend, 40), "omx_program_mix_info": (oa.CProgramMixInfo, 16),
             "omx_program_mix_record": (oa.CProgramMixRecord, 64)}
    for name, (struct, size) in sizes.items():
        assert C.sizeof(struct) == size
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), (name, "the header's comment does not give this size")
    assert oa.MIX_RECORD_DTYPE == mr.RECORD_DTYPE
    for dtype, struct in ((oa.MIX_RECORD_DTYPE, oa.CProgramMixRecord), (oa.MIX_SEND_DTYPE, oa.CProgramMixSend), (oa.MIX_INFO_DTYPE, oa.CProgramMixInfo)):
        assert dtype.itemsize == C.sizeof(struct)
        for f in dtype.names:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    assert [getattr(oa.CProgramMixSend, f).offset for f in oa.MIX_SEND_DTYPE.names] == [0, 4, 8, 16, 24, 32, 36]
    assert [getattr(oa.CProgramMixRecord, f).offset for f in mr.RECORD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert list(oa.MIX_SEND_DTYPE.names) == list(mr.Send.__dataclass_fields__) == list(oa.MixSend.__dataclass_fields__)
    syms = declared(os.path.join(INCLUDE, "program_mix.h"))
    assert syms == ["omx_program_loudness_bank_fetch_mixed", "omx_program_loudness_bank_mix", "omx_program_loudness_bank_mix_configure",
                    "omx_program_mix_extent", "omx_program_mix_null", "omx_program_mix_plan"]
    for s in syms:
        assert hasattr(omx.lib, s), f"declared in include/omx/program_mix.h but not exported: {s}"
    # additive: nothing of it is declared in omx.h, and the ABI version did not move for it
    assert "program_mix" not in open(os.path.join(ROOT, "include", "omx.h")).read()
    for name in ("MixSend", "MIX_SEND_DTYPE", "MIX_RECORD_DTYPE", "mix_table", "mix_plan", "mix_extent", "mix_null"):
        assert hasattr(oa, name), name
    assert (oa.MIX_MAX_LAYERS, oa.MIX_MAX_SENDS, oa.MIX_MAX_POSITION) == (mr.MAX_LAYERS, mr.MAX_SENDS, mr.MAX_POSITION)
    for name in ("configure_mix", "mix", "fetch_mixed"):
        assert hasattr(oa.ProgramLoudnessBank, name), name


def build_demo(tmp_path):
    """tests/c_abi/program_mix_demo.c: a plain C99 host that sums three stems into a bus and null-tests them against a printmaster"""
    out = str(tmp_path / "program_mix_demo")
    libdir = os.path.join(ROOT, "openmeters_amd", "csrc")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "program_mix_demo.c"), "-o", out, "-L", libdir, "-lomx_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_c99_demo_builds_against_the_header(tmp_path, omx):
    assert os.path.exists(build_demo(tmp_path))


def test_plan(omx):
    import openmeters_amd as oa
    plan = omx.fn("program_mix_plan", C.c_int, [C.c_uint32, C.c_void_p])
    for ch in range(1, 9):
        info = oa.mix_plan(omx, ch)
        t, b = int(info["tile_frames"]), int(info["layers_per_batch"])
        assert int(info["channels"]) == ch and t >= 64 and t % 64 == 0 and int(info["_pad"]) == 0
        assert 2 <= b <= 32 and 2 * b + 1 <= mr.MAX_LAYERS      # the depth cases B - 1 .. 2 B + 1 are distinct and allowed
    for ch in (0, 9, 2 ** 32 - 1):
        buf = np.full((16,), 0xAB, np.uint8)
        assert plan(ch, buf.ctypes.data) == capi.ERR_INVALID and (buf == 0xAB).all(), ch
        assert last_error(omx).startswith("program loudness mix plan: ")
    assert plan(2, None) == capi.ERR_INVALID


# ---------------------------------------------------------------- extent
def to_api(sends):
    import openmeters_amd as oa
    return [oa.MixSend(**s.__dict__) for s in sends]


def test_extent_equals_the_restatement(omx):
    import openmeters_amd as oa
    rng = np.random.default_rng(21)
    accepted = refused = 0
    for trial in range(200):
        n_in, n_out = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        frames_in = [int(v) for v in rng.integers(0 if trial % 5 else 40, 60, n_in)]
        sends = []
        for o in range(n_out):
            at, mine = 0, []
            for _ in range(int(rng.integers(55, 80) if trial % 5 == 0 else rng.integers(0, 8))):      # (every fifth table is deep)
                s = int(rng.integers(0, n_in))
                n = int(rng.integers(frames_in[s] // 2 if trial % 5 == 0 else 0, frames_in[s] + 1))
                at = max(0, at + int(rng.integers(-6, 10) if trial % 5 else rng.integers(0, 2)))
                mine.append(mr.Send(s, o, int(rng.integers(0, frames_in[s] - n + 1)), at, n, float(rng.integers(-4, 5)) / 4))
            if trial % 7:      # (every seventh table keeps its disorder)
                mine.sort(key=lambda c: c.dst_first)
            sends += mine
        try:
            want = mr.extent(sends, frames_in, n_out)
            accepted += 1
        except mr.Invalid:
            want = None
            refused += 1
        if want is None:
            with pytest.raises(capi.OmxError) as err:
                oa.mix_extent(omx, to_api(sends), frames_in, n_out)
            assert err.value.status == capi.ERR_INVALID
        else:
            assert [int(v) for v in oa.mix_extent(omx, to_api(sends), frames_in, n_out)] == want, (trial, sends)
    assert accepted >= 40 and refused >= 20
    # zero frames: a send of none, a table of none
    assert list(oa.mix_extent(omx, [oa.MixSend(frames=0, dst_first=5)], [0], 2)) == [0, 0]
    assert list(oa.mix_extent(omx, [], [3], 1)) == [0]
    assert list(oa.mix_extent(omx, [oa.MixSend(frames=2 ** 32 - 1, dst_first=2 ** 40 - 2 ** 32 + 1)], [2 ** 32 - 1], 1)) == [2 ** 40]
    # exactly 64 over a frame is accepted, a 65th refused; a send of 0 frames among them does not count; ends AT a start free a layer
    full = [mr.Send(0, 0, 0, 0, 10) for _ in range(64)]
    assert list(oa.mix_extent(omx, to_api(full), [10], 1)) == mr.extent(full, [10], 1) == [10]
    with_empty = full[:30] + [mr.Send(0, 0, 0, 0, 0)] + full[30:]
    assert list(oa.mix_extent(omx, to_api(with_empty), [10], 1)) == [10]
    behind = full + [mr.Send(0, 0, 0, 10, 5)]
    assert list(oa.mix_extent(omx, to_api(behind), [10], 1)) == mr.extent(behind, [10], 1) == [15]
    with pytest.raises(mr.Invalid):
        mr.extent(full + [mr.Send(0, 0, 0, 9, 1)], [10], 1)
    with pytest.raises(capi.OmxError):
        oa.mix_extent(omx, to_api(full + [mr.Send(0, 0, 0, 9, 1)]), [10], 1)
    assert "more than 64 sends" in last_error(omx)


def test_extent_refuses_bad_tables_and_writes_nothing(omx):
    import openmeters_amd as oa
    fn = omx.fn("program_mix_extent", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
    frames_in = np.array([100, 50], np.uint32)
    good = [mr.Send(0, 0, 0, 0, 40, 0.5), mr.Send(1, 0, 0, 30, 50, -1.0), mr.Send(0, 1, 60, 5, 40)]
    assert list(oa.mix_extent(omx, to_api(good), frames_in, 2)) == mr.extent(good, list(frames_in), 2) == [80, 45]

    def refused(sends, tag, n_in=2, n_out=2, restated=True):
        table = oa.mix_table(to_api(sends))
        out = np.full((max(n_out, 1),), 0xABABABABABABABAB, np.uint64)
        assert fn(table.ctypes.data, table.size, n_in, frames_in.ctypes.data, n_out, out.ctypes.data) == capi.ERR_INVALID, tag
        assert (out == 0xABABABABABABABAB).all(), (tag, "out_frames was written")
        assert last_error(omx).startswith("program loudness mix extent: "), (tag, last_error(omx))
        if restated:
            with pytest.raises(mr.Invalid):
                mr.extent(sends, list(frames_in[:n_in]), n_out)

    def with_(k, **kw):
        sends = [mr.Send(**c.__dict__) for c in good]
        for f, v in kw.items():
            setattr(sends[k], f, v)
        return sends

    refused([good[1], good[0], good[2]], "unsorted by dst_first")
    refused([good[2], good[0], good[1]], "unsorted by dst_bus")
    refused([mr.Send(0, 0, 0, 0, 40)] * 65, "a 65th send over a frame")
    refused(with_(0, src_first=61), "a send beyond frames_in")
    refused(with_(1, frames=51), "a send longer than frames_in")
    refused(with_(2, flags=1), "non-zero flags")
    refused(with_(2, flags=2 ** 31), "a high flag")
    refused(with_(1, gain=float("nan")), "NaN gain")
    refused(with_(1, gain=float("inf")), "infinite gain")
    refused(with_(1, gain=float("-inf")), "negative infinite gain")
    refused(with_(0, src_stream=2), "src_stream out of range")
    refused(with_(2, dst_bus=2), "dst_bus out of range")
    refused(with_(2, dst_first=2 ** 40 - 39), "dst_first + frames beyond 2^40")
    # more than 2^20 sends (of 0 frames each: nothing else is wrong with the table)
    many = np.zeros(mr.MAX_SENDS + 1, oa.MIX_SEND_DTYPE)
    out = np.full((1,), 7, np.uint64)
    assert fn(many.ctypes.data, many.size, 2, frames_in.ctypes.data, 1, out.ctypes.data) == capi.ERR_INVALID and out[0] == 7
    assert "2^20" in last_error(omx)
    assert fn(many.ctypes.data, mr.MAX_SENDS, 2, frames_in.ctypes.data, 1, out.ctypes.data) == 0 and out[0] == 0
    # null pointers
    table = oa.mix_table(to_api(good))
    out = np.full((2,), 7, np.uint64)
    assert fn(None, 3, 2, frames_in.ctypes.data, 2, out.ctypes.data) == capi.ERR_INVALID
    assert fn(table.ctypes.data, 3, 2, None, 2, out.ctypes.data) == capi.ERR_INVALID
    assert fn(table.ctypes.data, 3, 2, frames_in.ctypes.data, 2, None) == capi.ERR_INVALID
    assert (out == 7).all()


# ---------------------------------------------------------------- the null test's table
def test_mix_null_equals_the_restatement_and_refuses_bad_arguments(omx):
    import openmeters_amd as oa
    for stems, ref, frames, bus in (([0, 1, 2], 3, 12000, 1), ([5], 5, 0, 0), (list(range(63)), 63, 2 ** 40, 7), ([2, 2, 0], 1, 9, 3)):
        got = oa.mix_null(omx, stems, ref, frames, bus)
        want = oa.mix_table(to_api(mr.null_table(stems, ref, frames, bus)))
        assert got.tobytes() == want.tobytes(), (stems, got, want)
        assert (got["gain"][:-1] == 1.0).all() and got["gain"][-1] == -1.0 and not got["flags"].any()
        if frames <= 2 ** 32 - 1:      # the table is one the check accepts
            assert int(oa.mix_extent(omx, got, [frames] * 64, bus + 1)[bus]) == frames
    fn = omx.fn("program_mix_null", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p])
    stems = np.arange(64, dtype=np.uint32)
    for args, tag in (((None, 3, 3, 10, 0), "null stems"), ((stems.ctypes.data, 0, 3, 10, 0), "no stem"),
                      ((stems.ctypes.data, 64, 3, 10, 0), "64 stems"), ((stems.ctypes.data, 3, 3, 2 ** 40 + 1, 0), "frames beyond 2^40")):
        out = np.full((65 * 40,), 0xAB, np.uint8)
        assert fn(*args, out.ctypes.data) == capi.ERR_INVALID and (out == 0xAB).all(), tag
        assert last_error(omx).startswith("program loudness mix null: "), tag
    assert fn(stems.ctypes.data, 3, 3, 10, 0, None) == capi.ERR_INVALID
    with pytest.raises(mr.Invalid):
        mr.null_table([], 0, 5)
    with pytest.raises(mr.Invalid):
        mr.null_table(list(range(64)), 0, 5)


def test_null_test_of_a_lattice_leaves_nothing_in_the_restatement():
    stems, pm = mr.lattice(31, 500, 2, 3)
    (y,), (rec,) = mr.render(stems + [pm], mr.null_table([0, 1, 2], 3, 500), [500], 2)
    assert not y.any() and int(rec["max_layers"]) == 4 and float(rec["out_sample_peak"]) == 0.0 and np.float32(rec["out_sample_peak_db"]) == np.float32(-99.9)
    stems[1][77, 1] += np.float32(2.0 ** -16)
    (y,), (rec,) = mr.render(stems + [pm], mr.null_table([0, 1, 2], 3, 500), [500], 2)
    assert float(rec["out_sample_peak"]) == 2.0 ** -16 and np.count_nonzero(y) == 1
    assert abs(float(rec["out_sample_peak_db"]) - 20 * np.log10(2.0 ** -16)) <= 1e-4

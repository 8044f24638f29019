"""Programme bank groups on the GPU (`-m gpu`): openmeters_amd.ProgramLoudnessBank.measure_groups / fetch_groups against the numpy
restatement (tests/program_groups_ref.py, pinned by tests/test_cpu_program_groups.py, which also asserts the gate margin and the
bin-cleanliness of every input used here).

The restatement is fed the bank's own fetch_segments, as the result-pass checks of the other programme files are.  Bars: counts
exact; lra_low_energy, lra_high_energy and both maxima equal bits (order statistics and maxima do not depend on the order of the
sums); LUFS / LU fields 1e-4; the two means within ref.energy_bound(total gating blocks), relative.  A group of one member has the
bytes of fetch_intervals of that member.  Bounded banks: every count and f64 field equals the histogram restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import program_groups_ref as gr
import program_histogram_ref as hr
import program_loudness_ref as ref
import openmeters_amd
from openmeters_amd import capi
from openmeters_amd.capi import LoudnessConfig
from openmeters_amd.program_loudness import (FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL, GROUP_DTYPE, INTERVAL_DTYPE, RECORD_DTYPE, TO_END,
                                             ProgramLoudnessBank)
from parity import bar
from test_gpu_program_loudness import BAR, FLOOR, device_rows, torch_dev  # noqa: F401
from test_gpu_program_timeline import device_bytes, record_array

pytestmark = pytest.mark.gpu
POS1 = capi.positions_fallback(1)
NOT_OF_A_PART = ("frames", "overflow", "max_true_peak_db", "_pad")


def make_bank(torch, omx, xs, fs=gr.RATE, ch=1, form=0, capacity_seconds=100, storage="segments"):
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=fs), len(xs), ch, capacity_seconds, storage=storage)
    bank.set_option(capi.OPT_KERNEL_FORM, form)
    feed(torch, bank, xs, fs, ch)
    return bank


def feed(torch, bank, xs, fs=gr.RATE, ch=1):
    d, longest = device_rows(torch, [x if len(x) else np.zeros((1, ch), np.float32) for x in xs], ch)
    bank.process(d.data_ptr(), longest, ch, fs, capi.positions_fallback(ch), frames=[len(x) for x in xs],
                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def level(torch_dev, omx):
    """the level bank, its stored segment energies (the restatement's input) and its records, made once"""
    bank = make_bank(torch_dev, omx, gr.level_programmes())
    es = [bank.fetch_segments(s) for s in range(4)]
    assert [len(e) for e in es] == gr.LEVEL_SEGMENTS
    return bank, es


def check_group(got, want, tag, measured):
    """one group record against the restatement of the same members over the bank's own segments"""
    assert want["gate_margin"] >= ref.RESULT_PASS_MARGIN_MIN, (tag, want["gate_margin"])
    for f in gr.RECORD_LEVELS + gr.RECORD_ENERGIES:
        assert np.isfinite(got[f]), (tag, f, got[f])
    for f in gr.RECORD_COUNTS + ("frames", "overflow"):
        assert int(got[f]) == int(want[f]), (tag, f, int(got[f]), int(want[f]))
    assert got["max_true_peak_db"] == np.float32(FLOOR), tag
    for f in gr.ORDER_FREE + ("momentary_energy", "short_term_energy"):
        assert np.float64(got[f]).tobytes() == np.float64(want[f]).tobytes(), (tag, f, float(got[f]), float(want[f]))
    for f in gr.RECORD_LEVELS:
        d = bar(f"program groups: |d {f}| LU", abs(float(got[f]) - float(want[f])), BAR, (tag, got[f], want[f]))
        measured[f] = max(measured.get(f, 0.0), d)
    bound = ref.energy_bound(int(want["gating_blocks"]))
    for f in gr.MEANS:
        exp = float(want[f])
        rel = abs(float(got[f]) - exp) / exp if exp > 0.0 else abs(float(got[f]))
        measured[f] = max(measured.get(f, 0.0), rel)
        assert rel <= bound, (tag, f, float(got[f]), exp, rel, bound)


def fmt(measured):
    return {k: f"{v:.2e}" for k, v in measured.items()}


def members_of(table, group):
    return table[group[0]:group[0] + group[1]]


# ---------------------------------------------------------------- 1. anchor: a group of one member is the interval pass
@pytest.mark.parametrize("form", [FORM_REFERENCE_ORDER, FORM_TIME_PARALLEL])
def test_one_member_groups_have_the_bytes_of_fetch_intervals(torch_dev, omx, form):
    bank = make_bank(torch_dev, omx, gr.anchor_programmes(), form=form)
    assert bank.last_form() == form
    segments = [bank.fetch(s).segments for s in range(5)]
    assert segments == gr.ANCHOR_SEGMENTS
    members = gr.anchor_members()
    got = bank.fetch_groups(members, [(i, 1) for i in range(len(members))])
    want = bank.fetch_intervals(gr.resolve(members, segments))
    assert len(got) == len(members) == 60
    for i, m in enumerate(members):
        assert got[i].tobytes() == want[i].tobytes(), (m, got[i], want[i])
    # a group of one whole stream: the bytes of fetch but for frames, overflow and max_true_peak_db
    for s in range(5):
        rec, whole = record_array(bank.fetch(s)), got[members.index((s, 0, TO_END))]
        for f in RECORD_DTYPE.names:
            if f not in NOT_OF_A_PART:
                assert whole[f].tobytes() == rec[f].tobytes(), (s, f, whole[f], rec[f])
        assert whole["frames"] == segments[s] * gr.SEG and whole["overflow"] == 0 and whole["max_true_peak_db"] == np.float32(FLOOR)


# ---------------------------------------------------------------- 2. multi-member groups against the restatement
def test_level_groups_against_the_restatement(torch_dev, omx, level):
    """members 10 to 30 dB apart with 3, 4, 29, 30, 255, 301 and 700 segments"""
    bank, es = level
    names = list(gr.LEVEL_GROUPS)
    got = bank.fetch_groups(gr.LEVEL_MEMBERS, [gr.LEVEL_GROUPS[n] for n in names])
    measured = {}
    for i, name in enumerate(names):
        members = members_of(gr.LEVEL_MEMBERS, gr.LEVEL_GROUPS[name])
        want = gr.results(es, members, gr.SEG, FLOOR)
        check_group(got[i], want, name, measured)
        print(name, got[i]["integrated_lufs"], got[i]["loudness_range_lu"], int(got[i]["gating_above_relative"]), "of", int(got[i]["gating_blocks"]))
    album = got[names.index("loud and quiet album")]
    own = bank.fetch_intervals(members_of(gr.LEVEL_MEMBERS, gr.LEVEL_GROUPS["loud and quiet album"]))
    assert int(album["gating_above_relative"]) < int(own["gating_above_relative"].sum()) - 50      # the album's gate removes what the tracks keep
    short = got[names.index("too short for a short-term block")]
    assert short["short_term_blocks"] == 0 and short["gating_blocks"] == 27 and short["loudness_range_lu"] == 0.0
    # the device array and the fetch form agree
    d = bank.measure_groups(gr.LEVEL_MEMBERS, [gr.LEVEL_GROUPS[n] for n in names], stream=torch_dev.cuda.current_stream().cuda_stream)
    torch_dev.cuda.synchronize()
    assert device_bytes(d, len(names) * RECORD_DTYPE.itemsize) == got.tobytes()
    print("level groups, measured (LU / relative):", fmt(measured))


def test_long_groups_on_both_sides_of_the_staging_threshold(torch_dev, omx, level):
    """groups of 4026 ... 8862 short-term blocks in one call: from 4096 on the kernel stages the blocks once and reads them back"""
    bank, es = level
    names = list(gr.LONG_GROUPS)
    groups = [gr.LONG_GROUPS[n] for n in names]
    got, measured = bank.fetch_groups(gr.LONG_MEMBERS, groups), {}
    for i, name in enumerate(names):
        check_group(got[i], gr.results(es, members_of(gr.LONG_MEMBERS, gr.LONG_GROUPS[name]), gr.SEG, FLOOR), name, measured)
    assert [int(r["short_term_blocks"]) for r in got] == [4026, 4096, 4095, 4697, 8862]
    assert bank.fetch_groups(gr.LONG_MEMBERS, groups).tobytes() == got.tobytes()
    # each group alone (another place in the staging scratch) and after a call that used the scratch for other groups
    for i in (3, 1, 4):
        assert bank.fetch_groups(gr.LONG_MEMBERS, [groups[i]])[0].tobytes() == got[i].tobytes(), names[i]
    # the order-free fields of a staged group and of the same members in another order
    again = bank.fetch_groups(gr.LONG_MEMBERS[8:15][::-1], [(0, 7)])[0]
    for f in gr.RECORD_COUNTS + gr.ORDER_FREE:
        assert again[f].tobytes() == got[3][f].tobytes(), f
    print("long groups, measured (LU / relative):", fmt(measured))


# ---------------------------------------------------------------- 3. member order
def test_member_order_moves_only_the_means_and_the_latest_fields(torch_dev, omx, level):
    bank, es = level
    base = bank.fetch_groups(gr.LEVEL_MEMBERS, [gr.LEVEL_GROUPS[gr.PERMUTED]])[0]
    measured = {}
    for order in gr.PERMUTATIONS:
        members = gr.permuted_members(order)
        got = bank.fetch_groups(members, [(0, len(members))])[0]
        check_group(got, gr.results(es, members, gr.SEG, FLOOR), ("permuted", order), measured)
        for f in gr.RECORD_COUNTS + ("frames",):
            assert got[f] == base[f], (order, f)
        for f in gr.ORDER_FREE:
            assert got[f].tobytes() == base[f].tobytes(), (order, f)
        bound = ref.energy_bound(int(base["gating_blocks"]))
        for f in gr.MEANS:
            assert abs(float(got[f]) - float(base[f])) <= bound * float(base[f]), (order, f)
        last = bank.fetch_intervals([members[-1]])[0]       # the latest fields follow the new last member
        for f in ("momentary_energy", "short_term_energy", "momentary_lufs", "short_term_lufs"):
            assert got[f].tobytes() == last[f].tobytes(), (order, f)
    assert {bank.fetch_intervals([gr.permuted_members(o)[-1]])[0]["momentary_energy"].tobytes() for o in gr.PERMUTATIONS} != {base["momentary_energy"].tobytes()}


# ---------------------------------------------------------------- 4. shapes
def test_overlaps_duplicates_empty_groups_and_to_end(torch_dev, omx, level):
    bank, es = level
    names = list(gr.SHAPE_GROUPS)
    groups = [gr.SHAPE_GROUPS[n] for n in names]
    got = bank.fetch_groups(gr.SHAPE_MEMBERS, groups)
    assert bank.fetch_groups(gr.SHAPE_MEMBERS, groups).tobytes() == got.tobytes()        # the same call twice
    by, measured = dict(zip(names, got)), {}
    for name in names:
        check_group(by[name], gr.results(es, members_of(gr.SHAPE_MEMBERS, gr.SHAPE_GROUPS[name]), gr.SEG, FLOOR), name, measured)
    single, double = by["single"], by["double"]
    for f in gr.RECORD_COUNTS + ("frames",):                                              # a duplicated member counts twice, exactly
        assert int(double[f]) == 2 * int(single[f]), f
    for f in gr.ORDER_FREE:
        assert double[f].tobytes() == single[f].tobytes(), f
    empty = np.zeros((), RECORD_DTYPE)
    for f in ("integrated_lufs", "relative_threshold_lufs", "momentary_lufs", "short_term_lufs", "max_momentary_lufs", "max_short_term_lufs",
              "max_true_peak_db"):
        empty[f] = FLOOR
    for name in ("empty", "empty at the table's end", "at the end of the stream"):
        assert by[name].tobytes() == empty.tobytes(), (name, by[name])
    assert by["to end"].tobytes() == by["explicit"].tobytes() and by["part to end"].tobytes() == by["part explicit"].tobytes()
    assert by["to end"].tobytes() == bank.fetch_intervals([(2, 0, 700)])[0].tobytes()
    # each group alone gives the bytes it has inside the overlapping call
    for name in ("overlap a", "overlap b", "all"):
        first, count = gr.SHAPE_GROUPS[name]
        assert bank.fetch_groups(gr.SHAPE_MEMBERS[first:first + count], [(0, count)])[0].tobytes() == by[name].tobytes(), name
    # arrays of the two dtypes are taken as they are
    m = np.zeros((len(gr.SHAPE_MEMBERS),), INTERVAL_DTYPE)
    for i, (s, a, c) in enumerate(gr.SHAPE_MEMBERS):
        m[i] = (s, 0, a, c)
    g = np.array(groups, dtype=np.uint64).view(GROUP_DTYPE).reshape(-1)
    assert bank.fetch_groups(m, g).tobytes() == got.tobytes()
    print("shapes, measured (LU / relative):", fmt(measured))


def test_64_groups_of_64_members_in_one_call(torch_dev, omx):
    bank = make_bank(torch_dev, omx, gr.wide_programmes())
    es = [bank.fetch_segments(s) for s in range(gr.WIDE_STREAMS)]
    members, groups = gr.wide_call([len(e) for e in es])
    got, measured = bank.fetch_groups(members, groups), {}
    assert len(got) == 64
    for k, g in enumerate(groups):
        check_group(got[k], gr.results(es, members_of(members, g), gr.SEG, FLOOR), ("wide", k), measured)
    assert bank.fetch_groups(members, groups).tobytes() == got.tobytes()
    print("64 x 64, measured (LU / relative):", fmt(measured))


def test_later_appends_leave_explicit_members_alone(torch_dev, omx):
    xs = gr.append_programmes()
    cut = int(gr.RATE * gr.APPEND_CUT_SECONDS)
    bank = ProgramLoudnessBank(omx, LoudnessConfig(sample_rate=gr.RATE), 2, 1, 100)
    bank.set_option(capi.OPT_KERNEL_FORM, FORM_REFERENCE_ORDER)
    feed(torch_dev, bank, [x[:cut] for x in xs])
    before, measured = bank.fetch_groups(gr.APPEND_MEMBERS, gr.APPEND_GROUPS), {}
    es = [bank.fetch_segments(s) for s in range(2)]
    for k, g in enumerate(gr.APPEND_GROUPS):
        check_group(before[k], gr.results(es, members_of(gr.APPEND_MEMBERS, g), gr.SEG, FLOOR), ("before", k), measured)
    feed(torch_dev, bank, [x[cut:] for x in xs])
    after = bank.fetch_groups(gr.APPEND_MEMBERS, gr.APPEND_GROUPS)
    es = [bank.fetch_segments(s) for s in range(2)]
    assert [len(e) for e in es] == [400, 400]
    for k, g in enumerate(gr.APPEND_GROUPS):
        check_group(after[k], gr.results(es, members_of(gr.APPEND_MEMBERS, g), gr.SEG, FLOOR), ("after", k), measured)
        explicit = all(c != TO_END for _, _, c in members_of(gr.APPEND_MEMBERS, g))
        assert (after[k].tobytes() == before[k].tobytes()) == explicit, k
    assert after[3]["segments"] == 400 and before[3]["segments"] == 300


# ---------------------------------------------------------------- 5. known answers through the product
def test_album_answers_through_the_product(torch_dev, omx):
    bank = make_bank(torch_dev, omx, gr.known_programmes(), gr.KNOWN_RATE, 2, capacity_seconds=30)
    names = list(gr.KNOWN_GROUPS)
    got = dict(zip(names, bank.fetch_groups(gr.KNOWN_MEMBERS, [gr.KNOWN_GROUPS[n] for n in names])))
    es, measured = [bank.fetch_segments(s) for s in range(5)], {}
    for n in names:
        check_group(got[n], gr.results(es, members_of(gr.KNOWN_MEMBERS, gr.KNOWN_GROUPS[n]), 4800, FLOOR), n, measured)
    two, three, alone, rng = got["-23 and -29"], got["-23, -29 and -50"], got["-50 alone"], got["-20 and -30"]
    print(two["integrated_lufs"], three["integrated_lufs"], alone["integrated_lufs"], rng["loudness_range_lu"])
    assert abs(float(two["integrated_lufs"]) - gr.KNOWN_ALBUM_LUFS) <= 0.1 and abs(float(three["integrated_lufs"]) - gr.KNOWN_ALBUM_LUFS) <= 0.1
    assert three["integrated_energy"].tobytes() == two["integrated_energy"].tobytes()      # the -50 dBFS member adds no passing block
    assert three["gating_above_relative"] == two["gating_above_relative"] < three["gating_above_absolute"] == two["gating_above_absolute"] + 197
    assert alone["gating_above_relative"] == alone["gating_above_absolute"] == 197           # it would pass its own gate
    assert abs(float(rng["loudness_range_lu"]) - 10.0) <= 1.0


# ---------------------------------------------------------------- 6. bounded bank
def test_bounded_groups_equal_the_histogram_restatement_bit_for_bit(torch_dev, omx):
    B = openmeters_amd.histogram_boundaries(omx)
    xs = gr.bounded_programmes()
    stored, bounded = (make_bank(torch_dev, omx, xs, storage=storage) for storage in ("segments", "histogram"))
    assert bounded.is_bounded() and not stored.is_bounded()
    es = [stored.fetch_segments(s) for s in range(5)]
    assert [len(e) for e in es] == gr.BOUNDED_SEGMENTS
    names = list(gr.BOUNDED_GROUPS)
    members, groups = [], []
    for n in names:
        groups.append((len(members), len(gr.BOUNDED_GROUPS[n])))
        members += [(s, 0, TO_END if i % 2 else len(es[s])) for i, s in enumerate(gr.BOUNDED_GROUPS[n])]
    got = bounded.fetch_groups(members, groups)
    twin = stored.fetch_groups(members, groups)
    assert bounded.fetch_groups(members, groups).tobytes() == got.tobytes()
    worst = 0.0
    for i, n in enumerate(names):
        streams = gr.BOUNDED_GROUPS[n]
        want = gr.bounded_results(es, streams, B, gr.SEG, FLOOR)
        for f in gr.RECORD_COUNTS + ("frames", "overflow"):
            assert int(got[i][f]) == int(want[f]), (n, f, int(got[i][f]), int(want[f]))
        for f in gr.RECORD_ENERGIES:
            assert np.float64(got[i][f]).tobytes() == np.float64(want[f]).tobytes(), (n, f, float(got[i][f]), float(want[f]))
        for f in gr.RECORD_LEVELS:
            assert np.isfinite(got[i][f])
            bar(f"program groups, bounded: |d {f}| LU", abs(float(got[i][f]) - float(want[f])), BAR, (n, got[i][f], want[f]))
        assert got[i]["max_true_peak_db"] == np.float32(FLOOR)
        # against the stored twin (every group is bin-clean: tests/test_cpu_program_groups.py)
        for f in ("gating_above_absolute", "short_term_above_absolute", "segments", "frames", "gating_blocks", "short_term_blocks"):
            assert got[i][f] == twin[i][f], (n, f)
        for f in ("max_momentary_energy", "max_short_term_energy", "momentary_energy", "short_term_energy"):
            assert got[i][f].tobytes() == twin[i][f].tobytes(), (n, f)
        bar("program groups, bounded vs stored: |d integrated_lufs| LU", abs(float(got[i]["integrated_lufs"]) - float(twin[i]["integrated_lufs"])), BAR, n)
        d = abs(float(got[i]["loudness_range_lu"]) - float(twin[i]["loudness_range_lu"]))
        worst = max(worst, d)
        assert d <= hr.LRA_BOUND_LU, (n, d)
    # a group of one stream: the bytes of fetch outside frames and max_true_peak_db
    for n in ("one", "the short one"):
        s = gr.BOUNDED_GROUPS[n][0]
        rec, one = record_array(bounded.fetch(s)), got[names.index(n)]
        for f in RECORD_DTYPE.names:
            if f not in ("frames", "max_true_peak_db"):
                assert one[f].tobytes() == rec[f].tobytes(), (n, f, one[f], rec[f])
    # members that are not whole streams need the segments
    rec0, h0 = bounded.fetch(0), bounded.fetch_histogram(0).tobytes()
    for bad in ([(0, 0, 399)], [(0, 1, TO_END)], [(1, 0, TO_END), (0, 1, 399)], [(0, 400, 0)]):
        for call in (bounded.fetch_groups, bounded.measure_groups):
            with pytest.raises(capi.OmxError) as err:
                call(bad, [(0, len(bad))])
            assert err.value.status == capi.ERR_UNSUPPORTED, (bad, err.value.status)
        assert bounded.fetch(0) == rec0 and bounded.fetch_histogram(0).tobytes() == h0
    with pytest.raises(capi.OmxError) as err:
        bounded.fetch_groups([(0, 0, 401)], [(0, 1)])
    assert err.value.status == capi.ERR_INVALID
    print(f"bounded groups: range at most {worst:.3f} LU from the stored twin's")


# ---------------------------------------------------------------- 7. errors
def test_refused_calls_change_nothing(torch_dev, omx, level):
    bank, _ = level
    good_members, good_groups = gr.LEVEL_MEMBERS, [(0, 2), (2, 7)]
    d = bank.measure_groups(good_members, good_groups)
    torch_dev.cuda.synchronize()
    old = device_bytes(d, 2 * RECORD_DTYPE.itemsize)
    assert old == bank.fetch_groups(good_members, good_groups).tobytes()
    d = bank.measure_groups(good_members, good_groups)        # (the fetch above was a call on the bank: take the array again)
    before = [bank.fetch(s) for s in range(4)]

    def unchanged(tag):
        torch_dev.cuda.synchronize()
        assert device_bytes(d, 2 * RECORD_DTYPE.itemsize) == old, tag
        assert [bank.fetch(s) for s in range(4)] == before, tag

    bad_calls = [([(4, 0, 1)], [(0, 1)]),                       # a stream index out of range
                 ([(2 ** 32 - 1, 0, 0)], [(0, 1)]),
                 ([(0, 701, 0)], [(0, 1)]),                     # first_segment > segments[s]
                 ([(0, 701, TO_END)], [(0, 1)]),
                 ([(0, 0, 701)], [(0, 1)]),                     # first_segment + segment_count > segments[s]
                 ([(0, 699, 2)], [(0, 1)]),
                 ([(0, 2, 2 ** 64 - 2)], [(0, 1)]),
                 ([(0, 0, 700), (1, 0, 701)], [(0, 1)]),        # also a member that no group uses
                 ([(0, 0, 700)], [(0, 2)]),                     # a group range outside the member table
                 ([(0, 0, 700)], [(1, 1)]),
                 ([(0, 0, 700)], [(2, 0)]),
                 ([(0, 0, 700)], [(0, 1), (2 ** 64 - 1, 2)]),
                 ([(0, 0, 700)], [(1, 2 ** 64 - 1)])]
    for members, groups in bad_calls:
        for call in (bank.fetch_groups, bank.measure_groups):
            with pytest.raises(capi.OmxError) as err:
                call(members, groups)
            assert err.value.status == capi.ERR_INVALID, (members, groups, err.value.status)
            unchanged((members, groups))
    measure = omx.fn("program_loudness_bank_measure_groups", C.c_int,
                     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)])
    fetch = omx.fn("program_loudness_bank_fetch_groups", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p])
    m, g = ProgramLoudnessBank._intervals([(0, 0, 700)]), ProgramLoudnessBank._groups([(0, 1)])
    out, dst = C.c_void_p(), np.zeros((1,), RECORD_DTYPE)
    assert measure(bank._h, None, 1, g.ctypes.data, 1, None, C.byref(out)) == capi.ERR_INVALID and not out.value      # null members, n_members > 0
    assert measure(bank._h, m.ctypes.data, 1, None, 1, None, C.byref(out)) == capi.ERR_INVALID and not out.value      # null groups, n_groups > 0
    assert measure(bank._h, m.ctypes.data, 1, g.ctypes.data, 1, None, None) == capi.ERR_INVALID                        # null d_records
    assert measure(bank._h, m.ctypes.data, 2 ** 31, g.ctypes.data, 1, None, C.byref(out)) == capi.ERR_INVALID           # too many members
    assert measure(bank._h, m.ctypes.data, 1, g.ctypes.data, 2 ** 31, None, C.byref(out)) == capi.ERR_INVALID           # too many groups
    assert measure(None, m.ctypes.data, 1, g.ctypes.data, 1, None, C.byref(out)) == capi.ERR_INVALID
    assert fetch(bank._h, None, 1, g.ctypes.data, 1, dst.ctypes.data) == capi.ERR_INVALID
    assert fetch(bank._h, m.ctypes.data, 1, None, 1, dst.ctypes.data) == capi.ERR_INVALID
    assert fetch(bank._h, m.ctypes.data, 1, g.ctypes.data, 1, None) == capi.ERR_INVALID                                 # null dst
    assert fetch(bank._h, m.ctypes.data, 2 ** 31, g.ctypes.data, 1, dst.ctypes.data) == capi.ERR_INVALID
    assert not out.value and not dst.view(np.uint8).any()
    unchanged("null and oversized arguments")
    # no group: OMX_NONE, nothing is measured; a group without members and a call without members are fine
    assert measure(bank._h, m.ctypes.data, 1, None, 0, None, C.byref(out)) == 0 and not out.value
    assert fetch(bank._h, None, 0, None, 0, None) == 0
    assert bank.measure_groups(gr.LEVEL_MEMBERS, []) == 0 and len(bank.fetch_groups(gr.LEVEL_MEMBERS, [])) == 0
    unchanged("no group")
    assert bank.fetch_groups([], [(0, 0)])[0]["segments"] == 0


def test_a_group_of_more_than_2_32_blocks_is_refused(torch_dev, omx):
    """the same 700-segment stream 2^23 times in a group has 697 * 2^23 > 2^32 - 1 gating blocks; half of that is measured elsewhere
    only in the benchmark, here the refusal is what counts: nothing is launched"""
    bank = make_bank(torch_dev, omx, gr.level_programmes()[:1])
    members = np.zeros((2 ** 23,), INTERVAL_DTYPE)
    members["segment_count"] = 700
    before = bank.fetch(0)
    with pytest.raises(capi.OmxError) as err:
        bank.fetch_groups(members, [(0, 8), (0, 2 ** 23)])
    assert err.value.status == capi.ERR_INVALID
    assert bank.fetch(0) == before
    assert bank.fetch_groups(members[:8], [(0, 8)])[0]["gating_blocks"] == 8 * 697

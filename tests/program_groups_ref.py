"""f64 numpy restatement of the programme bank's groups (include/omx/program_groups.h, DESIGN.md section 10 "Groups") on top of
program_loudness_ref and program_histogram_ref: the record of several streams, or parts of streams, measured as one programme.
Members contribute their own gating and short-term blocks (no block spans two members); the group record is ref.results with the
concatenations G and ST in place of the sliding means.  Also the inputs shared by tests/test_cpu_program_groups.py and
tests/test_gpu_program_groups.py (the CPU file asserts the conditions the GPU comparisons need on every one of them)."""
import numpy as np

import program_histogram_ref as hr
import program_loudness_ref as ref

TO_END = 2 ** 64 - 1
RECORD_ENERGIES, RECORD_COUNTS, RECORD_LEVELS = hr.RECORD_ENERGIES, hr.RECORD_COUNTS, hr.RECORD_LEVELS
ORDER_FREE = ("lra_low_energy", "lra_high_energy", "max_momentary_energy", "max_short_term_energy")   # order statistics and maxima
MEANS = {"integrated_energy": "gating_above_relative", "relative_threshold_energy": "gating_above_absolute"}


def resolve(members, segments):
    """(stream, first, count) with TO_END replaced by what the stream holds"""
    out = []
    for s, first, count in members:
        n = int(segments[s]) - first if count == TO_END else count
        assert 0 <= first and n >= 0 and first + n <= int(segments[s]), (s, first, count)
        out.append((int(s), int(first), int(n)))
    return out


def blocks(es, members):
    """(G, ST, parts): the members' gating and short-term blocks concatenated in member order, and the members' slices of e[]"""
    members = resolve(members, [len(e) for e in es])
    parts = [np.asarray(es[s], np.float64)[a:a + n] for s, a, n in members]
    G = np.concatenate([ref.sliding_mean(p, 4) for p in parts] + [np.zeros(0)])
    ST = np.concatenate([ref.sliding_mean(p, 30) for p in parts] + [np.zeros(0)])
    return G, ST, parts


def results(es, members, segment_frames=0, floor=-99.9):
    """the group record (dict with the field names of omx_program_loudness_record, plus gate_margin) of `members`, a list of
    (stream, first_segment, segment_count), over a bank whose stored segment energies are es[stream]"""
    g, st, parts = blocks(es, members)
    segments = sum(len(p) for p in parts)
    r = {"segments": segments, "frames": segments * segment_frames, "overflow": 0, "max_true_peak_db": np.float32(floor),
         "gating_blocks": len(g), "short_term_blocks": len(st)}
    margin = min(ref._margin(g, ref.ABSOLUTE_GATE), ref._margin(st, ref.ABSOLUTE_GATE))
    ga = g[g > ref.ABSOLUTE_GATE]
    rel = 0.1 * ga.mean() if len(ga) else 0.0
    gr = ga[ga > rel]
    margin = min(margin, ref._margin(ga, rel))
    r["gating_above_absolute"], r["gating_above_relative"] = len(ga), len(gr)
    r["relative_threshold_energy"] = rel
    r["integrated_energy"] = gr.mean() if len(gr) else 0.0
    sa = st[st > ref.ABSOLUTE_GATE]
    srel = 0.01 * sa.mean() if len(sa) else 0.0
    sr = np.sort(sa[sa > srel])
    margin = min(margin, ref._margin(sa, srel))
    r["short_term_above_absolute"], r["short_term_above_relative"] = len(sa), len(sr)
    if len(sr):
        lo = sr[int(np.floor((len(sr) - 1) * 0.10 + 0.5))]
        hi = sr[int(np.floor((len(sr) - 1) * 0.95 + 0.5))]
        r["lra_low_energy"], r["lra_high_energy"] = lo, hi
        r["loudness_range_lu"] = np.float32(ref.level(hi) - ref.level(lo))
    else:
        r["lra_low_energy"] = r["lra_high_energy"] = 0.0
        r["loudness_range_lu"] = np.float32(0.0)
    # the latest blocks are the last member's
    last_g = ref.sliding_mean(parts[-1], 4) if parts else np.zeros(0)
    last_st = ref.sliding_mean(parts[-1], 30) if parts else np.zeros(0)
    r["momentary_energy"] = last_g[-1] if len(last_g) else 0.0
    r["short_term_energy"] = last_st[-1] if len(last_st) else 0.0
    r["max_momentary_energy"] = g.max() if len(g) else 0.0
    r["max_short_term_energy"] = st.max() if len(st) else 0.0
    for name in ("integrated", "relative_threshold", "momentary", "short_term", "max_momentary", "max_short_term"):
        r[name + "_lufs"] = ref.lufs(r[name + "_energy"], floor)
    r["gate_margin"] = margin
    return r


# ---- bounded mode: the members are whole streams, the group's histogram is the sum of theirs
def group_histogram(es, streams, B):
    """count[i] = sum of the members' counts; sum[i] = the members' sums added in member order, in f64, starting from 0"""
    h = {"gating_count": np.zeros(hr.BINS, np.uint64), "gating_sum": np.zeros(hr.BINS, np.float64),
         "short_term_count": np.zeros(hr.BINS, np.uint64), "short_term_sum": np.zeros(hr.BINS, np.float64)}
    for s in streams:
        m = hr.histogram(es[s], B)
        for f in h:
            h[f] = h[f] + m[f]
    return h


def bounded_results(es, streams, B, segment_frames=0, floor=-99.9):
    """the record of a group of whole streams on a bank with bounded storage: hr.results with the group's histogram in place of the
    stream's, the maxima over the members, the latest blocks of the last member, the counts summed"""
    h = group_histogram(es, streams, B)
    per = [(ref.sliding_mean(np.asarray(es[s], np.float64), 4), ref.sliding_mean(np.asarray(es[s], np.float64), 30)) for s in streams]
    segments = sum(len(es[s]) for s in streams)
    r = {"segments": segments, "frames": segments * segment_frames, "overflow": 0, "max_true_peak_db": np.float32(floor),
         "gating_blocks": sum(len(g) for g, _ in per), "short_term_blocks": sum(len(st) for _, st in per), "histogram": h}
    n, threshold, passing = hr.gate(h["gating_count"], h["gating_sum"], 0.1)
    r["gating_above_absolute"], r["relative_threshold_energy"] = n, threshold
    pc = int(hr.ascending_sum(np.where(passing, h["gating_count"], np.uint64(0))))
    r["gating_above_relative"] = pc
    r["integrated_energy"] = hr.ascending_sum(np.where(passing, h["gating_sum"], 0.0)) / np.float64(pc) if pc else 0.0
    n, _, passing = hr.gate(h["short_term_count"], h["short_term_sum"], 0.01)
    r["short_term_above_absolute"] = n
    counts = np.where(passing, h["short_term_count"], np.uint64(0))
    pc = int(hr.ascending_sum(counts))
    r["short_term_above_relative"] = pc
    if pc:
        upto = np.cumsum(counts)
        ends = []
        for q in (0.10, 0.95):
            rank = int(np.floor((np.float64(pc) - 1.0) * q + 0.5))
            i = int(np.searchsorted(upto, rank, side="right"))
            ends.append(h["short_term_sum"][i] / np.float64(h["short_term_count"][i]))
        r["lra_low_energy"], r["lra_high_energy"] = ends
        r["loudness_range_lu"] = np.float32(ref.level(ends[1]) - ref.level(ends[0]))
    else:
        r["lra_low_energy"] = r["lra_high_energy"] = 0.0
        r["loudness_range_lu"] = np.float32(0.0)
    last_g, last_st = per[-1] if per else (np.zeros(0), np.zeros(0))
    r["momentary_energy"] = last_g[-1] if len(last_g) else 0.0
    r["short_term_energy"] = last_st[-1] if len(last_st) else 0.0
    r["max_momentary_energy"] = max([g.max() for g, _ in per if len(g)] + [0.0])
    r["max_short_term_energy"] = max([st.max() for _, st in per if len(st)] + [0.0])
    for name in ("integrated", "relative_threshold", "momentary", "short_term", "max_momentary", "max_short_term"):
        r[name + "_lufs"] = ref.lufs(r[name + "_energy"], floor)
    return r


def group_bin_clean(es, streams, B):
    """True when no bin holds blocks of the group on both sides of a relative gate of the STORED group record, for both gates
    (hr.bin_clean over G and ST): then deciding the straddling bin as a whole decides every block as the stored mode does"""
    g, st, _ = blocks(es, [(s, 0, len(es[s])) for s in streams])
    stored = results(es, [(s, 0, len(es[s])) for s in streams])
    sa = st[st > ref.ABSOLUTE_GATE]
    for z_all, threshold in ((g, stored["relative_threshold_energy"]), (st, 0.01 * sa.mean() if len(sa) else 0.0)):
        z = z_all[z_all > B[0]]
        if not len(z) or threshold <= B[0]:
            continue
        inside = z[hr.bin_of(z, B) == hr.bin_of(np.array([threshold]), B)[0]]
        if len(inside) and (inside > threshold).any() and not (inside > threshold).all():
            return False
    return True


# ---------------------------------------------------------------- inputs shared by the CPU and the GPU file: 8 kHz mono unless said
RATE, SEG = 8000.0, 800

# 1. the anchor bank: five programmes of different lengths (seed, seconds); one-member groups over whole streams and seeded parts
ANCHOR = [(11, 40.0), (12, 33.3), (13, 12.55), (14, 2.95), (15, 0.35)]
ANCHOR_SEGMENTS = [400, 333, 125, 29, 3]


def anchor_programmes():
    return [ref.programme(seed, RATE, 1, seconds) for seed, seconds in ANCHOR]


def anchor_members(segments=ANCHOR_SEGMENTS, seed=5, per_stream=8):
    """per stream: the whole of it (explicit and TO_END), the empty part at its end, and seeded parts"""
    rng = np.random.default_rng([seed, 1770])
    out = []
    for s, n in enumerate(segments):
        out += [(s, 0, n), (s, 0, TO_END), (s, n, 0), (s, n // 2, TO_END)]
        for _ in range(per_stream):
            c = int(rng.integers(0, n + 1))
            out.append((s, int(rng.integers(0, n - c + 1)), c))
    return out


# 2. the level bank: four 70 s programmes 10 dB apart, so that the album's relative gate removes blocks the members' own gates keep.
# Seeds: 21 .. 24 were the first tried and hold every condition of tests/test_cpu_program_groups.py; none was rejected.
LEVEL_SEEDS, LEVEL_GAINS_DB, LEVEL_SECONDS = (21, 22, 23, 24), (0.0, -10.0, -20.0, -30.0), 70
LEVEL_SEGMENTS = [700, 700, 700, 700]


def level_programmes():
    return [(ref.programme(seed, RATE, 1, LEVEL_SECONDS) * np.float32(10.0 ** (gain / 20.0))).astype(np.float32)
            for seed, gain in zip(LEVEL_SEEDS, LEVEL_GAINS_DB)]


# member segment counts 3, 4, 29, 30, 255, 301 and 700: the too-short cases and the lane wrap (252, 272 and 697 gating blocks)
LEVEL_MEMBERS = [(0, 0, 700), (3, 0, 700),                                                                   # 0, 1
                 (0, 10, 301), (1, 5, 255), (2, 100, 30), (3, 7, 29), (1, 300, 4), (2, 0, 3), (3, 0, 700),   # 2 .. 8
                 (1, 0, 255), (1, 255, 255), (1, 510, 190), (2, 0, 700),                                     # 9 .. 12
                 (0, 0, 3), (1, 0, 4), (2, 0, 29)]                                                           # 13 .. 15
LEVEL_GROUPS = {"loud and quiet album": (0, 2), "every length": (2, 7), "lane wrap": (9, 4), "too short for a short-term block": (13, 3),
                "the box set": (0, 16), "across two groups": (1, 2), "one short-term block": (4, 4)}
PERMUTED = "every length"
PERMUTATIONS = [(6, 5, 4, 3, 2, 1, 0), (3, 0, 6, 1, 5, 2, 4), (1, 2, 3, 4, 5, 6, 0)]


def permuted_members(order):
    first, count = LEVEL_GROUPS[PERMUTED]
    return [LEVEL_MEMBERS[first + i] for i in order]


# long groups on the level bank, around the 4096 short-term blocks from which the group kernel stages its blocks (a 700-segment member
# has 671): 4026 and 4095 below it, 4096 and 4697 at and above it, 8862 with all of the table
_SIX = [(0, 0, 700), (1, 0, 700), (2, 0, 700), (3, 0, 700), (0, 0, 700), (1, 0, 700)]
LONG_MEMBERS = _SIX + [(3, 100, 99), (3, 100, 98)] + _SIX + [(2, 0, 700)]
LONG_GROUPS = {"4026 short-term blocks": (0, 6), "4096": (0, 7), "4095": (7, 7), "4697": (8, 7), "8862": (0, 15)}
STAGING_FROM = 4096

# 4. shapes on the level bank: overlapping ranges, a duplicated member, an empty group, TO_END, a member at the end of its stream
SHAPE_MEMBERS = [(0, 0, 700), (1, 100, 301), (1, 100, 301), (2, 0, TO_END), (3, 700, 0), (3, 200, TO_END), (2, 0, 700), (3, 200, 500)]
SHAPE_GROUPS = {"single": (1, 1), "double": (1, 2), "empty": (3, 0), "empty at the table's end": (8, 0), "to end": (3, 1), "explicit": (6, 1),
                "at the end of the stream": (4, 1), "part to end": (5, 1), "part explicit": (7, 1), "overlap a": (0, 4), "overlap b": (2, 4),
                "all": (0, 8)}

# the wide call: 64 groups x 64 members on a bank of 64 streams
WIDE_STREAMS, WIDE_SEED = 64, 3
WIDE_GAINS_DB = (0.0, -12.0, -24.0)


def wide_seconds(s):
    return 6.0 + 0.37 * s      # 60 ... 293 segments


def wide_programmes():
    return [(ref.programme(300 + s, RATE, 1, wide_seconds(s)) * np.float32(10.0 ** (WIDE_GAINS_DB[s % 3] / 20.0))).astype(np.float32)
            for s in range(WIDE_STREAMS)]


def wide_call(segments, seed=WIDE_SEED):
    """(members, groups): 4096 seeded members, group k = members[64 k .. 64 k + 64)"""
    rng = np.random.default_rng([seed, 6464])
    members = []
    for _ in range(64 * 64):
        s = int(rng.integers(0, len(segments)))
        n = int(segments[s])
        c = int(rng.integers(0, n + 1)) if rng.random() < 0.7 else int(rng.integers(0, min(n, 40) + 1))
        first = int(rng.integers(0, n - c + 1))
        members.append((s, first, TO_END if rng.random() < 0.1 else c))
    return members, [(64 * k, 64) for k in range(64)]


# appended segments: two streams fed in two calls; groups with explicit counts do not move, TO_END follows
APPEND_SEEDS, APPEND_SECONDS, APPEND_CUT_SECONDS = (31, 32), 40, 30
APPEND_MEMBERS = [(0, 0, 300), (1, 50, 250), (0, 100, 100), (1, 0, TO_END)]
APPEND_GROUPS = [(0, 2), (1, 2), (0, 3), (3, 1), (2, 2)]      # the last two hold the TO_END member


def append_programmes():
    return [ref.programme(seed, RATE, 1, APPEND_SECONDS) for seed in APPEND_SEEDS]


# 5. known answers: 48 kHz stereo 1 kHz sines of 20 s, one per stream
KNOWN_RATE, KNOWN_LEVELS_DBFS = 48000.0, (-23.0, -29.0, -50.0, -20.0, -30.0)
KNOWN_MEMBERS = [(0, 0, TO_END), (1, 0, TO_END), (2, 0, TO_END), (3, 0, TO_END), (4, 0, TO_END)]
KNOWN_GROUPS = {"-23 and -29": (0, 2), "-23, -29 and -50": (0, 3), "-50 alone": (2, 1), "-20 and -30": (3, 2)}
KNOWN_ALBUM_LUFS = 10.0 * np.log10((10.0 ** -2.3 + 10.0 ** -2.9) / 2.0)      # -25.04


def known_programmes():
    return [ref.tone_programme(KNOWN_RATE, [(db, 20)]) for db in KNOWN_LEVELS_DBFS]


# 6. the bounded bank: four 40 s programmes 10 dB apart and one short stream, fed to a stored twin as well; groups of 1, 3 and all
# streams (whole streams).  The level bank's seeds 21 .. 24 were tried first and rejected: its groups (0, 2, 3) and (0, 1, 2, 3, 4) are
# not bin-clean; 41 .. 44 is the next set tried and every group below is bin-clean (tests/test_cpu_program_groups.py asserts it).
BOUNDED_SEEDS, BOUNDED_SECONDS = (41, 42, 43, 44), 40
BOUNDED_EXTRA = (25, 2.5)      # (seed, seconds): 25 segments, no short-term block
BOUNDED_SEGMENTS = [400, 400, 400, 400, 25]
BOUNDED_GROUPS = {"one": (0,), "three": (0, 2, 3), "all": (0, 1, 2, 3, 4), "all, another order": (4, 3, 1, 0, 2), "twice": (1, 1),
                  "the short one": (4,)}


def bounded_programmes():
    return [(ref.programme(seed, RATE, 1, BOUNDED_SECONDS) * np.float32(10.0 ** (gain / 20.0))).astype(np.float32)
            for seed, gain in zip(BOUNDED_SEEDS, LEVEL_GAINS_DB)] + [ref.programme(BOUNDED_EXTRA[0], RATE, 1, BOUNDED_EXTRA[1])]

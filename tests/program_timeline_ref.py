"""f64 numpy restatement of include/omx/program_timeline.h on top of tests/program_loudness_ref.py: the timeline rows (momentary,
short-term and running integrated loudness on the 100 ms grid) and the record of an interval of a programme, both from the segment
energies e[].  tests/test_cpu_program_timeline.py pins both to program_loudness_ref.results: row j is the programme e[0 .. j], an
interval is the programme e[a .. a + c)."""
import numpy as np

import program_loudness_ref as ref

ROW_FIELDS = ("integrated_energy", "relative_threshold_energy", "momentary_lufs", "short_term_lufs", "integrated_lufs",
              "gating_above_absolute", "gating_above_relative", "valid")
ROW_DTYPE = np.dtype([("integrated_energy", "<f8"), ("relative_threshold_energy", "<f8"), ("momentary_lufs", "<f4"),
                      ("short_term_lufs", "<f4"), ("integrated_lufs", "<f4"), ("gating_above_absolute", "<u4"),
                      ("gating_above_relative", "<u4"), ("valid", "<u4")])
UNCLEAN_SHARE_MAX = 0.01   # at most 1 % of the rows of a case may lie within ref.RESULT_PASS_MARGIN_MIN of a gate


def empty_row(floor=-99.9):
    r = np.zeros((), ROW_DTYPE)
    r["momentary_lufs"] = r["short_term_lufs"] = r["integrated_lufs"] = np.float32(floor)
    return r


def row_indices(first, stride, count):
    return first + stride * np.arange(count, dtype=np.int64)


class Prefixes:
    """what every row of one stream shares: the blocks, and the blocks above the absolute gate compacted in time order, so that the
    set A of row j is a prefix of `ga` (the same array contents program_loudness_ref.results forms for e[0 .. j])"""

    def __init__(self, e):
        self.e = np.asarray(e, np.float64)
        self.g, self.st = ref.sliding_mean(self.e, 4), ref.sliding_mean(self.e, 30)   # g[k - 3] is gating block k, st[k - 29] short-term block k
        ga, sa = self.g > ref.ABSOLUTE_GATE, self.st > ref.ABSOLUTE_GATE
        self.ga, self.sa = self.g[ga], self.st[sa]
        self.n_ga, self.n_sa = np.concatenate([[0], np.cumsum(ga)]), np.concatenate([[0], np.cumsum(sa)])   # blocks of A among the first m
        with np.errstate(divide="ignore"):
            self.level_ga, self.level_sa = ref.level(self.ga), ref.level(self.sa)
            dist = [np.where(b > 0.0, np.abs(ref.level(np.where(b > 0.0, b, 1.0)) - ref.level(ref.ABSOLUTE_GATE)), np.inf) for b in (self.g, self.st)]
        self.abs_margin = [np.concatenate([[np.inf], np.minimum.accumulate(d)]) for d in dist]   # over the first m blocks

    def gating(self, j):
        """A of row j, its relative gate, R"""
        ga = self.ga[:self.n_ga[max(j - 2, 0)]]
        rel = 0.1 * ga.mean() if len(ga) else 0.0
        return ga, rel, ga[ga > rel]

    def margin(self, j):
        """program_loudness_ref.results(e[:j + 1])["gate_margin"]: the smallest distance in LU between a block of e[0 .. j] and a gate
        it is compared with (both block kinds against the absolute gate, A against the relative gates of loudness and of range)"""
        mg, ms = max(j - 2, 0), max(j - 28, 0)
        out = min(self.abs_margin[0][mg], self.abs_margin[1][ms])
        ga, rel, _ = self.gating(j)
        if len(ga) and rel > 0.0:
            out = min(out, float(np.abs(self.level_ga[:len(ga)] - ref.level(rel)).min()))
        sa = self.sa[:self.n_sa[ms]]
        srel = 0.01 * sa.mean() if len(sa) else 0.0
        if len(sa) and srel > 0.0:
            out = min(out, float(np.abs(self.level_sa[:len(sa)] - ref.level(srel)).min()))
        return out


def timeline(e, first=0, stride=1, count=None, floor=-99.9):
    """rows j = first + i * stride, i < count (None: up to the last segment) of a stream whose stored energies are e"""
    p = Prefixes(e)
    n = len(p.e)
    if count is None:
        count = max((n - first + stride - 1) // stride, 0)
    out = np.zeros((count,), ROW_DTYPE)
    for i, j in enumerate(row_indices(first, stride, count)):
        j = int(j)
        if j >= n:
            out[i] = empty_row(floor)
            continue
        ga, rel, gr = p.gating(j)
        integrated = gr.mean() if len(gr) else 0.0
        out[i] = (integrated, rel, ref.lufs(p.g[j - 3], floor) if j >= 3 else np.float32(floor),
                  ref.lufs(p.st[j - 29], floor) if j >= 29 else np.float32(floor), ref.lufs(integrated, floor), len(ga), len(gr), 1)
    return out


def row_margin(e, j):
    """the gate margin of row j: that of the programme e[0 .. j]"""
    return Prefixes(e).margin(j)


def clean_rows(e, first=0, stride=1, count=None):
    """per requested row that exists: True when its gate margin reaches ref.RESULT_PASS_MARGIN_MIN"""
    p = Prefixes(e)
    n = len(p.e)
    if count is None:
        count = max((n - first + stride - 1) // stride, 0)
    return np.array([p.margin(int(j)) >= ref.RESULT_PASS_MARGIN_MIN for j in row_indices(first, stride, count) if j < n], bool)


RECORD_ENERGIES = ("integrated_energy", "relative_threshold_energy", "lra_low_energy", "lra_high_energy", "momentary_energy",
                   "short_term_energy", "max_momentary_energy", "max_short_term_energy")
RECORD_COUNTS = ("segments", "gating_blocks", "gating_above_absolute", "gating_above_relative", "short_term_blocks",
                 "short_term_above_absolute", "short_term_above_relative")
RECORD_LEVELS = ("integrated_lufs", "relative_threshold_lufs", "loudness_range_lu", "momentary_lufs", "short_term_lufs",
                 "max_momentary_lufs", "max_short_term_lufs")


def intervals(e, first, count, segment_frames=0, floor=-99.9):
    """the record of e[first .. first + count) as if it were the whole programme (dict with the field names of
    omx_program_loudness_record, plus gate_margin)"""
    e = np.asarray(e, np.float64)
    assert 0 <= first and first + count <= len(e)
    part = e[first:first + count]
    g, st = ref.sliding_mean(part, 4), ref.sliding_mean(part, 30)
    r = {"segments": count, "frames": count * segment_frames, "overflow": 0, "max_true_peak_db": np.float32(floor),
         "gating_blocks": max(count - 3, 0), "short_term_blocks": max(count - 29, 0)}
    ga = g[g > ref.ABSOLUTE_GATE]
    rel = 0.1 * ga.mean() if len(ga) else 0.0
    gr = ga[ga > rel]
    sa = st[st > ref.ABSOLUTE_GATE]
    srel = 0.01 * sa.mean() if len(sa) else 0.0
    sr = np.sort(sa[sa > srel])
    r.update(gating_above_absolute=len(ga), gating_above_relative=len(gr), short_term_above_absolute=len(sa), short_term_above_relative=len(sr),
             relative_threshold_energy=rel, integrated_energy=gr.mean() if len(gr) else 0.0,
             lra_low_energy=sr[int(np.floor((len(sr) - 1) * 0.10 + 0.5))] if len(sr) else 0.0,
             lra_high_energy=sr[int(np.floor((len(sr) - 1) * 0.95 + 0.5))] if len(sr) else 0.0,
             momentary_energy=g[-1] if len(g) else 0.0, short_term_energy=st[-1] if len(st) else 0.0,
             max_momentary_energy=g.max() if len(g) else 0.0, max_short_term_energy=st.max() if len(st) else 0.0)
    r["loudness_range_lu"] = np.float32(ref.level(r["lra_high_energy"]) - ref.level(r["lra_low_energy"])) if len(sr) else np.float32(0.0)
    for name in ("integrated", "relative_threshold", "momentary", "short_term", "max_momentary", "max_short_term"):
        r[name + "_lufs"] = ref.lufs(r[name + "_energy"], floor)
    r["gate_margin"] = min(ref._margin(g, ref.ABSOLUTE_GATE), ref._margin(st, ref.ABSOLUTE_GATE), ref._margin(ga, rel), ref._margin(sa, srel))
    return r


# ---- inputs shared by the CPU and the GPU tests
HOUR_STRIDE, FOUR_HOURS_STRIDE = 7, 60

# the 64-stream bank of the interval test: programmes of different lengths at a low rate (the intervals only read e[])
INTERVAL_RATE, INTERVAL_STREAMS, INTERVAL_SEED, INTERVALS_PER_STREAM = 8000.0, 64, 0, 62
EDGE_LENGTHS = (0, 1, 3, 4, 29, 30)


def interval_bank_seconds(s):
    return 20.0 + 1.7 * s       # 200 ... 1271 segments


def interval_bank_programme(s):
    return ref.programme(100 + s, INTERVAL_RATE, 1, interval_bank_seconds(s))


def draw_intervals(segments, seed=INTERVAL_SEED, per_stream=INTERVALS_PER_STREAM):
    """(stream, first, count) for a bank whose streams hold `segments`: per stream the edge lengths at the first and at the last
    segment, the whole stream, and seeded intervals of every length; about 64 x 62 = 4000 in all"""
    rng = np.random.default_rng([seed, 77])
    out = []
    for s, n in enumerate(segments):
        n = int(n)
        mine = [(s, 0, n)]
        for c in EDGE_LENGTHS:
            if c <= n:
                mine += [(s, 0, c), (s, n - c, c)]
        while len(mine) < per_stream:
            c = int(rng.integers(0, n + 1)) if rng.random() < 0.5 else int(rng.integers(0, min(n, 120) + 1))
            mine.append((s, int(rng.integers(0, n - c + 1)), c))
        out += mine
    return out


# banks of 1, 5 and 65 streams whose streams hold 0, 1, 3, 4, 29, 30 and a few hundred segments (half a segment more, left open)
EDGE_RATE = 8000.0
EDGE_SEGMENTS = (350, 0, 1, 3, 4, 29, 30, 211, 487)
EBU_THROUGH_THE_PRODUCT = ("3341-3", "3341-4", "3342-1")


def edge_programmes(n_streams):
    return [ref.programme(200 + s, EDGE_RATE, 1, EDGE_SEGMENTS[s % len(EDGE_SEGMENTS)] / 10.0 + 0.05) for s in range(n_streams)]

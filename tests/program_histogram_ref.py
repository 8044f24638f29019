"""f64 numpy restatement of the programme bank's bounded storage (include/omx/program_histogram.h) on top of
program_loudness_ref: the histograms of the gating and short-term blocks of stored segment energies e[], and the record made from
them.  Every sum follows the definition's order literally (np.add.at adds in index order; np.cumsum adds ascending), so the f64
fields are meant to equal the product's bit for bit.  The boundaries B always come from the library
(openmeters_amd.histogram_boundaries), never from an expression of this file.  Also the inputs shared by the CPU and GPU tests."""
import numpy as np

import program_loudness_ref as ref

BINS, TAIL = 1000, 29
LRA_BOUND_LU = 0.2   # against the stored mode: each range end is the mean of the bin (0.1 LU wide) that holds the true rank element
RECORD_ENERGIES = ("integrated_energy", "relative_threshold_energy", "lra_low_energy", "lra_high_energy", "momentary_energy",
                   "short_term_energy", "max_momentary_energy", "max_short_term_energy")
RECORD_COUNTS = ("segments", "gating_blocks", "gating_above_absolute", "gating_above_relative", "short_term_blocks",
                 "short_term_above_absolute", "short_term_above_relative")
RECORD_LEVELS = ("integrated_lufs", "relative_threshold_lufs", "loudness_range_lu", "momentary_lufs", "short_term_lufs",
                 "max_momentary_lufs", "max_short_term_lufs")


def numpy_boundaries():
    """the header's expression in numpy (what the library's table is compared with, not what anything bins with)"""
    return np.power(10.0, (-70.0 + 0.691 + np.arange(BINS + 1) / 10.0) / 10.0)


def bin_of(z, B):
    """bins of the blocks z (all > B[0]): the largest i <= 999 with B[i] < z"""
    return np.searchsorted(B[:BINS], z, side="left") - 1


def fold(blocks, B):
    """(count[1000] u64, sum[1000] f64) of the blocks above B[0], added in ascending j"""
    count, total = np.zeros(BINS, np.uint64), np.zeros(BINS, np.float64)
    z = blocks[blocks > B[0]]
    if len(z):
        i = bin_of(z, B)
        assert i.min() >= 0 and i.max() < BINS
        np.add.at(count, i, np.uint64(1))
        np.add.at(total, i, z)
    return count, total


def histogram(e, B):
    """omx_program_histogram of a stream whose segment energies since the last reset are e"""
    e = np.asarray(e, np.float64)
    g, st = ref.sliding_mean(e, 4), ref.sliding_mean(e, 30)
    gc, gs = fold(g, B)
    sc, ss = fold(st, B)
    return {"gating_count": gc, "gating_sum": gs, "short_term_count": sc, "short_term_sum": ss, "tail": e[max(len(e) - TAIL, 0):].copy(),
            "segments": len(e)}


def ascending_sum(v):
    return np.cumsum(v)[-1] if len(v) else v.dtype.type(0)


def gate(count, total, factor):
    """(threshold, passing bins) of one histogram"""
    n = int(ascending_sum(count))
    threshold = factor * (ascending_sum(total) / np.float64(n)) if n else 0.0
    with np.errstate(all="ignore"):
        passing = (count != 0) & (total / count.astype(np.float64) > threshold)
    return n, threshold, passing


def results(e, B, floor=-99.9):
    """the record of a bounded stream (the fields of omx_program_loudness_record but frames, overflow and max_true_peak_db)"""
    e = np.asarray(e, np.float64)
    h = histogram(e, B)
    g, st = ref.sliding_mean(e, 4), ref.sliding_mean(e, 30)
    r = {"segments": len(e), "gating_blocks": len(g), "short_term_blocks": len(st), "histogram": h}
    n, threshold, passing = gate(h["gating_count"], h["gating_sum"], 0.1)
    r["gating_above_absolute"], r["relative_threshold_energy"] = n, threshold
    # (the sums of the passing bins: zeros elsewhere add nothing and change no bit)
    pc = int(ascending_sum(np.where(passing, h["gating_count"], np.uint64(0))))
    r["gating_above_relative"] = pc
    r["integrated_energy"] = ascending_sum(np.where(passing, h["gating_sum"], 0.0)) / np.float64(pc) if pc else 0.0
    n, _, passing = gate(h["short_term_count"], h["short_term_sum"], 0.01)
    r["short_term_above_absolute"] = n
    counts = np.where(passing, h["short_term_count"], np.uint64(0))
    pc = int(ascending_sum(counts))
    r["short_term_above_relative"] = pc
    if pc:
        upto = np.cumsum(counts)
        ends = []
        for q in (0.10, 0.95):
            rank = int(np.floor((np.float64(pc) - 1.0) * q + 0.5))
            i = int(np.searchsorted(upto, rank, side="right"))   # the first bin whose cumulative count exceeds the rank
            ends.append(h["short_term_sum"][i] / np.float64(h["short_term_count"][i]))
        r["lra_low_energy"], r["lra_high_energy"] = ends
        r["loudness_range_lu"] = np.float32(ref.level(ends[1]) - ref.level(ends[0]))
    else:
        r["lra_low_energy"] = r["lra_high_energy"] = 0.0
        r["loudness_range_lu"] = np.float32(0.0)
    r["momentary_energy"] = g[-1] if len(g) else 0.0
    r["short_term_energy"] = st[-1] if len(st) else 0.0
    r["max_momentary_energy"] = g.max() if len(g) else 0.0
    r["max_short_term_energy"] = st.max() if len(st) else 0.0
    for name in ("integrated", "relative_threshold", "momentary", "short_term", "max_momentary", "max_short_term"):
        r[name + "_lufs"] = ref.lufs(r[name + "_energy"], floor)
    return r


def bin_clean(e, B):
    """True when no bin holds blocks on both sides of a relative gate of the stored mode (ref.results), for both gates: then deciding
    the straddling bin as a whole decides every block as the stored mode does"""
    e = np.asarray(e, np.float64)
    stored = ref.results(e)
    for blocks, threshold in ((ref.sliding_mean(e, 4), stored["relative_threshold_energy"]),
                              (ref.sliding_mean(e, 30), short_term_threshold(e))):
        z = blocks[blocks > B[0]]
        if not len(z) or threshold <= B[0]:
            continue
        inside = z[bin_of(z, B) == bin_of(np.array([threshold]), B)[0]]
        if len(inside) and (inside > threshold).any() and not (inside > threshold).all():
            return False
    return True


def short_term_threshold(e):
    st = ref.sliding_mean(np.asarray(e, np.float64), 30)
    sa = st[st > ref.ABSOLUTE_GATE]
    return 0.01 * sa.mean() if len(sa) else 0.0


# ---- inputs shared by tests/test_cpu_program_histogram.py and tests/test_gpu_program_histogram.py
EDGE_RATE = 8000.0      # mono, 800 frames per segment
EDGE_SEG = 800
CUT_SEED, CUT_SECONDS = 1, 40
LONG_SECONDS = 1200     # ref.hour_programme(kind, seconds=LONG_SECONDS, seed=LONG_SEEDS[kind]): 12 000 segments
# seed 0 of "steps" is not bin-clean (two short-term blocks of 5334 share the straddling bin with blocks on the other side of the gate,
# and so are seeds 1 .. 14); seed 15 is the first that is (tests/test_cpu_program_histogram.py asserts it)
LONG_SEEDS = {"tone": 0, "steps": 15}
RAGGED_SEGMENTS = (0, 2, 3, 31, 400)
RAGGED_SEEDS = (1, 2, 3, 4, 5)
RAGGED_RESET_STREAM, RAGGED_RESET_AT = 4, 170 * EDGE_SEG + 123   # stream 4 starts over in the middle of a segment
OVERFLOW_SEED, OVERFLOW_SECONDS, OVERFLOW_CAPACITY = 6, 60, 20
EBU_THROUGH_THE_PRODUCT = ("3341-3", "3342-3")


def long_programme(kind):
    return ref.hour_programme(kind, seconds=LONG_SECONDS, seed=LONG_SEEDS[kind])


def cut_programme():
    return ref.programme(CUT_SEED, EDGE_RATE, 1, CUT_SECONDS)


def cut_schedules(frames):
    """name -> list of call lengths that add up to `frames`"""
    def chunks(sizes, total=frames):
        out, k = [], 0
        while total:
            out.append(min(sizes[k % len(sizes)], total))
            total -= out[-1]
            k += 1
        return out
    return {"one call": [frames], "256 frames": chunks([256]), "799 / 800 / 801": chunks([799, 800, 801]),
            "3, 4, 29, 30, 31 segments": chunks([EDGE_SEG * n for n in (3, 4, 29, 30, 31)]), "1 frame first": [1] + chunks([4096], frames - 1)}


def ragged_programmes():
    return [ref.programme(seed, EDGE_RATE, 1, 40)[:n * EDGE_SEG + (17 if n else 0)] for seed, n in zip(RAGGED_SEEDS, RAGGED_SEGMENTS)]


def bank_programmes(n_streams):
    """banks of 3 and 65 streams: the ragged programmes in turn"""
    pool = ragged_programmes()
    return [pool[(s + 1) % len(pool)] for s in range(n_streams)]


def sine(amplitude, seconds, fs=EDGE_RATE, freq=1000.0):
    return (amplitude * np.sin(2 * np.pi * freq * np.arange(int(fs * seconds)) / fs)).astype(np.float32)[:, None]


def range_programmes():
    """name -> 8 kHz mono programme for the ends of the bins' range"""
    return {"top bin": sine(64.0, 5), "below the gate": sine(1e-4, 5), "equal blocks": sine(0.1, 300),
            "silence, then a tone": np.concatenate([np.zeros((int(EDGE_RATE * 4), 1), np.float32), sine(0.1, 6)])}


def overflow_programme():
    return ref.programme(OVERFLOW_SEED, EDGE_RATE, 1, OVERFLOW_SECONDS)


def edge_inputs():
    """every 8 kHz mono input of the GPU file but the long ones: (tag, x)"""
    out = [("cut", cut_programme()), ("overflow", overflow_programme())]
    out += [(("ragged", s), x) for s, x in enumerate(ragged_programmes())]
    x = ragged_programmes()[RAGGED_RESET_STREAM]
    out += [("ragged, after the reset", x[RAGGED_RESET_AT:])]
    out += [(("range", name), x) for name, x in range_programmes().items()]
    return out

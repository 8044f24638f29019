/* Programme loudness bank, bounded storage: a second storage mode for programmes without an end.
 *
 * A bank made by omx_program_loudness_bank_create (include/omx/program_loudness.h) stores one f64 per 100 ms segment in an array
 * sized at creation; a full stream sets `overflow` and takes no more samples.  A bank made by
 * omx_program_loudness_bank_create_bounded keeps, per stream, a histogram of its gating blocks and one of its short-term blocks
 * (1000 bins of 0.1 LU from the absolute gate upwards), the newest 29 segment energies and its running maxima: about 32 KB whatever
 * the length, a result pass that costs the same at any length, and no overflow.
 *
 * DEFINITIONS ("Bounded storage"; tests/program_histogram_ref.py restates them)
 *   Segment energies e[j], gating blocks g[j] (j >= 3) and short-term blocks st[j] (j >= 29) are those of the stored mode: the same
 *   segment pass, the same expression for a block, oldest segment first.
 *   B[i] = pow(10, (-70 + 0.691 + i / 10.0) / 10), i = 0 .. 1000, in f64; B[0] is the absolute gate.
 *   Binning: a block of energy z is binned when z > B[0]; its bin is the largest i <= 999 with B[i] < z (bin i is (B[i], B[i+1]],
 *   the top bin is open above).  Binning adds 1 to the bin's count and z to the bin's sum.  Additions into one bin happen in
 *   ascending j, within a call and across calls, in f64 without fused multiply-add: with the reference-order segment pass the
 *   histogram has the same bits however the programme is cut into calls.
 *   Record (the layout of omx_program_loudness_record):
 *     frames, segments, gating_blocks, short_term_blocks: the running counts.  overflow: 0.
 *     gating_above_absolute     = sum of gating_count[i]
 *     relative_threshold_energy = 0.1 * (sum of gating_sum[i]) / (sum of gating_count[i]), both sums over ascending i
 *     bin i passes the relative gate when it is not empty and gating_sum[i] / gating_count[i] > that threshold
 *     gating_above_relative     = sum of the counts of the passing bins
 *     integrated_energy         = (sum of the sums) / (sum of the counts) of the passing bins, ascending i
 *     loudness range: the same on the short-term histogram with the factor 0.01; n = the count in the passing bins; the ranks
 *       floor((n - 1) * 0.10 + 0.5) and floor((n - 1) * 0.95 + 0.5) are located in the cumulative counts of the passing bins;
 *       lra_low_energy / lra_high_energy = sum / count of the bins those ranks fall in (each within 0.1 LU of the rank element).
 *     latest and maximum momentary / short-term energies: kept exactly as blocks complete.
 *     dB fields, the floor and max_true_peak_db as in the stored mode; no passing block: integrated = the floor, range = 0.
 *   Every block that is certainly above or below a gate is treated as in the stored mode; only the one bin that straddles a relative
 *   gate is decided as a whole, by its mean.
 *
 * Everything else on a bounded bank goes through the functions of program_loudness.h and program_peaks.h, unchanged: process
 * (ragged counts, reset masks, both kernel forms), reset, note_snapshots, results, fetch, set_peaks / peaks / fetch_peaks.
 * What needs the stored segments returns OMX_ERR_UNSUPPORTED on a bounded bank and changes nothing: fetch_segments, timeline,
 * fetch_timeline, measure_intervals, fetch_intervals. */
#ifndef OMX_PROGRAM_HISTOGRAM_H
#define OMX_PROGRAM_HISTOGRAM_H

#include "program_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_PROGRAM_HISTOGRAM_BINS 1000
#define OMX_PROGRAM_HISTOGRAM_TAIL 29

/* B[0 .. 1000]: B[i] = pow(10, (-70 + 0.691 + i / 10.0) / 10), in f64.
 * B[0] is, bit for bit, the absolute gate of the result pass.
 * Pure host function: needs no device. */
int omx_program_histogram_boundaries(double dst[OMX_PROGRAM_HISTOGRAM_BINS + 1]);

/* A programme loudness bank with bounded storage.  No capacity argument:
 * the stream never fills, `overflow` stays 0. */
int omx_program_loudness_bank_create_bounded(const omx_loudness_config* cfg, uint32_t n_streams,
                                             uint32_t channels, omx_program_loudness_bank** out);

int omx_program_loudness_bank_is_bounded(const omx_program_loudness_bank* b);   /* 1 / 0 */

typedef struct omx_program_histogram {
    uint64_t gating_count[OMX_PROGRAM_HISTOGRAM_BINS];
    double   gating_sum[OMX_PROGRAM_HISTOGRAM_BINS];       /* sum of the block energies binned here */
    uint64_t short_term_count[OMX_PROGRAM_HISTOGRAM_BINS];
    double   short_term_sum[OMX_PROGRAM_HISTOGRAM_BINS];
    double   tail[OMX_PROGRAM_HISTOGRAM_TAIL];             /* the newest segment energies, oldest first */
    uint64_t segments;                                     /* completed since the last reset */
    uint32_t tail_count, _pad;                             /* min(segments, 29) */
} omx_program_histogram;

/* Copy of one stream's histogram; synchronises.  OMX_ERR_INVALID on a bank that is not bounded. */
int omx_program_loudness_bank_fetch_histogram(omx_program_loudness_bank* b, uint64_t stream_index,
                                              omx_program_histogram* dst);

#ifdef __cplusplus
}
#endif
#endif

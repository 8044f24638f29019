/* Programme loudness bank, peaks: maximum true peak and maximum sample peak of every stream, measured by the bank itself on the PCM
 * that omx_program_loudness_bank_process takes.  With them a host gets the four EBU R 128 figures (integrated loudness, loudness
 * range, maximum momentary / short-term loudness, maximum true peak) from process + fetch, without a second bank.
 *
 * Additive: this header adds three functions and one record to include/omx/program_loudness.h; nothing declared there changes and
 * OMX_ABI_VERSION stays as it is.  Peaks are OFF by default: a bank that never calls set_peaks launches and allocates nothing more.
 *
 * DEFINITION ("Programme loudness bank", peaks)
 *   For stream s and channel c let x[0 .. N) be the samples taken since the last reset — exactly the frames the segment pass took,
 *   so they stop where `overflow` stops them — and x[n] = 0 for n < 0.  fs is the sanitised rate, compared in f64.
 *     fs <  96000          : o_p[n] = sum_{i = 0 .. 11} x[n - i] * fir4[i][p], p = 0, 1, 2;  fir4[t][p] = true_peak_coefficient(4 t + p + 1, 4)
 *     96000 <= fs < 192000 : o_0[n] = sum_{i = 0 .. 23} x[n - i] * fir2[i];                  fir2[t]    = true_peak_coefficient(2 t + 1, 2)
 *     fs >= 192000         : no interpolated outputs
 *   true_peak_coefficient(j, factor) = (float)(hann(j) * sin(x) / x), x = (j - 24) * pi / factor, hann(j) = 0.5 (1 - cos(2 pi j / 48)),
 *   in f64.  Every sum is f32 in the order i = 0, 1, ...; every product is rounded before it is added (no fused multiply-add).
 *     v[n]         = max(|x[n]|, |o_p[n]| ...), max ignoring NaN operands (fmaxf)
 *     true_peak    = max_n v[n], starting from 0;      sample_peak = max_n |x[n]|
 *     true_peak_frame = the smallest n with v[n] == true_peak, 0 when the peak is 0; sample_peak_frame likewise
 *     dB fields    = power_to_db(p * p, floor_db): p * p > 0 ? max(logf(p * p) * 4.3429448f, floor_db) : floor_db
 *   So a NaN sample adds nothing to either peak for its own frame and the next 11 / 23, and an infinite sample makes the peak infinite.
 *   This is the reference's sample-by-sample meter run over the whole programme; the result does not depend, in any bit, on how the
 *   programme is cut into calls. */
#ifndef OMX_PROGRAM_PEAKS_H
#define OMX_PROGRAM_PEAKS_H

#include "program_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omx_program_peak_record {
    uint64_t frames;                               /* = omx_program_loudness_record.frames */
    uint64_t true_peak_frame[OMX_MAX_CHANNELS];    /* frames since the last reset */
    uint64_t sample_peak_frame[OMX_MAX_CHANNELS];
    float true_peak[OMX_MAX_CHANNELS];             /* linear; 0 for slots at or above `channels` */
    float sample_peak[OMX_MAX_CHANNELS];
    float true_peak_db[OMX_MAX_CHANNELS];          /* floor_db for unused slots */
    float sample_peak_db[OMX_MAX_CHANNELS];
    float max_true_peak_db, max_sample_peak_db;    /* over the channels below `channels` */
    uint32_t max_true_peak_channel;                /* lowest index on a tie */
    uint32_t oversampling;                         /* 4, 2 or 1; 0 until the stream takes a sample (and again after a reset) */
    uint32_t channels, _pad;                       /* channel count of the programme; 0 until the stream takes a sample */
} omx_program_peak_record;                         /* 288 bytes */

/* on != 0: process also measures the peaks (one time-parallel pass over the PCM of the call and one small fold, on the caller's
 * stream, after the segment pass); 0: as a bank without this header.  Allowed only while no stream holds samples (a new bank, or
 * every stream reset): otherwise OMX_ERR_INVALID and nothing changes.
 * With peaks on, omx_program_loudness_record.max_true_peak_db is the larger of what omx_program_loudness_bank_note_snapshots folded
 * and the max_true_peak_db measured here.  omx_program_loudness_bank_reset and a call's reset_mask clear the peaks, the frame numbers
 * and the carried filter history of the flagged streams. */
int omx_program_loudness_bank_set_peaks(omx_program_loudness_bank* b, uint32_t on);
/* *d_records: device array [n_streams], valid until the next call on the bank; it is written by the process calls, so work on `stream`
 * that reads it has to be ordered behind them.  OMX_ERR_INVALID with peaks off. */
int omx_program_loudness_bank_peaks(omx_program_loudness_bank* b, void* stream, const omx_program_peak_record** d_records);
/* Copy of one stream's record, synchronises.  OMX_ERR_INVALID with peaks off or an index out of range. */
int omx_program_loudness_bank_fetch_peaks(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_peak_record* dst);

#ifdef __cplusplus
}
#endif
#endif

/* Programme loudness bank, timeline and intervals: loudness over time on the 100 ms grid (momentary, short-term and running integrated
 * loudness: the "M / S / I" log of a loudness meter) and the programme record of any part of a programme (a spot, a reel, a chapter,
 * "the last ten minutes").  Both are pure functions of the segment energies e[] the bank already stores: no PCM is read again, and
 * in the reference-order form e[] — hence every figure here — does not depend on how the programme was cut into calls.
 *
 * Additive: this header adds four functions and two structures to include/omx/program_loudness.h; nothing declared there or in
 * program_peaks.h changes and OMX_ABI_VERSION stays as it is.  A bank that never calls one of them launches and allocates nothing more.
 *
 * DEFINITIONS ("Programme loudness bank", timeline and intervals), on top of those of program_loudness.h: g[k], the gating
 * block, for k >= 3; st[k], the short-term block, for k >= 29; the absolute gate; L(z); lufs(z) = mean_square_to_lufs with the
 * configured floor.
 *
 *   TIMELINE ROW j of stream s, 0 <= j < segments[s]: the programme as it stood at the end of segment j.
 *     momentary_lufs  = lufs(g[j]), the floor for j < 3;   short_term_lufs = lufs(st[j]), the floor for j < 29
 *     running integrated loudness = the integrated loudness of e[0 .. j]:
 *       A = {k : 3 <= k <= j, g[k] > absolute gate}
 *       relative_threshold_energy = 0.1 * mean(A), 0 when A is empty
 *       R = {k in A : g[k] > relative_threshold_energy}
 *       integrated_energy = mean(R), 0 when R is empty;  integrated_lufs = lufs(integrated_energy)
 *       gating_above_absolute = |A|;  gating_above_relative = |R|
 *     valid = 1
 *   A requested row with j >= segments[s] (a shorter stream of a ragged bank, a stream after its reset) is the EMPTY ROW: valid 0, the
 *   three dB fields at the floor, everything else 0.
 *   Sums are f64.  mean(A) is a blocked prefix sum whose order depends on k alone, mean(R) adds the blocks in ascending k: row j has
 *   the same bits through whichever (first, stride, count) it is asked for, and before and after later calls appended segments.
 *   Loudness range over time is not a field (two order statistics per row): ask for prefix intervals at the instants wanted.
 *
 *   INTERVAL RECORD: the omx_program_loudness_record of e[first_segment .. first_segment + segment_count) of one stream, by the result
 *   pass's own definitions (and its own code), as if that were the whole programme.
 *     segments = segment_count;  frames = segment_count * the segment length in frames;  overflow = 0
 *     max_true_peak_db = the floor: the peak records have no time axis, so a part of a programme has no peak of its own here
 *       (program_peak_timeline.h measures the peaks of an interval).
 *   A count of 0, or fewer than 4 / 30 segments, gives the empty fields a young stream has.  The interval [0, segments[s]) has the
 *   bits of omx_program_loudness_bank_fetch(s) in every field but frames, overflow and max_true_peak_db. */
#ifndef OMX_PROGRAM_TIMELINE_H
#define OMX_PROGRAM_TIMELINE_H

#include "program_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omx_program_timeline_row {
    double integrated_energy;          /* mean of the gating blocks k <= j above both gates */
    double relative_threshold_energy;  /* 0.1 * mean of the gating blocks k <= j above the absolute gate */
    float momentary_lufs;
    float short_term_lufs;
    float integrated_lufs;
    uint32_t gating_above_absolute;
    uint32_t gating_above_relative;
    uint32_t valid;                    /* 1: segment j is stored; 0: the empty row */
} omx_program_timeline_row;            /* 40 bytes */

typedef struct omx_program_interval {
    uint32_t stream;
    uint32_t _pad;
    uint64_t first_segment;
    uint64_t segment_count;
} omx_program_interval;                /* 24 bytes */

/* Rows j = first + i * stride, i < count, of EVERY stream into the caller's device buffer d_rows [n_streams][count], enqueued on
 * `stream`.  stride >= 1.  count == 0: OMX_NONE, nothing is written.  OMX_ERR_INVALID: a null d_rows with count > 0, stride == 0,
 * first + (count - 1) * stride beyond 64 bits, n_streams * count beyond 2^32 - 1, a bank of more than 65535 streams (the launch carries
 * the stream in a grid dimension of 16 bits; omx_program_loudness_bank_fetch_timeline serves such a bank stream by stream).
 * Otherwise OMX_PRODUCED.
 * Cost and footprint: the first call allocates 20 bytes of scratch per stream and block up to the largest j asked for (2.5 times the
 * stored e[] of that range: 23 MB for 8 streams x 4 h), grow-only and kept until the bank is destroyed; every call scans each stream
 * from block 0 to its last j again (0.3 ms for 4 h), also for a short window at the end, and the all-pairs work of row j grows with j. */
int omx_program_loudness_bank_timeline(omx_program_loudness_bank* b, uint64_t first, uint64_t stride, uint64_t count,
                                       omx_program_timeline_row* d_rows, void* stream);
/* The same rows of one stream into host memory dst [count]; synchronises.  Also OMX_ERR_INVALID: stream_index out of range. */
int omx_program_loudness_bank_fetch_timeline(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t stride,
                                             uint64_t count, omx_program_timeline_row* dst);
/* intervals: host array [n].  *d_records: device array [n], written on `stream`, valid until the next call on the bank.
 * OMX_ERR_INVALID: a stream index out of range, first_segment + segment_count > segments[stream], a null array with n > 0, a null
 * d_records (also with n == 0), more than 2^31 - 1 intervals.
 * n == 0: OMX_NONE.  Otherwise OMX_PRODUCED. */
int omx_program_loudness_bank_measure_intervals(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                void* stream, const omx_program_loudness_record** d_records);
/* Measures, copies to dst [n] (host) and synchronises. */
int omx_program_loudness_bank_fetch_intervals(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                              omx_program_loudness_record* dst);
/* A refused call changes nothing: neither the bank's state nor what an earlier call returned. */

#ifdef __cplusplus
}
#endif
#endif

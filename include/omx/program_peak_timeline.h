/* Programme loudness bank, peak timeline: true peak and sample peak over time on the bank's own 100 ms grid, for any part of a
 * programme and for groups of parts ("where does the programme exceed -1 dBTP", the true peak of a spot, a reel or a chapter, an album
 * gain for tracks cut out of one long capture that is not held down by peaks outside them).  program_peaks.h keeps one figure per
 * stream since the last reset; with this header the peak pass also keeps a maximum per segment, and everything here is made from
 * those: no PCM is read again.
 *
 * Additive: this header adds two structures and eight functions; nothing declared in program_loudness.h, program_peaks.h,
 * program_timeline.h, program_groups.h or program_normalize.h changes and OMX_ABI_VERSION stays as it is.  The timeline is OFF by
 * default: a bank that never calls set_peak_timeline allocates and launches nothing more, and every record of the other headers keeps
 * its bytes whether the timeline is on or off (the interval and group LOUDNESS records still carry max_true_peak_db = the floor).
 *
 * DEFINITION ("Peak timeline"; tests/program_peak_timeline_ref.py restates it frame by frame), with x, o_p,
 * v[n] and N (frames taken since the last reset: they stop where `overflow` stops them) of program_peaks.h and the segment length
 * L = ((uint32_t)fs + 5) / 10 frames of program_loudness.h:
 *   PEAK SEGMENT j covers the frames [j L, min((j + 1) L, N)) and exists when it holds at least one frame: there are ceil(N / L) of
 *   them, and the last one may be open (fewer than L frames so far).  Per channel:
 *     true_peak[j]   = max v[n] over the segment's frames, starting from 0;     sample_peak[j] = max |x[n]| likewise
 *   with the fmaxf semantics of program_peaks.h (a NaN adds nothing, an infinity makes the peak infinite), each with the offset, in
 *   frames from the segment's first frame, of the first frame that reaches it; the offset is 0 when the peak is 0.
 *   FILTER HISTORY.  The interpolator's history is the programme's: v[n] near the start of segment j depends on the last 11 (4x) or
 *   23 (2x) frames of segment j - 1.  So the peak of a part is the peak of the PROGRAMME DURING that part, not the peak of the excerpt
 *   measured from silence: an impulse on the last frame of a segment leaves its interpolated tail in the next segment's true peak
 *   (and nothing in its sample peak).
 *   ROW i of (first, stride, count) is the maximum over the segments [first + i stride, first + (i + 1) stride) that exist: an
 *   aggregate, so stride = 10 gives a peak log per second.  Among equal values the earlier frame wins.  Offsets count from the row's
 *   first frame, (first + i stride) L.  frames = the frames the row covers; valid = 0 when none of its segments exists, and then every
 *   other field is 0.  Channels at or above the programme's channel count read 0.
 *   INTERVAL PEAK of an omx_program_interval {stream, first_segment, segment_count}: the same maximum over the STORED (complete)
 *   segments [first_segment, first_segment + segment_count) of the stream, the frames the interval's loudness record covers; frame
 *   numbers count from the stream's last reset.  segment_count == OMX_PROGRAM_TO_END: up to the last stored segment.
 *   GROUP PEAK of members / groups tables as in program_groups.h: the maximum over the group's members.  Among equal values the first
 *   member in table order wins, within it the earliest frame; *_member is that member's index relative to the group's first member.
 *   frames = the sum over the members.  A group of one member has the bytes of that member's interval peak.  An empty group, or a
 *   part without frames: peaks 0, dB fields at the floor, channels 0.
 *   dB fields = power_to_db(p * p, floor_db) as in program_peaks.h; max_* over the channels below `channels`, the lowest channel on a
 *   tie.
 *   IDENTITY.  For every stream and channel the larger of interval [0, segments) and the open row (first = segments, stride 1) —
 *   the interval on equality — equals omx_program_loudness_bank_fetch_peaks in value and in frame number.
 *   Every figure is a maximum of the per-frame values the peak pass forms anyway, kept with integer maximum operations: the bits do
 *   not depend on how the programme is cut into calls.  Peaks folded by note_snapshots are not part of the timeline.
 *
 * STORAGE.  16 bytes per channel and segment of capacity, [n_streams][capacity_seconds * 10 + 1][channels]: a stereo day is 28 MB per
 * stream.  Reserved (grow-only, kept until the timeline is switched off) by the first process call that brings frames.  A reset of a
 * stream clears what it had stored, at a cost proportional to that. */
#ifndef OMX_PROGRAM_PEAK_TIMELINE_H
#define OMX_PROGRAM_PEAK_TIMELINE_H

#include "program_normalize.h"
#include "program_peaks.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omx_program_peak_row {
    float true_peak[OMX_MAX_CHANNELS];             /* offset   0: linear */
    float sample_peak[OMX_MAX_CHANNELS];           /* offset  32 */
    uint32_t true_peak_offset[OMX_MAX_CHANNELS];   /* offset  64: frames from the row's first frame; 0 for a peak of 0 */
    uint32_t sample_peak_offset[OMX_MAX_CHANNELS]; /* offset  96 */
    uint32_t frames;                               /* offset 128: frames the row covers (stride * L for a row of complete segments) */
    uint32_t valid;                                /* offset 132: 0: none of the row's segments exists, everything else is 0 */
} omx_program_peak_row;                            /* 136 bytes */

typedef struct omx_program_part_peak {
    uint64_t frames;                               /* offset   0: frames covered, summed over the members */
    uint64_t true_peak_frame[OMX_MAX_CHANNELS];    /* offset   8: frames since the stream's last reset */
    uint64_t sample_peak_frame[OMX_MAX_CHANNELS];  /* offset  72 */
    uint32_t true_peak_member[OMX_MAX_CHANNELS];   /* offset 136: index relative to the group's first member; 0 for an interval */
    uint32_t sample_peak_member[OMX_MAX_CHANNELS]; /* offset 168 */
    float true_peak[OMX_MAX_CHANNELS];             /* offset 200: linear; 0 for slots at or above `channels` */
    float sample_peak[OMX_MAX_CHANNELS];           /* offset 232 */
    float true_peak_db[OMX_MAX_CHANNELS];          /* offset 264: floor_db for unused slots */
    float sample_peak_db[OMX_MAX_CHANNELS];        /* offset 296 */
    float max_true_peak_db, max_sample_peak_db;    /* offset 328, 332: over the channels below `channels` */
    uint32_t max_true_peak_channel;                /* offset 336: lowest index on a tie */
    uint32_t channels;                             /* offset 340: the programme's channel count; 0 for a part without frames */
} omx_program_part_peak;                           /* 344 bytes */

/* on != 0: the peak pass of process also keeps the per-segment maxima; 0: as a bank without this header, and the storage is freed.
 * OMX_ERR_INVALID, with nothing changed: peaks are off (omx_program_loudness_bank_set_peaks first), or a stream holds samples (reset
 * every stream first).  OMX_ERR_UNSUPPORTED: a bank with bounded storage (program_histogram.h), which has no time axis.
 * omx_program_loudness_bank_set_peaks(b, 0) on a bank with the timeline on also switches the timeline off. */
int omx_program_loudness_bank_set_peak_timeline(omx_program_loudness_bank* b, uint32_t on);

/* Rows i < count of EVERY stream into the caller's device buffer d_rows [n_streams][count], enqueued on `stream`.  stride >= 1.
 * count == 0: OMX_NONE, nothing is written.  OMX_ERR_INVALID, with nothing written: the timeline is off, a null d_rows, stride == 0,
 * stride * L beyond 2^32 - 1, first + (count - 1) * stride beyond 64 bits, count beyond 2^31 - 257 (the rows of one stream in one
 * launch), n_streams * count beyond 2^32 - 1, a bank of more than 65535 streams (fetch_peak_rows serves such a bank stream by
 * stream).  Otherwise OMX_PRODUCED.  A row of complete segments keeps its bytes through later appends. */
int omx_program_loudness_bank_peak_rows(omx_program_loudness_bank* b, uint64_t first, uint64_t stride, uint64_t count,
                                        omx_program_peak_row* d_rows, void* stream);
/* The same rows of one stream into host memory dst [count]; synchronises, with the same limits on first, stride and count (n_streams
 * counts as 1).  Also OMX_ERR_INVALID: stream_index out of range. */
int omx_program_loudness_bank_fetch_peak_rows(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t stride,
                                              uint64_t count, omx_program_peak_row* dst);

/* intervals: host array [n].  *d_peaks: device array [n], written on `stream`, valid until the next call on the bank.
 * OMX_ERR_INVALID, with nothing changed: the timeline is off; and as omx_program_loudness_bank_measure_intervals: a stream index out
 * of range, first_segment + segment_count > segments[stream] (for a count other than OMX_PROGRAM_TO_END), a null array with n > 0, a
 * null d_peaks, more than 2^31 - 1 intervals.  n == 0: OMX_NONE.  Otherwise OMX_PRODUCED. */
int omx_program_loudness_bank_measure_interval_peaks(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                     void* stream, const omx_program_part_peak** d_peaks);
/* Measures, copies to dst [n] (host) and synchronises.  Also OMX_ERR_INVALID: a null dst with n > 0. */
int omx_program_loudness_bank_fetch_interval_peaks(omx_program_loudness_bank* b, const omx_program_interval* intervals, uint64_t n,
                                                   omx_program_part_peak* dst);
/* members, groups: host tables as for omx_program_loudness_bank_measure_groups, with its refusals.  *d_peaks: device array [n_groups],
 * valid until the next call on the bank.  Also OMX_ERR_INVALID: the timeline is off.  n_groups == 0: OMX_NONE. */
int omx_program_loudness_bank_measure_group_peaks(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                                  const omx_program_group* groups, uint64_t n_groups, void* stream,
                                                  const omx_program_part_peak** d_peaks);
int omx_program_loudness_bank_fetch_group_peaks(omx_program_loudness_bank* b, const omx_program_interval* members, uint64_t n_members,
                                                const omx_program_group* groups, uint64_t n_groups, omx_program_part_peak* dst);

/* omx_program_loudness_bank_plan_group_gains with ONE difference: the source peak of a group is the group peak's max_true_peak_db
 * from the timeline (the peak during the members' own segments), not the maximum over the members' whole streams.  Same rule checks,
 * same validation of the tables, same gain buffer, lifetime and omx_program_loudness_bank_fetch_gains, the same gain function
 * (omx_program_gain_evaluate).  It overwrites what earlier measure_groups / measure_group_peaks calls returned.  Also
 * OMX_ERR_INVALID, with nothing changed: the timeline is off. */
int omx_program_loudness_bank_plan_part_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule,
                                              const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                              uint64_t n_groups, void* stream, const omx_program_gain_record** d_gains);
/* A refused call changes nothing: neither the bank's state nor what an earlier call returned.  Every refusal's text
 * (omx_last_error) starts "program loudness peak timeline: ". */

#ifdef __cplusplus
}
#endif
#endif

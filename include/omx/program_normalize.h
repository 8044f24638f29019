/* Programme loudness bank, normalisation: the gain that brings a programme (or an album) to a target level, planned on the device
 * from the bank's own records, and a pass that applies such gains to PCM in device memory ("64 programmes at -23 LUFS, -1 dBTP",
 * "this album at -14 LUFS with one gain for all tracks").  The figures of EBU R 128 are measured for this; with this header the host
 * fetches no record, uploads no gain and writes no kernel of its own.
 *
 * Additive: this header adds three structures, six functions and a few constants; nothing declared in
 * program_loudness.h, program_peaks.h, program_timeline.h, program_histogram.h or program_groups.h changes and OMX_ABI_VERSION stays
 * as it is.  A bank that never calls one of them launches and allocates nothing more.  All work goes on the caller's stream; only
 * the fetch_* functions synchronise.  No call of this header changes any measurement state: every record of program_loudness.h and
 * program_peaks.h has the same bytes before and after.
 *
 * DEFINITION OF THE GAIN ("Normalisation"; tests/program_normalize_ref.py restates it).  Every step is f64 on
 * the f32 fields of the source record.  Inputs: I = integrated_lufs, n = gating_above_relative, P = max_true_peak_db, F = the bank's
 * floor_db; the rule's target, ceiling, min and max.
 *   1. n == 0: limited_by = NO_MEASUREMENT, gain_db = 0, gain = 1, peak_known = (P > F), the predicted fields equal the source fields.
 *      Stop.  (Nothing passed the gates: there is no loudness to normalise.)
 *   2. g = (double)target - (double)I;  limited_by = TARGET.
 *   3. peak_known = P > F.  (A peak at the floor is "never measured": peaks off and nothing folded by note_snapshots, or silence.)
 *   4. with OMX_GAIN_LIMIT_PEAK and peak_known: pg = (double)ceiling - (double)P;  if pg < g: g = pg, limited_by = PEAK.
 *   5. if g > max: g = max, limited_by = MAX_GAIN.
 *   6. then, if g < min: g = min, limited_by = MIN_GAIN.  THE MINIMUM CLAMP WINS OVER THE PEAK LIMIT: the record then shows a
 *      predicted_peak_db above the ceiling, and the host that set such a clamp has to look at it.
 *   7. gain_db = (float)g;  gain = (float)pow(10.0, (double)gain_db / 20.0);
 *      predicted_lufs = (float)((double)I + (double)gain_db);
 *      predicted_peak_db = peak_known ? (float)((double)P + (double)gain_db) : F.
 *   The plan kernels and omx_program_gain_evaluate run the same inline function, so they cannot drift apart; gain_db, the predicted
 *   fields, limited_by and peak_known do not depend on where they were computed, and `gain` may differ by one f32 ulp between the
 *   device's and the host's pow.
 *
 * DEFINITION OF THE PASS.  out[s][f][c] = in[s][f][c] * gain for f < frames[s]: one IEEE f32 multiply, so NaN and infinity propagate,
 * denormals are kept and the result does not depend on the call's shape.  Frames at or above frames[s] of d_out are not written. */
#ifndef OMX_PROGRAM_NORMALIZE_H
#define OMX_PROGRAM_NORMALIZE_H

#include "program_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_GAIN_LIMIT_PEAK 1u          /* omx_program_gain_rule.flags: keep the predicted true peak at or below true_peak_ceiling_db */

#define OMX_GAIN_BY_TARGET 0u           /* omx_program_gain_record.limited_by: the target was reached */
#define OMX_GAIN_BY_PEAK 1u             /* the true-peak ceiling held the gain below the target's */
#define OMX_GAIN_BY_MAX_GAIN 2u         /* clamped at max_gain_db */
#define OMX_GAIN_BY_MIN_GAIN 3u         /* clamped at min_gain_db (wins over the peak limit) */
#define OMX_GAIN_BY_NO_MEASUREMENT 4u   /* no gating block above both gates: unity gain */

#define OMX_PROGRAM_UNITY_GAIN UINT32_MAX   /* as a gain index of apply_gains: factor 1 */

typedef struct omx_program_gain_rule {
    float target_lufs;            /* finite */
    float true_peak_ceiling_db;   /* used only with OMX_GAIN_LIMIT_PEAK; finite then */
    float min_gain_db, max_gain_db; /* finite, min <= max: the clamp */
    uint32_t flags;               /* OMX_GAIN_LIMIT_PEAK; any other bit: OMX_ERR_INVALID */
    uint32_t _pad;
} omx_program_gain_rule;          /* 24 bytes */

typedef struct omx_program_gain_record {
    float gain_db, gain;                   /* gain = the linear factor applied to samples */
    float source_lufs, source_peak_db;     /* what the gain was made from */
    float predicted_lufs, predicted_peak_db;
    uint32_t limited_by;                   /* OMX_GAIN_BY_* */
    uint32_t peak_known;                   /* 0: source_peak_db sat at the floor, no peak limit was applied */
} omx_program_gain_record;                 /* 32 bytes */

/* Host only, needs no device: the record the plan kernels write for these source values.
 * OMX_ERR_INVALID, with nothing written: a null rule or out, a non-finite rule field that is in use, min_gain_db > max_gain_db,
 * an unknown flag. */
int omx_program_gain_evaluate(const omx_program_gain_rule* rule, float integrated_lufs, uint64_t gating_above_relative,
                              float max_true_peak_db, float floor_db, omx_program_gain_record* out);

/* One gain per stream (track gain): the result pass when something changed since the last one, then one small kernel.
 * The source is the stream's omx_program_loudness_record.  With omx_program_loudness_bank_set_peaks on, its max_true_peak_db holds the
 * measured peak; with peaks off and nothing folded by note_snapshots it sits at the floor, peak_known is 0 and no peak limit applies.
 * *d_gains: device array [n_streams], in a buffer the bank owns; it stays valid through later apply_gains calls, until the next
 * plan_gains / plan_group_gains call or destroy.  OMX_ERR_INVALID, with nothing changed: a bad rule (as above), a null d_gains. */
int omx_program_loudness_bank_plan_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule, void* stream,
                                         const omx_program_gain_record** d_gains);
/* One gain per group (album gain): omx_program_loudness_bank_measure_groups of the same members and groups, then one kernel.
 * It validates exactly as measure_groups does (a bounded bank with a partial member: OMX_ERR_UNSUPPORTED) and overwrites what an
 * earlier measure_groups returned, as any bank call may.  Source loudness: the group record's.  Source peak: the maximum of
 * max_true_peak_db over the STREAMS of the group's members, whole-programme figures: the peak records have no time axis, so for a
 * member that is a part of a stream this is conservative (the gain may be lower than the part alone would need, never higher).
 * omx_program_loudness_bank_plan_part_gains (program_peak_timeline.h) takes the peak of the members' own segments instead.
 * A stream counts once however often it appears.  An empty group: OMX_GAIN_BY_NO_MEASUREMENT, source_peak_db = the floor.
 * *d_gains: device array [n_groups], same buffer and lifetime as above.  n_groups == 0 (with a good rule): OMX_NONE, nothing is
 * planned and an earlier plan stays. */
int omx_program_loudness_bank_plan_group_gains(omx_program_loudness_bank* b, const omx_program_gain_rule* rule,
                                               const omx_program_interval* members, uint64_t n_members, const omx_program_group* groups,
                                               uint64_t n_groups, void* stream, const omx_program_gain_record** d_gains);
/* Copy of the last plan's records [first, first + count) to the host; synchronises.  OMX_ERR_INVALID: no plan yet, a range outside
 * the last plan, a null dst with count > 0. */
int omx_program_loudness_bank_fetch_gains(omx_program_loudness_bank* b, uint64_t first, uint64_t count, omx_program_gain_record* dst);

typedef struct omx_program_apply_record {
    uint64_t frames;          /* frames scaled in this call */
    uint64_t samples_over;    /* samples with |out| > 1.0f (NaN is not counted, infinity is) */
    float gain;               /* the factor used */
    float out_sample_peak;    /* max |out|, fmaxf semantics (NaN ignored), 0 for no frames */
    float out_sample_peak_db; /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t gain_index;      /* the record used; OMX_PROGRAM_UNITY_GAIN for unity */
} omx_program_apply_record;   /* 32 bytes */

/* d_in, d_out: device f32 [n_streams][frames_capacity][channels], the layout of omx_program_loudness_bank_process.  d_out == d_in is
 * allowed (in place); any other overlap of the two buffers: OMX_ERR_INVALID.  frames: host array [n_streams] or NULL =
 * frames_capacity for every stream.  d_gains: a device array of n_gains gain records (what a plan call returned, or the caller's
 * own: only `gain` is read).  gain_of_stream: host array [n_streams], stream s is scaled by d_gains[gain_of_stream[s]].gain;
 * OMX_PROGRAM_UNITY_GAIN = factor 1; NULL = stream s uses record s.  An index at or above n_gains: OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID, as for process: channels outside 1 .. 8, frames[s] > frames_capacity, frames_capacity > 2^32 - 1, a null
 * d_in or d_out when any stream brings frames, a null d_gains when any stream names a record (an index other than OMX_PROGRAM_UNITY_GAIN); a null d_applied.
 * A refused call changes nothing: neither d_out nor the gain records nor what an earlier call left in the apply records.
 * *d_applied: device array [n_streams], written fresh by every call (also by one without frames), valid until the next
 * apply_gains call or destroy.  samples_over and out_sample_peak are order-free, so the record does not depend on the run.
 * The bank lends its stream count, its staging and its scratch; the measurement state is not touched, and feeding d_out to a second
 * bank is how a host verifies the result.  Returns OMX_PRODUCED when any stream brought a frame, else OMX_NONE. */
int omx_program_loudness_bank_apply_gains(omx_program_loudness_bank* b, const float* d_in, float* d_out, uint64_t frames_capacity,
                                          const uint32_t* frames, uint32_t channels, const omx_program_gain_record* d_gains,
                                          uint64_t n_gains, const uint32_t* gain_of_stream, void* stream,
                                          const omx_program_apply_record** d_applied);
/* Copy of one stream's record of the last apply_gains call; synchronises.  OMX_ERR_INVALID: no apply_gains call yet, an index out
 * of range, a null dst. */
int omx_program_loudness_bank_fetch_applied(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_apply_record* dst);

#ifdef __cplusplus
}
#endif
#endif

/* Programme loudness bank, signal QC: is the signal itself intact?  A delivery check asks, beside loudness and true peak, for a DC
 * offset, for runs of samples stuck at full scale (clipping), for dropouts (runs of digital silence inside the programme), for the
 * silence in front of and behind the programme (where a host trims), for NaN samples and for a stereo pair that is out of phase.  The
 * remix, limiter and PCM records count overs without structure: they cannot tell 400 scattered overs from one 400-sample flat top, and
 * they say nothing of silence, DC or phase.  This pass reads device PCM once and keeps an integer record per stream.
 *
 * Additive: this header adds six structures, seven functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls inspect_configure allocates and launches nothing more.  All work
 * goes on the caller's stream; only fetch_inspected synchronises (and inspect_configure).  No call of this header touches measurement
 * state, gain plans, apply records, the limiter, the export, the resampler or the remix: every record of the earlier headers has the
 * same bytes before and after.
 *
 * DEFINITION ("Signal QC"; tests/program_inspect_ref.py restates it).
 *   For one stream x[n][c] is the f32 PCM taken since the inspector's last reset, n = 0 .. N-1, c < channels.
 *   Predicates  hot[n][c] = fabsf(x[n][c]) >= clip_level            (false for NaN, true for infinity)
 *               quiet[n]  = every channel has fabsf(x[n][c]) <= silence_level   (one NaN in the frame makes it false)
 *   Runs        R_c[n] = hot[n][c] ? R_c[n-1] + 1 : 0, R_c[-1] = 0;  Q[n] likewise over quiet.
 *   Channel     nan_samples        number of NaN samples
 *               clipped_samples    #{n : hot[n][c]}
 *               clip_runs          #{n : R_c[n] == clip_min_run}: a run is counted at the frame at which it reaches the minimum
 *                                  length, so the count needs no knowledge of where the run ends
 *               longest_clip_run   max_n R_c[n]
 *               longest_clip_start the smallest n - R_c[n] + 1 among the frames that reach that maximum; both 0 when nothing is hot
 *               open_clip_run      R_c[N-1]
 *   Stream      frames = N; silent_frames, silent_runs, longest_silent_run, longest_silent_start likewise over Q and silence_min_run;
 *               leading_silence    frames in front of the first frame that is not quiet, N when every frame is quiet
 *               trailing_silence   Q[N-1]
 *   DC          a NaN sample contributes 0; otherwise xc = fminf(fmaxf(x, -4.0f), 4.0f), q = (int64)rintf(xc * 268435456.0f) (2^28, an
 *               exact scaling; ties to even); dc_sum = the sum of q as an int64.
 *   Pairs       for a pair (a, b) every frame forms three products, each rounded to f32, nothing fused: x_a * x_b, x_a * x_a, x_b * x_b.
 *               For each product p: NaN gives 0, otherwise pc = fminf(fmaxf(p, -1.0f), 1.0f), q = (int64)rintf(pc * 1073741824.0f)
 *               (2^30).  sum_ab (int64), sum_aa, sum_bb (uint64) are the sums of q.
 *   Limit       a stream takes at most 2^32 - 1 frames between resets (the host mirrors N and refuses the call beyond that): no sum
 *               can leave 64 bits, |q| <= 2^30.
 *   Every quantity of the record is an integer made from single f32 operations on single frames, plus run lengths: any parallel
 *   schedule gives the same bits, and the record does not depend, in any bit, on how the programme is cut into calls.
 *
 * SUMMARY (host only).  omx_program_inspect_summarize turns a record into the figures a person reads, in C double:
 *   dc_offset[c]    (float)((double)dc_sum / 268435456.0 / (double)frames), 0 with no frames
 *   dc_offset_db[c] (float)fmax(20 log10(fabs((double)dc_offset[c])), OMX_INSPECT_DB_FLOOR), the floor itself when dc_offset is 0
 *   correlation[p]  correlation_valid = sum_aa > 0 && sum_bb > 0; (float)(sum_ab / sqrt((double)sum_aa * (double)sum_bb)) clamped to
 *                   [-1, 1], 0 when not valid
 *   interior_silent_runs = silent_runs - [leading_silence >= silence_min_run]
 *                                      - [trailing_silence >= silence_min_run && leading_silence < frames]
 *   verdict         OMX_INSPECT_NAN         any nan_samples
 *                   OMX_INSPECT_CLIPPED     any clip_runs
 *                   OMX_INSPECT_DROPOUT     interior_silent_runs > 0
 *                   OMX_INSPECT_ALL_SILENT  frames > 0 && leading_silence == frames
 *                   OMX_INSPECT_DC          any fabs(dc_offset) > dc_limit
 *                   OMX_INSPECT_ANTIPHASE   any valid pair with correlation < correlation_min */
#ifndef OMX_PROGRAM_INSPECT_H
#define OMX_PROGRAM_INSPECT_H

#include "program_remix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_INSPECT_MAX_PAIRS 4u
#define OMX_INSPECT_DEFAULT_CLIP_LEVEL 0.99996948f   /* 32767 / 32768 */
#define OMX_INSPECT_DEFAULT_CLIP_MIN_RUN 3u
#define OMX_INSPECT_DEFAULT_SILENCE_LEVEL 0.0f
#define OMX_INSPECT_DEFAULT_SILENCE_MIN_RUN 480u
#define OMX_INSPECT_DEFAULT_DC_LIMIT 1e-3f
#define OMX_INSPECT_DEFAULT_CORRELATION_MIN -0.2f
#define OMX_INSPECT_MAX_CLIP_MIN_RUN 65535u
#define OMX_INSPECT_MAX_SILENCE_MIN_RUN 16777216u    /* 2^24 */
#define OMX_INSPECT_DB_FLOOR -400.0f                 /* dc_offset_db of a zero offset */
/* omx_program_inspect_summary.verdict */
#define OMX_INSPECT_NAN 1u
#define OMX_INSPECT_CLIPPED 2u
#define OMX_INSPECT_DROPOUT 4u
#define OMX_INSPECT_ALL_SILENT 8u
#define OMX_INSPECT_DC 16u
#define OMX_INSPECT_ANTIPHASE 32u

typedef struct omx_program_inspect_rule {
    float clip_level;               /* finite, > 0 */
    uint32_t clip_min_run;          /* 1 .. 65535 */
    float silence_level;            /* finite, >= 0; 0 means exact digital silence */
    uint32_t silence_min_run;       /* 1 .. 2^24 */
    float dc_limit;                 /* finite, >= 0 */
    float correlation_min;          /* in [-1, 1] */
    uint32_t flags;                 /* must be 0 */
} omx_program_inspect_rule;         /* 28 bytes */

typedef struct omx_program_inspect_info {
    uint32_t tile_frames;           /* frames one workgroup of the main kernel takes at this channel count */
    uint32_t channels;
    uint32_t _pad[2];
} omx_program_inspect_info;         /* 16 bytes */

typedef struct omx_program_inspect_channel {
    int64_t dc_sum;
    uint64_t nan_samples;
    uint64_t clipped_samples;
    uint64_t clip_runs;
    uint64_t longest_clip_run;
    uint64_t longest_clip_start;
    uint64_t open_clip_run;
    uint64_t _pad;
} omx_program_inspect_channel;      /* 64 bytes */

typedef struct omx_program_inspect_pair {
    int64_t sum_ab;
    uint64_t sum_aa;
    uint64_t sum_bb;
    uint32_t a, b;
} omx_program_inspect_pair;         /* 32 bytes */

typedef struct omx_program_inspect_record {
    uint64_t frames;
    uint64_t silent_frames;
    uint64_t silent_runs;
    uint64_t longest_silent_run;
    uint64_t longest_silent_start;
    uint64_t leading_silence;
    uint64_t trailing_silence;
    uint32_t channels;
    uint32_t n_pairs;
    omx_program_inspect_channel channel[OMX_MAX_CHANNELS];  /* entries at and beyond `channels` are zero */
    omx_program_inspect_pair pair[OMX_INSPECT_MAX_PAIRS];   /* entries at and beyond `n_pairs` are zero */
} omx_program_inspect_record;       /* 704 bytes */

typedef struct omx_program_inspect_summary {
    uint32_t verdict;               /* OMX_INSPECT_* bits */
    uint32_t channels;
    uint32_t n_pairs;
    uint32_t _pad;
    uint64_t interior_silent_runs;
    float dc_offset[OMX_MAX_CHANNELS];
    float dc_offset_db[OMX_MAX_CHANNELS];
    float correlation[OMX_INSPECT_MAX_PAIRS];
    uint32_t correlation_valid[OMX_INSPECT_MAX_PAIRS];
} omx_program_inspect_summary;      /* 120 bytes */

/* Host only, needs no device: the header's defaults.  OMX_ERR_INVALID: a null rule. */
int omx_program_inspect_rule_default(omx_program_inspect_rule* rule);
/* Host only, needs no device: the main kernel's tile at a channel count.  OMX_ERR_INVALID, with nothing written: channels outside
 * 1 .. 8, a null info. */
int omx_program_inspect_plan(uint32_t channels, omx_program_inspect_info* info);
/* Host only, needs no device: SUMMARY above.  Entries at and beyond record->channels / record->n_pairs are zero.
 * OMX_ERR_INVALID, with nothing written: a null pointer, a bad rule (the table above), record->channels outside 1 .. 8,
 * record->n_pairs above OMX_INSPECT_MAX_PAIRS. */
int omx_program_inspect_summarize(const omx_program_inspect_rule* rule, const omx_program_inspect_record* record,
                                  omx_program_inspect_summary* summary);

/* Sets the rule, the channel count of the PCM and the pairs (host array [n_pairs][2] of channel indices; may be NULL with n_pairs 0),
 * allocates the records and resets every stream.  Allowed only while no stream of the inspector holds frames: a new bank, or after
 * inspect_reset of every stream.  *d_inspected of an earlier call is invalid afterwards.
 * OMX_ERR_INVALID, with nothing changed: a bad rule, channels outside 1 .. 8, n_pairs > OMX_INSPECT_MAX_PAIRS, a null pairs with
 * n_pairs > 0, a pair index at or above channels, a == b, a stream that holds frames. */
int omx_program_loudness_bank_inspect_configure(omx_program_loudness_bank* b, const omx_program_inspect_rule* rule, uint32_t channels,
                                                const uint32_t* pairs, uint32_t n_pairs);
/* The flagged streams start over with a zero record (reset_mask: host array [n_streams], NULL = every stream).
 * OMX_ERR_INVALID: before configure. */
int omx_program_loudness_bank_inspect_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_in: device f32 [n_streams][frames_capacity][channels]; the call reads it and writes nothing into it.  frames: host array
 * [n_streams] or NULL = frames_capacity for every stream.
 * OMX_ERR_INVALID: a call before configure; frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a stream that would hold more
 * than 2^32 - 1 frames since its reset; a null d_in when any stream brings frames; a null d_inspected.
 * A refused call changes nothing.
 * *d_inspected: device array [n_streams] of the running records, valid until inspect_configure or destroy; work on `stream` that
 * reads it has to be ordered behind the call.  Returns OMX_PRODUCED when any stream brought a frame, else OMX_NONE. */
int omx_program_loudness_bank_inspect(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                      void* stream, const omx_program_inspect_record** d_inspected);
/* Copy of one stream's running record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_inspected(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_inspect_record* dst);

#ifdef __cplusplus
}
#endif
#endif

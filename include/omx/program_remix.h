/* Programme loudness bank, channel layout: a static mixing matrix on device PCM.  A delivery specification names a loudness, a
 * true-peak ceiling, a sample format, a sample rate and a channel layout; program_normalize.h, program_limit.h, program_pcm.h and
 * program_resample.h give the first four.  Loudness and true peak are properties of the delivered channels (rear and side channels
 * weigh 1.41, LFE weighs 0, a fold-down sums correlated channels), so the mix sits in front of process: a 5.1 master that leaves as a
 * stereo Lo/Ro fold-down, a film-order file that becomes L R C LFE Ls Rs, a stereo programme checked as its mono fold, a pair taken
 * out of an 8-channel capture never go back to the host.
 *
 * Additive: this header adds three structures, six functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls remix_configure allocates and launches nothing more.  All work
 * goes on the caller's stream; only fetch_remixed synchronises (and remix_configure, see there).  No call of this header touches
 * measurement state, gain plans, apply records, the limiter, the export or the resampler: every record of the earlier headers has the
 * same bytes before and after.
 *
 * DEFINITION ("Channel layout: remix and downmix"; tests/program_remix_ref.py restates it).
 *   Matrix  m[channels_out][channels_in] f32, row-major.
 *   Mix     for frame f and output channel o, the input channels i are taken in increasing order.  A coefficient that is exactly zero
 *           (either sign) is SKIPPED: its input sample does not enter the arithmetic at all.  The first term that is not skipped sets
 *             acc = m[o][i] * x[f][i]
 *           and each later one does
 *             acc = acc + m[o][i] * x[f][i]
 *           Every product is rounded to f32 before it is added, nothing is fused.  A row without a non-zero coefficient gives +0.0f.
 *           out[f][o] = acc.
 *   So a row with the single coefficient 1.0f copies its input bit for bit (-0.0f, infinities and quiet NaNs included), an infinity
 *   or a NaN in a dropped channel (LFE at level 0) does not reach the output, and the output of a frame depends on that frame alone:
 *   it does not depend, in any bit, on how the programme is cut into calls.
 *
 * PRESETS (host only).  omx_program_remix_downmix builds the ITU-R BS.775-style fold-down from OMX_POS_* positions,
 * omx_program_remix_select the matrix that reorders channels or takes some of them out.  Both only fill a matrix: the bank takes any
 * finite matrix.
 *
 * RECORD.  Written fresh by every call, as omx_program_apply_record is.  The count is an integer sum and the peak a maximum: the record
 * does not depend on the schedule. */
#ifndef OMX_PROGRAM_REMIX_H
#define OMX_PROGRAM_REMIX_H

#include "program_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_REMIX_MAX_MATRICES 65536u     /* matrices of one table */
#define OMX_REMIX_KIND_STEREO 0u          /* omx_program_downmix_rule.kind: Lo/Ro */
#define OMX_REMIX_KIND_MONO 1u            /* the mono fold of Lo/Ro */
#define OMX_REMIX_NORMALIZE 1u            /* omx_program_downmix_rule.flags: a full-scale input cannot exceed full scale */
#define OMX_REMIX_DEFAULT_CENTER 0.70710678f
#define OMX_REMIX_DEFAULT_SURROUND 0.70710678f
#define OMX_REMIX_DEFAULT_LFE 0.0f

typedef struct omx_program_remix_info {
    uint32_t tile_frames;           /* frames one workgroup of the main kernel takes under this channel pair */
    uint32_t channels_in, channels_out;
    uint32_t _pad;
} omx_program_remix_info;           /* 16 bytes */

typedef struct omx_program_downmix_rule {
    uint32_t kind;                  /* OMX_REMIX_KIND_* */
    float center_level;             /* c: FRONT_CENTER and MONO into both sides; finite, 0 .. 2 */
    float surround_level;           /* s: REAR_* and SIDE_* into their side; finite, 0 .. 2 */
    float lfe_level;                /* l: LOW_FREQUENCY into both sides; finite, 0 .. 2 */
    uint32_t flags;                 /* 0 or OMX_REMIX_NORMALIZE */
} omx_program_downmix_rule;         /* 20 bytes */

typedef struct omx_program_remix_record {
    uint64_t frames;                /* frames this call mixed for the stream */
    uint64_t samples_over;          /* output samples with |out| > 1.0f (NaN is not counted, infinity is) */
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored) */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t matrix_index;          /* the matrix the stream used */
    uint32_t terms;                 /* its non-zero coefficients */
} omx_program_remix_record;         /* 32 bytes */

/* Host only, needs no device: the main kernel's tile under a channel pair.  OMX_ERR_INVALID, with nothing written: a channel count
 * outside 1 .. 8, a null info. */
int omx_program_remix_plan(uint32_t channels_in, uint32_t channels_out, omx_program_remix_info* info);

/* Host only, needs no device: the fold-down of a layout given as OMX_POS_* positions (positions_in[i] for i < channels_in; the rest is
 * not read).  Every input has a weight pair (wl, wr):
 *     FRONT_LEFT (1, 0)     FRONT_RIGHT (0, 1)     FRONT_CENTER and MONO (c, c)     LOW_FREQUENCY (l, l)
 *     REAR_LEFT and SIDE_LEFT (s, 0)     REAR_RIGHT and SIDE_RIGHT (0, s)     everything else (UNKNOWN, AUX) (0, 0)
 * With OMX_REMIX_NORMALIZE: n = max(sum |wl[i]|, sum |wr[i]|), each sum in f32, in order of i, starting at +0.0f; when n > 1.0f every
 * weight is divided by n (f32 division).  One divisor serves both sides: the balance is kept, and a full-scale input cannot exceed
 * full scale.
 * OMX_REMIX_KIND_STEREO: matrix [2][channels_in], the rows wl and wr; *channels_out = 2, positions_out = {FRONT_LEFT, FRONT_RIGHT}.
 * OMX_REMIX_KIND_MONO: matrix [1][channels_in], the row 0.5f * (wl[i] + wr[i]) in f32 (of the normalised weights, with the flag);
 * *channels_out = 1, positions_out = {MONO}.  This is the fold of Lo/Ro: BS.775's own 3/2 -> 1/0 row is this row times sqrt(2).
 * positions_out gets all 8 entries, OMX_POS_UNKNOWN behind channels_out.  matrix must hold 2 * channels_in floats for STEREO,
 * channels_in for MONO.
 * OMX_ERR_INVALID, with nothing written: a null pointer, channels_in outside 1 .. 8, an unknown kind or flag, a level that is not
 * finite or lies outside [0, 2]. */
int omx_program_remix_downmix(const omx_program_downmix_rule* rule, uint32_t channels_in, const uint8_t positions_in[OMX_MAX_CHANNELS],
                              float* matrix, uint32_t* channels_out, uint8_t positions_out[OMX_MAX_CHANNELS]);

/* Host only, needs no device: reorder, or take channels out.  matrix [channels_out][channels_in]: m[o][i] = 1.0f for the lowest i with
 * positions_in[i] == positions_out[o], every other coefficient +0.0f.  An output without a source gets a zero row and bit o of
 * *missing_mask.  OMX_ERR_INVALID, with nothing written: a null pointer, a channel count outside 1 .. 8. */
int omx_program_remix_select(uint32_t channels_in, const uint8_t positions_in[OMX_MAX_CHANNELS], uint32_t channels_out,
                             const uint8_t positions_out[OMX_MAX_CHANNELS], float* matrix, uint32_t* missing_mask);

/* Uploads n_matrices matrices ([n_matrices][channels_out][channels_in] f32, host memory) and allocates the records.  Allowed at any
 * time: the pass keeps no per-stream state.  Remix calls still enqueued on any stream are waited for (the device is synchronised)
 * before an earlier table is released; *d_remixed of an earlier call is invalid afterwards.
 * OMX_ERR_INVALID, with nothing changed: a channel count outside 1 .. 8, a null table, n_matrices 0 or above OMX_REMIX_MAX_MATRICES,
 * a coefficient that is not finite. */
int omx_program_loudness_bank_remix_configure(omx_program_loudness_bank* b, uint32_t channels_in, uint32_t channels_out,
                                              const float* matrices, uint32_t n_matrices);

/* d_in: device f32 [n_streams][frames_capacity][channels_in]; frames: host array [n_streams] or NULL = frames_capacity for every
 * stream.  d_out: device f32 [n_streams][frames_capacity][channels_out]; no float of d_out[s] at or beyond frames[s] * channels_out is
 * written.  matrix_of_stream: host array [n_streams], or NULL = matrix 0 for every stream.  Out of place only: any overlap of d_in and
 * d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a matrix index out of range;
 * a null d_in or d_out when any stream brings frames; a null d_remixed.
 * A refused call changes nothing: neither d_out nor the records.
 * *d_remixed: device array [n_streams] of this call's records, valid until remix_configure or destroy; work on `stream` that reads it
 * has to be ordered behind the call.  Returns OMX_PRODUCED when any stream brought a frame, else OMX_NONE. */
int omx_program_loudness_bank_remix(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                    float* d_out, const uint32_t* matrix_of_stream, void* stream,
                                    const omx_program_remix_record** d_remixed);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_remixed(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_remix_record* dst);

#ifdef __cplusplus
}
#endif
#endif

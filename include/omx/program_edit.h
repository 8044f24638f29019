/* Programme loudness bank, edit: clips, trims, fades and crossfades on device PCM.  Every earlier stage maps frame n of a stream to
 * frame n of the same stream (the resampler changes only the rate): the chain cannot change where a programme starts, where it ends or
 * what it is made of.  Signal QC says where the silence in front of and behind a programme lies, "where a host trims"; groups measure a
 * programme without its ad breaks or the album loudness of twelve tracks, but nothing makes that programme or that album.  This header
 * adds the edit-decision-list pass: a table of clips says which source frames of which input stream land where in which output stream,
 * with a gain, a fade-in and a fade-out each; two clips may overlap (a crossfade).  inspect, trim, fade, join, measure, normalise, limit
 * and export then run without PCM going back to the host.
 *
 * Additive: this header adds four structures, eight functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls edit_configure allocates and launches nothing more.  All work
 * goes on the caller's stream; only fetch_edited synchronises (and edit_configure, see there).  No call of this header touches
 * measurement state, gain plans, apply records, the limiter, the export, the resampler, the remix or the inspector: every record of the
 * earlier headers has the same bytes before and after.
 *
 * DEFINITION ("Edit: clips, trims, fades and crossfades"; tests/program_edit_ref.py restates it).
 *   Clip    puts source frames [src_first, src_first + frames) of input stream src_stream at output frames
 *           [dst_first, dst_first + frames) of output stream dst_stream.  The table is sorted by (dst_stream, dst_first); at most TWO
 *           clips cover any output frame; dst_first + frames <= 2^40.  Two clips may read the same source frames.  A clip of 0 frames
 *           does nothing.
 *   Phase   for a fade of F frames (1 <= F <= 2^24) and an index i < F, all in unsigned 64-bit integers:
 *             M = floor(2^63 / F)          (made on the host: the kernel does no integer division)
 *             p = ((2 i + 1) * M) >> 40    (the product stays below 2^64; 0 <= p < 2^24)
 *           p is the 24-bit fixed-point value of (i + 1/2) / F.
 *   Curve   each curve is a table of 4097 f32 values, made on the host in double and rounded once: linear k / 4096, equal power
 *           sin(pi/2 * k / 4096), raised cosine 1/2 - 1/2 cos(pi * k / 4096); entry 0 is exactly 0 and entry 4096 exactly 1.
 *             a = tab[p >> 12], b = tab[(p >> 12) + 1], fr = (float)(p & 4095) * 2^-12 (exact)
 *             g = a + (b - a) * fr         three f32 operations, each rounded, nothing fused
 *           The device calls no transcendental function.  g is monotone in i and 0 <= g <= 1: 0 itself only beyond
 *           F = 2^23 (where p can be 0), 1 itself only where a curve is flat to f32 (the end of a long equal-power or
 *           raised-cosine fade), never on the linear curve, whose g is p / 2^24.
 *   Weight  of a clip at its local frame j (output frame dst_first + j), starting from w = gain:
 *             if j < fade_in_frames:                w = w * g_in(j)
 *             if frames - 1 - j < fade_out_frames:  w = w * g_out(frames - 1 - j)     (the fade-out mirrors a fade-in)
 *           Both may hold inside a short clip; then both factors apply, in that order.
 *   Sample  a frame outside both fades of a clip whose gain is exactly 1.0f is COPIED, bit for bit (-0.0f, infinities, NaN payloads
 *           and denormals included); otherwise y = w * x, rounded.  An output frame under two clips is y_first + y_second, the clip
 *           earlier in the table on the left; a frame under no clip is +0.0f.  The bits of a NaN that comes out of that addition are
 *           not defined.
 *   The output frame depends only on its absolute position and the table: it has the same bits through whichever window
 *   (out_first, out_frames) it is rendered.
 *
 * RECORD.  Written fresh by every call, per output stream.  The counts are integers and the peak is a maximum: the record does not
 * depend on the schedule.  Over windows that tile an output every count adds up and the peak is the maximum. */
#ifndef OMX_PROGRAM_EDIT_H
#define OMX_PROGRAM_EDIT_H

#include "program_inspect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_EDIT_CURVE_LINEAR 0u
#define OMX_EDIT_CURVE_EQUAL_POWER 1u
#define OMX_EDIT_CURVE_RAISED_COSINE 2u
#define OMX_EDIT_CURVE_POINTS 4097u
#define OMX_EDIT_MAX_FADE 16777216u               /* 2^24 frames */
#define OMX_EDIT_MAX_OUTPUTS 16777216u            /* 2^24 output streams */
#define OMX_EDIT_MAX_POSITION 1099511627776ull    /* 2^40: no output frame lies at or beyond it */

typedef struct omx_program_edit_clip {
    uint32_t src_stream;            /* input stream, below the bank's n_streams */
    uint32_t dst_stream;            /* output stream, below the call's n_out */
    uint64_t src_first;             /* first source frame */
    uint64_t dst_first;             /* first output frame */
    uint64_t frames;
    uint32_t fade_in_frames;        /* 0 = none; <= frames and <= 2^24 */
    uint32_t fade_out_frames;       /* 0 = none; <= frames and <= 2^24 */
    uint8_t fade_in_curve;          /* OMX_EDIT_CURVE_* */
    uint8_t fade_out_curve;
    uint16_t flags;                 /* must be 0 */
    float gain;                     /* finite */
} omx_program_edit_clip;            /* 48 bytes */

typedef struct omx_program_edit_info {
    uint32_t tile_frames;           /* output frames one workgroup of the main kernel takes at this channel count */
    uint32_t channels;
    uint32_t _pad[2];
} omx_program_edit_info;            /* 16 bytes */

typedef struct omx_program_trim_rule {
    uint64_t keep_head;             /* frames of the leading silence to keep (all of it when it is shorter) */
    uint64_t keep_tail;             /* frames of the trailing silence to keep */
    uint64_t pad_head;              /* frames of +0.0f in front of the clip */
    uint64_t pad_tail;              /* frames of +0.0f behind it */
    uint32_t fade_in_frames;        /* <= 2^24; clamped to the kept length */
    uint32_t fade_out_frames;
    uint8_t fade_in_curve;          /* OMX_EDIT_CURVE_* */
    uint8_t fade_out_curve;
    uint16_t flags;                 /* must be 0 */
    uint32_t _pad;
} omx_program_trim_rule;            /* 48 bytes */

typedef struct omx_program_edit_record {
    uint64_t out_first;             /* the window this call rendered */
    uint64_t frames;
    uint64_t silent_frames;         /* frames of the window under no clip */
    uint64_t faded_frames;          /* frames at which some fade factor applied */
    uint64_t mixed_frames;          /* frames under two clips */
    uint64_t samples_over;          /* output samples with |out| > 1.0f (NaN is not counted, infinity is) */
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored) */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t clips;                 /* clips of the table that touch the window */
    uint32_t _pad;
} omx_program_edit_record;          /* 64 bytes */

/* Host only, needs no device: the main kernel's tile at a channel count.  OMX_ERR_INVALID, with nothing written: channels outside
 * 1 .. 8, a null info. */
int omx_program_edit_plan(uint32_t channels, omx_program_edit_info* info);
/* Host only, needs no device: the curve's table, Curve above.  OMX_ERR_INVALID, with nothing written: an unknown curve, a null dst. */
int omx_program_edit_curve(uint32_t curve, float dst[OMX_EDIT_CURVE_POINTS]);
/* Host only, needs no device: g of Phase and Curve above, by the inline function the kernel runs.  OMX_ERR_INVALID, with nothing
 * written: an unknown curve, fade_frames 0 or above 2^24, index >= fade_frames, a null g. */
int omx_program_edit_gain(uint32_t curve, uint32_t fade_frames, uint32_t index, float* g);
/* Host only, needs no device: validates a table and writes, per output stream, one past its last covered frame (0 for a stream
 * without a clip that has frames).  frames_in[i]: the frames input stream i holds.
 * OMX_ERR_INVALID, with nothing written: a null clips with n_clips > 0, a null frames_in with n_in > 0, a null out_frames with
 * n_out > 0; a src_stream at or above n_in, a dst_stream at or above n_out; a table that is not sorted by (dst_stream, dst_first); a
 * third clip over an output frame; src_first + frames beyond frames_in[src_stream]; dst_first + frames beyond 2^40; a fade longer than
 * the clip or than 2^24; an unknown curve; a flag set; a gain that is not finite. */
int omx_program_edit_extent(const omx_program_edit_clip* clips, uint64_t n_clips, uint32_t n_in, const uint32_t* frames_in, uint32_t n_out,
                            uint64_t* out_frames);
/* Host only, needs no device: the clip that cuts a stream where inspect found silence.  With N = record->frames,
 * L = record->leading_silence, T = record->trailing_silence: a stream that is silent from end to end (L == N) gives a clip of 0 frames
 * and *out_frames = pad_head + pad_tail.  Otherwise
 *   src_first = L - min(keep_head, L), frames = N - src_first - (T - min(keep_tail, T)), dst_first = pad_head,
 *   fade_in_frames = min(rule's, frames), fade_out_frames likewise, the rule's curves, gain 1.0f, *out_frames = pad_head + frames + pad_tail.
 * OMX_ERR_INVALID, with nothing written: a null pointer, an unknown curve, a flag set, a fade above 2^24, a record with L > N, T > N or
 * L < N and L + T > N, N beyond 2^32 - 1, *out_frames beyond 2^40. */
int omx_program_edit_trim(const omx_program_inspect_record* record, const omx_program_trim_rule* rule, uint32_t src_stream, uint32_t dst_stream,
                          omx_program_edit_clip* clip, uint64_t* out_frames);

/* Sets the channel count of the PCM and the largest n_out of a call, allocates the records ([max_outputs], each the record of a call
 * that brought nothing) and uploads the three curve tables.  Allowed at any time: the pass keeps no per-stream state.  Edit calls still
 * enqueued on any stream are waited for (the device is synchronised) before an earlier allocation is released; *d_edited of an earlier
 * call is invalid afterwards.
 * OMX_ERR_INVALID, with nothing changed: channels outside 1 .. 8, max_outputs 0 or above 2^24. */
int omx_program_loudness_bank_edit_configure(omx_program_loudness_bank* b, uint32_t channels, uint32_t max_outputs);

/* d_in: device f32 [n_streams][frames_capacity][channels]; frames_in: host array [n_streams] of the frames each input stream holds, or
 * NULL = frames_capacity for every stream.  clips: host array [n_clips], the table (DEFINITION).  d_out: device f32
 * [n_out][out_capacity][channels].  The call renders output frames [out_first[o], out_first[o] + out_frames[o]) of output stream o into
 * d_out[o][0 ..]; out_first: host array [n_out] or NULL = 0 for every output; out_frames: host array [n_out], out_frames[o] <=
 * out_capacity.  No float of d_out[o] at or beyond out_frames[o] * channels is written; frames of the window under no clip are written
 * as +0.0f.  Out of place only: any overlap of d_in and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; n_out 0 or above max_outputs; whatever omx_program_edit_extent refuses (with the
 * bank's n_streams as n_in); frames_in[s] > frames_capacity; a capacity beyond 2^32 - 1; out_frames[o] > out_capacity;
 * out_first[o] + out_frames[o] beyond 2^40; more than 2^26 clips; a null out_frames or d_edited; a null d_out when any window holds a frame; a null d_in when
 * the table holds a clip with frames.
 * A refused call changes nothing: neither d_out nor the records.
 * *d_edited: device array [max_outputs] of the records, entries below n_out written fresh by this call, valid until edit_configure or
 * destroy; work on `stream` that reads it has to be ordered behind the call.  Returns OMX_PRODUCED when any output frame was written,
 * else OMX_NONE. */
int omx_program_loudness_bank_edit(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames_in,
                                   const omx_program_edit_clip* clips, uint64_t n_clips, float* d_out, uint64_t out_capacity, uint32_t n_out,
                                   const uint64_t* out_first, const uint32_t* out_frames, void* stream,
                                   const omx_program_edit_record** d_edited);
/* Copy of one output's record; synchronises.  OMX_ERR_INVALID: before configure, an index at or above max_outputs, a null dst. */
int omx_program_loudness_bank_fetch_edited(omx_program_loudness_bank* b, uint64_t output_index, omx_program_edit_record* dst);

#ifdef __cplusplus
}
#endif
#endif

/* Programme loudness bank, limiter: a look-ahead true-peak limiter for normalised output.  program_normalize.h reaches a loudness
 * target OR keeps the true peak under a ceiling (OMX_GAIN_LIMIT_PEAK holds the gain down); delivery specifications ask for both
 * ("-14 LUFS and -1 dBTP").  With this header the target gain is applied in full and the few peaks above the ceiling are taken down
 * by a gain envelope that starts to fall before each peak arrives.
 *
 * Additive: this header adds two structures and five functions; nothing declared in the headers it includes changes and
 * OMX_ABI_VERSION stays as it is.  A bank that never calls limiter_configure allocates and launches nothing more.  All work goes on
 * the caller's stream; only fetch_limited synchronises.  No call of this header changes any measurement state: every record of the
 * earlier headers has the same bytes before and after.
 *
 * DEFINITION ("Limiter"; tests/program_limit_ref.py restates it).  For one stream, x[n][c] is the PCM taken
 * since the limiter's last reset, n = 0 .. N-1, c < channels; g the stream's gain factor, fs the sanitised rate.
 *   Level     v_c[n] = the v[n] of program_peaks.h for channel c: the maximum of |x[n]| and the interpolated outputs of the rate's band
 *             (4x below 96 kHz, 2x below 192 kHz, none above), f32 sums in order, products rounded before they are added, fmaxf
 *             ignoring NaN.  v[n] = max_c v_c[n]: all channels are linked, LFE included.  u[n] = v[n] * fabsf(g), one f32 multiply.
 *   Ceiling   c = (float)pow(10.0, (double)ceiling_db / 20.0), computed once on the host and stored in the record.
 *   Required  q[n] = u[n] > c ? (uint32)floor((double)c / (double)u[n] * 16777216.0) : 2^24.  A NaN u compares false (q = 2^24), an
 *             infinite u gives 0.  q[n] = 2^24 for n < 0, and for n >= N once the stream is flushed.
 *   Hold      w[n] = min(q[n-W+1 .. n]), W = A + 24 + R, A = attack_frames, R = release_hold_frames.  (24 covers the longest
 *             interpolator window; it is the same in every band.)
 *   Smooth    S[n] = sum(w[n-A+1 .. n]) as a u64: an integer sum, exact and order-free.
 *   Envelope  LA = A + 23 is the latency in frames.  Gf[j] = (float)((double)S[j + LA] / (double)((uint64)A << 24)).
 *             Gf[j] is at or below q[t] / 2^24 for every t in [j-R, j+24], and exactly 1.0f wherever nothing within reach exceeds
 *             the ceiling.
 *   Output    k[j] = g * Gf[j] in f32; out[j][c] = x[j][c] * k[j], one f32 multiply per sample.  NaN and infinity follow from this
 *             arithmetic.  A stream that is never limited gets the bits of apply_gains.
 * Every quantity between the f32 level and the f32 envelope is an integer, so any parallel schedule gives the same bits, and the
 * output does not depend, in any bit, on how the programme is cut into calls.
 *
 * BOUND.  |out| <= c * (1 + 2^-21) for normal values: the f32 roundings between the level and the output sample (u, the envelope,
 * k and the product) each stay within 2^-24 relative of their exact values and rounding is monotone; DESIGN.md derives it.
 * The TRUE peak of the output is not bounded by construction, because the envelope moves inside the interpolator's window; what it
 * reaches is a property of this definition, measured on the restatement and written down in DESIGN.md.
 *
 * STREAMING.  Per stream the limiter keeps N frames taken and E frames emitted.  A call that brings F frames emits frames [E, E') to
 * d_out[s][0 .. E'-E): E' = max(E, N - LA) without a flush, E' = N with the stream flagged in flush_mask.  A flushed stream takes no
 * more frames until it is reset.  The gain factor is read on the device when the stream takes its first frame after a reset and kept
 * until the next reset; the record reports it.  The host mirrors N, E and the flushed flag and validates every call before anything
 * is enqueued. */
#ifndef OMX_PROGRAM_LIMIT_H
#define OMX_PROGRAM_LIMIT_H

#include "program_normalize.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_LIMIT_IDLE 0u      /* omx_program_limit_record.state: no frame taken since the reset */
#define OMX_LIMIT_RUNNING 1u
#define OMX_LIMIT_FLUSHED 2u   /* everything taken has been emitted; the stream takes no more frames until it is reset */

typedef struct omx_program_limit_rule {
    float ceiling_db;               /* finite, within [-120, 20] */
    uint32_t attack_frames;         /* A: 1 .. 4096 */
    uint32_t release_hold_frames;   /* R: 0 .. 16384 */
    uint32_t flags;                 /* must be 0 */
} omx_program_limit_rule;           /* 16 bytes */

typedef struct omx_program_limit_record {
    uint64_t frames_in;         /* N: frames taken since the reset */
    uint64_t frames_out;        /* E: frames emitted since the reset */
    uint64_t frames_written;    /* frames this call wrote to d_out[s] */
    uint64_t frames_limited;    /* emitted frames with Gf < 1, since the reset */
    uint64_t samples_over;      /* samples with |out| > 1.0f (NaN is not counted, infinity is), since the reset */
    float gain;                 /* g, as latched; 1 while idle */
    float ceiling;              /* c, linear */
    float min_envelope;         /* the smallest Gf emitted since the reset, 1 when none */
    float out_sample_peak;      /* max |out|, fmaxf semantics (NaN ignored), since the reset */
    float out_sample_peak_db;   /* power_to_db(p * p, floor_db), as program_peaks.h */
    float max_reduction_db;     /* -power_to_db(min_envelope * min_envelope, floor_db) */
    uint32_t gain_index;        /* the gain record latched; OMX_PROGRAM_UNITY_GAIN for unity and while idle */
    uint32_t state;             /* OMX_LIMIT_* */
    uint32_t latency_frames;    /* LA */
    uint32_t _pad;
} omx_program_limit_record;     /* 80 bytes */

/* Host only, needs no device: *frames = attack_frames + 23.  OMX_ERR_INVALID, with nothing written: a null rule or frames, a
 * ceiling_db that is not finite or lies outside [-120, 20], attack_frames outside 1 .. 4096, release_hold_frames above 16384, a
 * flag set. */
int omx_program_limit_latency(const omx_program_limit_rule* rule, uint32_t* frames);

/* Sets the rule and the format of the PCM the limiter takes, allocates its state and leaves every stream idle.  Allowed only while
 * no stream of the limiter holds frames (a new bank, or every stream reset): otherwise OMX_ERR_INVALID and nothing changes.
 * Rates and channel counts and their errors are those of omx_program_loudness_bank_process; a bad rule (as above): OMX_ERR_INVALID. */
int omx_program_loudness_bank_limiter_configure(omx_program_loudness_bank* b, const omx_program_limit_rule* rule, uint32_t channels,
                                                float sample_rate);
/* The flagged streams (host array [n_streams]; NULL: every stream) forget their frames, their history and their gain and are idle
 * again.  OMX_ERR_INVALID before configure. */
int omx_program_loudness_bank_limiter_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);

/* d_in: device f32 [n_streams][frames_capacity][channels]; frames: host array [n_streams] or NULL = frames_capacity for every stream.
 * d_out: device f32 [n_streams][out_capacity][channels]; stream s gets its emitted frames at d_out[s][0 ..), frames at or above
 * frames_written[s] are not written.  flush_mask: host array [n_streams] or NULL = no stream.  d_gains, n_gains, gain_of_stream and
 * OMX_PROGRAM_UNITY_GAIN: as omx_program_loudness_bank_apply_gains; the factor is read only when a stream takes its first frame after
 * a reset.  Out of place only: any overlap of d_in and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; frames for a flushed stream; a stream that would emit more than out_capacity frames;
 * frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a gain index at or above n_gains; a null d_in when any stream brings
 * frames, a null d_out when any stream emits, a null d_gains when any stream names a record; a null d_limited.
 * A refused call changes nothing: neither d_out nor the records nor the limiter's state.
 * *d_limited: device array [n_streams] of the running records, valid until limiter_configure or destroy; work on `stream` that reads
 * it has to be ordered behind the call.  Returns OMX_PRODUCED when any stream emitted a frame, else OMX_NONE. */
int omx_program_loudness_bank_apply_limited(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity,
                                            const uint32_t* frames, float* d_out, uint64_t out_capacity, const uint8_t* flush_mask,
                                            const omx_program_gain_record* d_gains, uint64_t n_gains, const uint32_t* gain_of_stream,
                                            void* stream, const omx_program_limit_record** d_limited);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_limited(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_limit_record* dst);

#ifdef __cplusplus
}
#endif
#endif

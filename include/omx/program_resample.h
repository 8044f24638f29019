/* Programme loudness bank, sample-rate conversion: a rational polyphase resampler on device PCM.  A delivery specification names a
 * loudness, a true-peak ceiling, a sample format and a sample rate; program_normalize.h, program_limit.h and program_pcm.h give the
 * first three.  True peak and K-weighted loudness are properties of the delivered rate, so the conversion sits between import_pcm and
 * process: a master at 44.1 or 96 kHz that leaves as 48 kHz never goes back to the host.
 *
 * Additive: this header adds three structures, seven functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls resampler_configure allocates and launches nothing more.  All
 * work goes on the caller's stream; only fetch_resampled synchronises.  No call of this header touches measurement state, gain plans,
 * apply records, the limiter or the export: every record of the earlier headers has the same bytes before and after.
 *
 * DEFINITION ("Sample-rate conversion"; tests/program_resample_ref.py restates it).
 *   Plan    g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g.  Z = half_width.
 *           H = 2 * ceil(Z * max(1, M / L) / 2) (integers: Z for L >= M, else 2 * ceil(Z * M / (2 * L))): the half width in input frames
 *           and the latency.  T = 2 * H taps per phase, a multiple of 4.  fc = (double)cutoff * min(1, L / M), in f64.
 *   Taps    computed once on the host in f64, every step its own operation.  For phase p < L and tap k < T:
 *             d = (double)(k - H + 1) - (double)p / (double)L;  r = d / (double)H
 *             h = 0 where |d| >= H, else  fc * sinc(fc * d) * I0((double)beta * sqrt(1 - r * r)) / I0((double)beta)
 *             sinc(u) = 1 at u = 0, else sin(a) / a with a = pi * u
 *             I0(v): y = v * 0.5; t = 1; s = 1; for i = 1 .. OMX_RESAMPLE_I0_TERMS: t = t * (y / i); s = s + t * t.  (The power series
 *             with a fixed number of terms: at v = 20 the first term left out is below 1e-40 of the sum.)
 *           Each phase is divided by the f64 sum of its taps, added in order of increasing k: every phase has unit DC gain.  Then each
 *           tap is rounded to f32.  The table is [L][T] f32.
 *   Output  for one stream, x[n][c] are the frames taken since the resampler's last reset, n = 0 .. N-1; x is +0.0f for n < 0, and for
 *           n >= N once the stream is flushed.  For output frame m >= 0:  pos = m * M (u64), i0 = pos / L, p = pos % L,
 *             out[m][c] = (a0 + a1) + (a2 + a3)
 *           a_j starts at +0.0f and takes, in order of increasing k over k = j, j + 4, .. < T, the f32 product
 *           h[p][k] * x[i0 - H + 1 + k][c]: every product is rounded before it is added, nothing is fused.  NaN and infinity follow
 *           from this arithmetic (an infinity under a zero tap is a NaN).
 *   The output does not depend, in any bit, on how the programme is cut into calls.
 *
 * STREAMING.  Per stream the resampler keeps N frames taken and E frames emitted.  A call that brings F frames sets N += F and emits
 * frames [E, E') to d_out[s][0 .. E'-E):  E' = max(E, N > H ? ceil((N - H) * L / M) : 0) without a flush (every input an emitted frame
 * reads has been taken), E' = ceil(N * L / M) with the stream flagged in flush_mask.  A flushed stream takes no more frames until it
 * is reset.  The last T - 1 input frames of every stream stay on the device between calls; a call may bring fewer than that,
 * including none.  The host mirrors N, E and the flushed flag and validates every call before anything is enqueued.
 *
 * RECORD.  Counts are integer sums and the peak is a maximum: the record does not depend on the schedule. */
#ifndef OMX_PROGRAM_RESAMPLE_H
#define OMX_PROGRAM_RESAMPLE_H

#include "program_pcm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_RESAMPLE_IDLE 0u      /* omx_program_resample_record.state: no frame taken since the reset */
#define OMX_RESAMPLE_RUNNING 1u
#define OMX_RESAMPLE_FLUSHED 2u   /* the tail has been emitted; the stream takes no more frames until it is reset */

#define OMX_RESAMPLE_DEFAULT_HALF_WIDTH 32u
#define OMX_RESAMPLE_DEFAULT_BETA 12.0f
#define OMX_RESAMPLE_DEFAULT_CUTOFF 0.94f
#define OMX_RESAMPLE_I0_TERMS 64u         /* terms of the I0 power series behind the leading 1 */
#define OMX_RESAMPLE_MAX_FACTOR 1024u     /* largest L and largest M */
#define OMX_RESAMPLE_MAX_HALF_WIDTH 512u  /* largest H */
#define OMX_RESAMPLE_MIN_RATE 3364u       /* whole Hz; the rates omx_program_loudness_bank_process accepts */
#define OMX_RESAMPLE_MAX_RATE 768000u

typedef struct omx_program_resample_rule {
    uint32_t rate_in, rate_out;     /* whole Hz */
    uint32_t half_width;            /* Z: zero crossings per side at unity bandwidth; even, 8 .. 64 */
    float beta;                     /* Kaiser beta: finite, 0 .. 20 */
    float cutoff;                   /* the -6 dB point as a fraction of the narrower Nyquist: in (0.5, 1] */
    uint32_t flags;                 /* must be 0 */
} omx_program_resample_rule;        /* 24 bytes */

typedef struct omx_program_resample_info {
    uint32_t L, M;                  /* rate_out / g, rate_in / g */
    uint32_t taps;                  /* T = 2 H */
    uint32_t latency_frames;        /* H, in input frames */
    uint64_t table_floats;          /* L * T */
    uint32_t tile_frames;           /* output frames one workgroup of the main kernel computes under this plan */
    uint32_t _pad;
} omx_program_resample_info;        /* 32 bytes */

typedef struct omx_program_resample_record {
    uint64_t frames_in;             /* N: frames taken since the reset */
    uint64_t frames_out;            /* E: frames emitted since the reset */
    uint64_t frames_written;        /* frames this call wrote to d_out[s] */
    uint64_t samples_over;          /* samples with |out| > 1.0f (NaN is not counted, infinity is), since the reset */
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored), since the reset */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t state;                 /* OMX_RESAMPLE_* */
    uint32_t L, M, taps;
    uint32_t latency_frames;        /* H */
    uint32_t _pad;
} omx_program_resample_record;      /* 64 bytes */

/* Host only, needs no device: the plan of `rule`.  OMX_ERR_INVALID, with nothing written: a null rule or info, a rate of 0,
 * rate_in == rate_out, half_width odd or outside 8 .. 64, beta not finite or outside [0, 20], cutoff not in (0.5, 1], a flag set.
 * OMX_ERR_UNSUPPORTED, with nothing written: a rate outside OMX_RESAMPLE_MIN_RATE .. OMX_RESAMPLE_MAX_RATE, L or M above
 * OMX_RESAMPLE_MAX_FACTOR, H above OMX_RESAMPLE_MAX_HALF_WIDTH. */
int omx_program_resample_plan(const omx_program_resample_rule* rule, omx_program_resample_info* info);
/* Host only, needs no device: the [L][T] f32 table the kernel uses (the function resampler_configure itself calls).  n_floats must be
 * the plan's table_floats, else OMX_ERR_INVALID; a null dst: OMX_ERR_INVALID; a bad rule: as omx_program_resample_plan. */
int omx_program_resample_taps(const omx_program_resample_rule* rule, float* dst, uint64_t n_floats);
/* Host only, needs no device: *frames_out = E' - E of a stream that has taken frames_in_before and emitted frames_out_before frames
 * and now takes `frames` more, with (flush != 0) or without a flush: the STREAMING formula, so that a host can size d_out.
 * OMX_ERR_INVALID: a null frames_out, frames_in_before + frames beyond 2^63; a bad rule: as omx_program_resample_plan. */
int omx_program_resample_frames(const omx_program_resample_rule* rule, uint64_t frames_in_before, uint64_t frames_out_before,
                                uint64_t frames, uint32_t flush, uint64_t* frames_out);

/* Sets the rule and the channel count of the PCM the resampler takes, builds and uploads the table, allocates the carried frames and
 * the records and leaves every stream idle.  Allowed only while no stream of the resampler holds frames (a new bank, or every stream
 * reset): otherwise OMX_ERR_INVALID and nothing changes.  Also OMX_ERR_INVALID: channels outside 1 .. 8; a bad rule: as
 * omx_program_resample_plan. */
int omx_program_loudness_bank_resampler_configure(omx_program_loudness_bank* b, const omx_program_resample_rule* rule, uint32_t channels);
/* The flagged streams (host array [n_streams]; NULL: every stream) forget their frames and are idle again.  OMX_ERR_INVALID before
 * configure. */
int omx_program_loudness_bank_resampler_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);

/* d_in: device f32 [n_streams][frames_capacity][channels]; frames: host array [n_streams] or NULL = frames_capacity for every stream.
 * d_out: device f32 [n_streams][out_capacity][channels]; stream s gets its emitted frames at d_out[s][0 ..), frames at or above
 * frames_written[s] are not written.  flush_mask: host array [n_streams] or NULL = no stream.  Out of place only: any overlap of d_in
 * and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; frames for a flushed stream; a stream that would emit more than out_capacity frames;
 * frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a null d_in when any stream brings frames, a null d_out when any stream
 * emits; a null d_resampled.
 * A refused call changes nothing: neither d_out nor the records nor the resampler's state.
 * *d_resampled: device array [n_streams] of the running records, valid until resampler_configure or destroy; work on `stream` that
 * reads it has to be ordered behind the call.  Returns OMX_PRODUCED when any stream emitted a frame, else OMX_NONE. */
int omx_program_loudness_bank_resample(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       float* d_out, uint64_t out_capacity, const uint8_t* flush_mask, void* stream,
                                       const omx_program_resample_record** d_resampled);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_resampled(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_resample_record* dst);

#ifdef __cplusplus
}
#endif
#endif

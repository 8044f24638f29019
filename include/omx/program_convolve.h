/* Programme loudness bank, convolve: a FIR convolution stage on device PCM.  The filter stage (program_filter.h) is a cascade of at
 * most two biquads, so its phase moves with frequency.  A FIR with a compensated delay leaves the programme where it was on the time
 * axis, which is what a mastering EQ, a band-limit in front of a fold-down or a crossover whose bands sum back to the input needs, and
 * what edit, mix, the peak timeline and the interval tables (all addressing absolute frames) rely on.  A measured response (a room or
 * line correction, a matched de-emphasis, a Hilbert or band-pass analysis filter) exists only as taps, and a FIR of a few hundred taps
 * replaces a long biquad chain in one pass.
 *
 * Additive: this header adds four structures, nine functions and a few constants; nothing declared in the headers it includes changes
 * and OMX_ABI_VERSION stays as it is.  A bank that never calls convolve_configure allocates and launches nothing more.  All work goes
 * on the caller's stream; only fetch_convolved and convolve_configure synchronise.  No call of this header touches measurement state,
 * gain plans or the records of any other stage.
 *
 * DEFINITION ("Convolve"; tests/program_convolve_ref.py restates it).  Per stream and channel, h[0 .. T-1] are
 * the f32 taps of the channel's FIR.  x[n] are the frames taken since the stage's last reset; x[n] = +0.0f for n < 0, and for n >= N
 * once the stream is flushed.  D = delay_frames is set at configure and is one value for the whole bank, 0 <= D <= max_taps - 1.  For
 * output frame m >= 0, with n = m + D:
 *     acc = (double)h[0] * (double)x[n]
 *     acc = acc + (double)h[k] * (double)x[n - k]      for k = 1 .. T-1, in that order
 *     out[m] = (float)acc          (round to nearest even; f32 denormals are produced, nothing is flushed)
 *   Every product is EXACT in f64 (24 x 24 significant bits fit in 53 and the exponents stay inside the f64 range: program_mix.h), so
 *   fma(h, x, acc) and acc + h * x are the same f64 value and the kernel may use either.  Each sum is rounded to f64 once.
 *   The order of k is part of the function: a tree over the taps, or split accumulators, is a different function.
 *   Every tap takes part, zero taps and the zeros outside the stream included: an infinity under a zero tap is a NaN, and -0.0f under
 *   a unit impulse comes out +0.0f once a term of +0.0 is added (a zero tap times a sample that is not negative, or a zero outside
 *   the stream; a FIR of ONE tap 1.0f keeps the sign).
 *   A channel on OMX_CONVOLVE_BYPASS is out[m] = x[m], copied on bits, -0.0f and NaN payloads included: it is aligned with the
 *   compensated output of the filtered channels (what a unit impulse at k = D gives, up to the sign of zero and NaN bits).
 *   The bits of a NaN the arithmetic produces are not defined.
 *   The output does not depend, in any bit, on how the programme is cut into calls.
 *
 * STREAMING (the resampler's model, program_resample.h).  Per stream the host mirrors N frames taken, E frames emitted and a flushed
 * flag.  A call that brings F frames sets N += F and emits frames [E, E') to d_out[s][0 ..):  E' = max(E, N > D ? N - D : 0) without
 * a flush, E' = N with the stream flagged in flush_mask.  After a flush the output has exactly the input's length; with D = (T-1)/2 a
 * symmetric FIR leaves the programme in place.  With D = 0 every call emits what it takes and a flush emits nothing.  A flushed stream
 * takes no frames until it is reset.  The newest max_taps - 1 input frames of every stream stay on the device between calls; a call
 * may bring fewer than that, or none.  Out of place only.
 *
 * DESIGN FORMULAS (host only, f64, every step its own operation; sin and sqrt are the only library functions).  fs = sample rate,
 * T = n_taps (odd), M = (T-1)/2.  For k = 0 .. M:
 *     d = (double)k - (double)M;  r = d / (double)M;  c = 2 * fc / fs
 *     w[k] = c * sinc(c * d) * I0(beta * sqrt(1 - r * r)) / I0(beta)
 *     sinc(u) = 1 at u = 0, else sin(a) / a with a = pi * u;  I0: the series of program_resample.h, OMX_RESAMPLE_I0_TERMS terms.
 *   w[T-1-k] = w[k]; lp(fc)[k] = w[k] / sum, sum = the f64 sum of all T values of w added in order of increasing k.
 *   LOWPASS = lp(f_hi);  HIGHPASS = delta_M - lp(f_lo);  BANDPASS = lp(f_hi) - lp(f_lo);  BANDSTOP = delta_M - BANDPASS  (delta_M is
 *   1 at k = M, else 0; every difference is one f64 subtraction, BANDSTOP two).  The f64 taps k <= M are rounded to f32 and mirrored:
 *   h[k] == h[T-1-k] on bits.
 *
 * REFUSALS.  A refused call returns OMX_ERR_INVALID and sets omx_last_error() to "program loudness <who>: <why>", where <who> is
 * "convolve", "convolve_configure", "convolve_reset", "fetch_convolved", "convolve plan", "convolve design", "convolve check",
 * "convolve response" or "convolve frames".
 *
 * RECORD.  The counts and the peak run since the stream's reset, as in the resample record; they are integer sums and a maximum, so
 * the record does not depend on the schedule. */
#ifndef OMX_PROGRAM_CONVOLVE_H
#define OMX_PROGRAM_CONVOLVE_H

#include "program_mix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_CONVOLVE_MAX_TAPS 4096u          /* taps of one FIR */
#define OMX_CONVOLVE_MAX_FIRS 64u            /* FIRs of one table */
#define OMX_CONVOLVE_BYPASS 0xFFFFFFFFu      /* fir_of_channel: the channel is copied, not filtered */

#define OMX_CONVOLVE_LOWPASS 0u              /* omx_program_convolve_spec.kind */
#define OMX_CONVOLVE_HIGHPASS 1u
#define OMX_CONVOLVE_BANDPASS 2u
#define OMX_CONVOLVE_BANDSTOP 3u

#define OMX_CONVOLVE_IDLE 0u                 /* omx_program_convolve_record.state: no frame taken since the reset */
#define OMX_CONVOLVE_RUNNING 1u
#define OMX_CONVOLVE_FLUSHED 2u              /* the tail has been emitted; the stream takes no more frames until it is reset */

typedef struct omx_program_fir {
    const float* taps;              /* host array [n_taps], every tap finite */
    uint32_t n_taps;                /* 1 .. OMX_CONVOLVE_MAX_TAPS */
    uint32_t flags;                 /* must be 0 */
} omx_program_fir;                  /* 16 bytes */

typedef struct omx_program_convolve_spec {
    uint32_t kind;                  /* OMX_CONVOLVE_LOWPASS .. BANDSTOP */
    uint32_t n_taps;                /* T: odd, 3 .. 4095 */
    double f_lo_hz, f_hi_hz;        /* LOWPASS uses f_hi_hz, HIGHPASS f_lo_hz, the band kinds both (f_lo_hz < f_hi_hz) */
    double beta;                    /* Kaiser beta, 0 .. 20 */
} omx_program_convolve_spec;        /* 32 bytes */

typedef struct omx_program_convolve_info {
    uint32_t tile_frames;           /* output frames one workgroup of the main kernel computes at this channel count */
    uint32_t frames_per_thread;     /* consecutive output frames of one channel a thread keeps in registers */
    uint32_t tap_block;             /* taps per staging of the input span; a longer FIR runs in blocks of ascending k */
    uint32_t channels;
} omx_program_convolve_info;        /* 16 bytes */

typedef struct omx_program_convolve_record {
    uint64_t frames_in;             /* N: frames taken since the reset */
    uint64_t frames_out;            /* E: frames emitted since the reset */
    uint64_t frames_written;        /* frames this call wrote to d_out[s] */
    uint64_t samples_over;          /* samples with |out| > 1.0f (NaN is not counted, infinity is), since the reset */
    uint64_t samples_nonfinite;     /* samples that are NaN or infinite, since the reset */
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored), since the reset */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t state;                 /* OMX_CONVOLVE_IDLE / RUNNING / FLUSHED */
    uint32_t delay_frames;          /* D */
    uint32_t max_taps;              /* the longest FIR the table's channels reference */
    uint32_t _pad;
} omx_program_convolve_record;      /* 64 bytes */

/* ---- host only, no device needed */

/* The main kernel's tile, register window and tap block at a channel count, for a table whose longest FIR has max_taps taps.
 * OMX_ERR_INVALID, with nothing written: channels outside 1 .. 8, max_taps 0 or above OMX_CONVOLVE_MAX_TAPS, a null info. */
int omx_program_convolve_plan(uint32_t channels, uint32_t max_taps, omx_program_convolve_info* info);
/* *frames_out = E' - E of a stream under delay D that has taken frames_in_before and emitted frames_out_before frames and now takes
 * `frames` more, with (flush != 0) or without a flush: the STREAMING formula, so that a host can size d_out.
 * OMX_ERR_INVALID, with nothing written: a null frames_out, delay above OMX_CONVOLVE_MAX_TAPS - 1, frames_in_before + frames beyond
 * 2^63, frames_out_before above frames_in_before. */
int omx_program_convolve_frames(uint32_t delay_frames, uint64_t frames_in_before, uint64_t frames_out_before, uint64_t frames,
                                uint32_t flush, uint64_t* frames_out);
/* OMX_NONE for a FIR the bank takes.  OMX_ERR_INVALID: a null pointer, null taps, n_taps 0 or above OMX_CONVOLVE_MAX_TAPS, a flag
 * set, a tap that is not finite. */
int omx_program_convolve_check(const omx_program_fir* fir);
/* The taps of a spec at a sample rate (DESIGN FORMULAS) into taps_out[0 .. n_taps).  OMX_ERR_INVALID, with nothing written: a null
 * pointer, an unknown kind, n_taps even or outside 3 .. 4095, a sample rate that is not finite or not positive, a frequency the kind
 * uses that is not finite, not positive or at or above sample_rate / 2, f_lo_hz >= f_hi_hz where both are used, beta not finite or
 * outside [0, 20], n_floats != n_taps. */
int omx_program_convolve_design(const omx_program_convolve_spec* spec, double sample_rate, float* taps_out, uint32_t n_floats);
/* H(e^{jw}) = sum over k of h[k] e^{-jwk} at w = 2 pi frequency_hz / sample_rate, summed in f64 in order of increasing k:
 * 20 log10 |H| (-infinity at a zero) and arg H in (-pi, pi].  Either result pointer may be null.  OMX_ERR_INVALID: whatever
 * omx_program_convolve_check refuses, a rate or frequency that is not finite, a rate that is not positive, a negative frequency. */
int omx_program_convolve_response(const omx_program_fir* fir, double sample_rate, double frequency_hz, double* magnitude_db,
                                  double* phase_rad);

/* ---- the bank */

/* firs: host array [n_firs]; fir_of_channel: host array [n_streams][channels] of table indices or OMX_CONVOLVE_BYPASS, NULL = FIR 0
 * on every channel.  Checks every FIR as omx_program_convolve_check does, uploads the tables, allocates the carried frames and the
 * records and leaves every stream idle.  Allowed only while no stream of the stage holds frames: a new bank, or after convolve_reset
 * of every stream.  max_taps is the longest FIR a channel references (1 when every channel is bypassed).  Synchronises.
 * OMX_ERR_INVALID, with nothing changed: channels outside 1 .. 8, a null table, n_firs 0 or above OMX_CONVOLVE_MAX_FIRS, an index
 * that is neither below n_firs nor OMX_CONVOLVE_BYPASS, a FIR that check refuses, delay_frames > max_taps - 1, a stream that holds
 * frames. */
int omx_program_loudness_bank_convolve_configure(omx_program_loudness_bank* b, uint32_t channels, const omx_program_fir* firs,
                                                 uint32_t n_firs, const uint32_t* fir_of_channel, uint32_t delay_frames);
/* The flagged streams (host array [n_streams]; NULL: every stream) forget their frames and are idle again.  OMX_ERR_INVALID before
 * configure. */
int omx_program_loudness_bank_convolve_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_in: device f32 [n_streams][frames_capacity][channels]; frames: host array [n_streams] or NULL = frames_capacity for every stream.
 * d_out: device f32 [n_streams][out_capacity][channels]; stream s gets its emitted frames at d_out[s][0 ..), no float at or beyond
 * frames_written[s] * channels is written.  flush_mask: host array [n_streams] or NULL = no stream.  Out of place only: any overlap
 * of d_in and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; frames for a flushed stream; a stream that would emit more than out_capacity frames;
 * frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a null d_in when any stream brings frames, a null d_out when any stream
 * emits; a null d_convolved.
 * A refused call changes nothing: neither d_out nor the records nor the stage's state.
 * *d_convolved: device array [n_streams] of the running records, valid until convolve_configure or destroy; work on `stream` that
 * reads it has to be ordered behind the call.  Returns OMX_PRODUCED when any stream emitted a frame, else OMX_NONE. */
int omx_program_loudness_bank_convolve(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       float* d_out, uint64_t out_capacity, const uint8_t* flush_mask, void* stream,
                                       const omx_program_convolve_record** d_convolved);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_convolved(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_convolve_record* dst);

#ifdef __cplusplus
}
#endif
#endif

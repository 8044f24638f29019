/* Programme loudness bank, spectrum: an IIR filter stage on device PCM.  The bank can change a signal's level, length, layout, rate and
 * format; this header lets it change the spectrum: take out the DC offset that inspect reports (program_inspect.h), low-pass the LFE
 * in front of a fold-down (program_remix.h), undo or apply 50/15 us and 75 us emphasis, and the highpass / lowpass / equalizer / bass /
 * treble of a delivery chain, without the PCM going back to the host.
 *
 * Additive: this header adds five structures, twelve functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls filter_configure allocates and launches nothing more.  All work
 * goes on the caller's stream; only fetch_filtered and filter_configure synchronise.  No call of this header touches measurement
 * state, gain plans or the records of any other stage.
 *
 * A filter is a cascade of at most OMX_FILTER_MAX_SECTIONS (2) biquad sections: four f64 of state per channel.  A longer cascade is a
 * second pass over the PCM (a second bank call with another table) and is out of the scope of this header.
 *
 * DEFINITION ("Filter"; tests/program_filter_ref.py restates it).  Per stream and channel; the state s1, s2 of
 * each section is f64 and zero after a reset:
 *     v = (double)x[n][c]
 *     for each section k < n_sections, in order:
 *         y  = b0 * v + s1
 *         s1 = (b1 * v - a1 * y) + s2
 *         s2 =  b2 * v - a2 * y
 *         v  = y
 *     out[n][c] = (float)v            (round to nearest even; f32 denormals are produced, nothing is flushed)
 *   Every product and every sum is rounded to f64 once, nothing is fused.  The state is carried from call to call, so in reference
 *   order the output does not depend, in any bit, on how the programme is cut into calls.
 *   A channel on OMX_FILTER_BYPASS copies its bits: -0.0f, infinities and NaN payloads included.
 *   A sample that is not finite enters the arithmetic as it is; it poisons that channel's state until filter_reset, and the record
 *   counts what comes out.  Which NaN the arithmetic produces (its sign and payload) is the hardware's choice; only a bypass keeps them.
 *
 * EVALUATION ORDER.  Reference order runs the recurrence as written.  The time-parallel form cuts a call into work items of
 * chunk_frames frames, finds every item's start state (zero-state end states as dot products, a double-double scan of the zero-input
 * transition) and runs the items side by side; its output differs from reference order by at most one f32 ulp of the stream's
 * loudest sample (2^-23 x max(peak in, peak out)), and a table with a filter that cannot hold that runs in reference order whatever
 * is asked for (DESIGN.md gives the rule).  With an infinity in the input the two forms agree on where the output stops being finite,
 * not on infinity against NaN.
 *
 * DESIGN FORMULAS (host only; sin, cos, tan, sqrt and pow are the only library functions).  fs = sample rate, f = frequency_hz.
 *   w0 = 2 pi f / fs,  cs = cos(w0),  al = sin(w0) / (2 Q),  Q = q or 1/sqrt(2) when q == 0,  A = pow(10, gain_db / 40).
 *   Every RBJ section is divided by its a0.
 *   LOWPASS  order 1: K = tan(pi f / fs); b0 = b1 = K / (1 + K), b2 = 0; a1 = (K - 1) / (K + 1), a2 = 0.
 *   HIGHPASS order 1: b0 = 1 / (1 + K), b1 = -b0, b2 = 0; a1, a2 as LOWPASS.
 *   LOWPASS  order 2 (RBJ): b0 = b2 = (1 - cs) / 2, b1 = 1 - cs; a0 = 1 + al, a1 = -2 cs, a2 = 1 - al.
 *   HIGHPASS order 2 (RBJ): b0 = b2 = (1 + cs) / 2, b1 = -(1 + cs); a as LOWPASS.
 *   order 4 (Butterworth): two order-2 sections with Q = 1 / sqrt(2 + sqrt(2)) = 0.54119610 and 1 / sqrt(2 - sqrt(2)) = 1.30656296;
 *            q is not used.
 *   LOW_SHELF  (RBJ): r = 2 sqrt(A) al;  b0 = A ((A+1) - (A-1) cs + r), b1 = 2 A ((A-1) - (A+1) cs), b2 = A ((A+1) - (A-1) cs - r);
 *            a0 = (A+1) + (A-1) cs + r, a1 = -2 ((A-1) + (A+1) cs), a2 = (A+1) + (A-1) cs - r.
 *   HIGH_SHELF (RBJ): b0 = A ((A+1) + (A-1) cs + r), b1 = -2 A ((A-1) + (A+1) cs), b2 = A ((A+1) + (A-1) cs - r);
 *            a0 = (A+1) - (A-1) cs + r, a1 = 2 ((A-1) - (A+1) cs), a2 = (A+1) - (A-1) cs - r.
 *   PEAKING (RBJ): b0 = 1 + al A, b1 = -2 cs, b2 = 1 - al A; a0 = 1 + al / A, a1 = -2 cs, a2 = 1 - al / A.
 *   NOTCH   (RBJ): b0 = 1, b1 = -2 cs, b2 = 1; a0 = 1 + al, a1 = -2 cs, a2 = 1 - al.
 *   DC_BLOCK: y = x - x1 + R y1 with R = 1 - 2 pi f / fs:  b0 = 1, b1 = -1, b2 = 0; a1 = -R, a2 = 0.
 *   DEEMPHASIS: the analogue (1 + s t2) / (1 + s t1), t1 = time_constant_us, t2 = time_constant_zero_us (0: no zero; 50 / 15 us gives
 *            the pair), through s = 2 fs (1 - 1/z) / (1 + 1/z).  k1 = 2 fs t1, k2 = 2 fs t2:
 *            b0 = (1 + k2) / (1 + k1), b1 = (1 - k2) / (1 + k1), b2 = 0; a1 = (1 - k1) / (1 + k1), a2 = 0.
 *   PREEMPHASIS: the exact inverse section: b0 = (1 + k1) / (1 + k2), b1 = (1 - k1) / (1 + k2); a1 = (1 - k2) / (1 + k2).  Without a
 *            zero (t2 = 0) its pole lies on the unit circle and the design is refused as unstable.
 *
 * RECORD.  Written fresh by every call.  The counts are integer sums and the peak a maximum: the record does not depend on the
 * schedule. */
#ifndef OMX_PROGRAM_FILTER_H
#define OMX_PROGRAM_FILTER_H

#include "program_peak_timeline.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_FILTER_MAX_SECTIONS 2u
#define OMX_FILTER_MAX_FILTERS 256u       /* filters of one table */
#define OMX_FILTER_BYPASS 0xFFFFFFFFu     /* filter_of_channel: the channel is copied, not filtered */

#define OMX_FILTER_HIGHPASS 0u            /* omx_program_filter_spec.kind */
#define OMX_FILTER_LOWPASS 1u
#define OMX_FILTER_LOW_SHELF 2u
#define OMX_FILTER_HIGH_SHELF 3u
#define OMX_FILTER_PEAKING 4u
#define OMX_FILTER_NOTCH 5u
#define OMX_FILTER_DC_BLOCK 6u
#define OMX_FILTER_DEEMPHASIS 7u
#define OMX_FILTER_PREEMPHASIS 8u

typedef struct omx_program_filter_section {
    double b0, b1, b2, a1, a2;      /* a0 = 1 */
} omx_program_filter_section;       /* 40 bytes */

typedef struct omx_program_filter {
    uint32_t n_sections;            /* 1 .. OMX_FILTER_MAX_SECTIONS */
    uint32_t _pad;
    omx_program_filter_section section[OMX_FILTER_MAX_SECTIONS];
} omx_program_filter;               /* 88 bytes */

typedef struct omx_program_filter_spec {
    uint32_t kind;                  /* OMX_FILTER_* */
    uint32_t order;                 /* HIGHPASS / LOWPASS: 1, 2 or 4; every other kind: 0 or the kind's own order */
    double frequency_hz;            /* corner, centre or DC_BLOCK frequency; not used by the emphasis kinds */
    double q;                       /* order-2 HIGHPASS / LOWPASS, shelves, PEAKING, NOTCH; 0: 1/sqrt(2) */
    double gain_db;                 /* shelves and PEAKING */
    double time_constant_us;        /* emphasis kinds: the pole (the zero for PREEMPHASIS) */
    double time_constant_zero_us;   /* emphasis kinds: the other time constant of a pair, below time_constant_us; 0: none */
} omx_program_filter_spec;          /* 48 bytes */

typedef struct omx_program_filter_info {
    uint32_t chunk_frames;          /* frames per work item of the time-parallel form */
    uint32_t tile_frames;           /* frames per LDS tile of the kernels */
    uint32_t channels;
    uint32_t streams_per_wavefront; /* streams one wavefront of the pass takes under this channel count */
} omx_program_filter_info;          /* 16 bytes */

typedef struct omx_program_filter_record {
    uint64_t frames;                /* frames this call filtered for the stream */
    uint64_t frames_total;          /* frames since the stream's reset */
    uint64_t samples_over;          /* output samples of this call with |out| > 1.0f (NaN is not counted, infinity is) */
    uint64_t samples_nonfinite;     /* output samples of this call that are NaN or infinite */
    float out_sample_peak;          /* max |out| of this call, fmaxf semantics (NaN ignored) */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t form;                  /* the evaluation order that ran: 1 reference order, 2 time-parallel; 0: no frames yet */
    uint32_t _pad;
} omx_program_filter_record;        /* 48 bytes */

/* ---- host only, no device needed, C double arithmetic */

/* The filter of a spec at a sample rate (the formulas above).  OMX_ERR_INVALID, with nothing written: a null pointer, an unknown
 * kind, an order the kind does not have, a sample rate that is not finite or not positive; for the kinds that use them a frequency
 * that is not finite, not positive or at or above sample_rate / 2, a q that is not finite or negative, a gain that is not finite, a
 * time constant that is not finite or not positive, a zero time constant that is not finite, negative or not below the other.
 * OMX_ERR_UNSUPPORTED, with nothing written: the designed filter is not strictly stable (omx_program_filter_check). */
int omx_program_filter_design(const omx_program_filter_spec* spec, double sample_rate, omx_program_filter* filter);
/* out = the sections of a, then those of b (out may be a or b).  OMX_ERR_INVALID, with nothing written: a null pointer, a section
 * count outside 1 .. 2 in a or b, more than OMX_FILTER_MAX_SECTIONS sections together. */
int omx_program_filter_cascade(const omx_program_filter* a, const omx_program_filter* b, omx_program_filter* out);
/* OMX_NONE for a filter the bank takes.  OMX_ERR_INVALID: null, n_sections outside 1 .. 2, a coefficient that is not finite.
 * OMX_ERR_UNSUPPORTED: a section that is not strictly stable, that is, not |a2| < 1 && |a1| < 1 + a2. */
int omx_program_filter_check(const omx_program_filter* filter);
/* H(e^{jw}) at w = 2 pi frequency_hz / sample_rate from the coefficients: 20 log10 |H| (-infinity at a zero) and arg H in
 * (-pi, pi].  Either result pointer may be null.  OMX_ERR_INVALID: a null filter, a section count outside 1 .. 2, a rate or
 * frequency that is not finite, a rate that is not positive, a negative frequency. */
int omx_program_filter_response(const omx_program_filter* filter, double sample_rate, double frequency_hz, double* magnitude_db,
                                double* phase_rad);
/* The work item of the time-parallel form and the tile of the kernels.  OMX_ERR_INVALID, with nothing written: channels outside
 * 1 .. 8, a sample rate that is not finite or not positive, a null info. */
int omx_program_filter_plan(uint32_t channels, double sample_rate, omx_program_filter_info* info);

/* ---- the bank */

/* filters: host array [n_filters]; filter_of_channel: host array [n_streams][channels] of table indices or OMX_FILTER_BYPASS, NULL =
 * filter 0 on every channel.  Checks every filter as omx_program_filter_check does, makes the time-parallel tables on the host,
 * allocates state and records and resets every stream.  Allowed only while no stream holds filter state: a new bank, or after
 * filter_reset of every stream.  Synchronises.
 * OMX_ERR_INVALID, with nothing changed: channels outside 1 .. 8, a sample rate that is not finite or not positive, a null table,
 * n_filters 0 or above OMX_FILTER_MAX_FILTERS, an index that is neither below n_filters nor OMX_FILTER_BYPASS, a filter that check
 * calls invalid, a stream that holds state.  OMX_ERR_UNSUPPORTED, with nothing changed: a filter that is not strictly stable. */
int omx_program_loudness_bank_filter_configure(omx_program_loudness_bank* b, uint32_t channels, double sample_rate,
                                               const omx_program_filter* filters, uint32_t n_filters, const uint32_t* filter_of_channel);
/* The flagged streams start over with zero state and a zero record (NULL: every stream). */
int omx_program_loudness_bank_filter_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_in, d_out: device f32 [n_streams][frames_capacity][channels]; frames: host array [n_streams] or NULL = frames_capacity for every
 * stream.  d_out == d_in filters in place; any other overlap is OMX_ERR_INVALID.  No float of d_out[s] at or beyond
 * frames[s] * channels is written.
 * Also OMX_ERR_INVALID: a call before configure; frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a null d_in or d_out when
 * any stream brings frames; a null d_filtered.  A refused call changes nothing: neither d_out nor the state nor the records.
 * *d_filtered: device array [n_streams] of this call's records, valid until filter_configure or destroy.  Returns OMX_PRODUCED when
 * any stream brought a frame, else OMX_NONE. */
int omx_program_loudness_bank_filter(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                     float* d_out, void* stream, const omx_program_filter_record** d_filtered);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_filtered(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_filter_record* dst);
/* 0 = by call shape, 1 = reference order, 2 = time-parallel (a table that cannot hold the parity bar still runs in reference order).
 * Apart from OMX_OPT_KERNEL_FORM, whose meaning for process does not change.  OMX_ERR_INVALID: another value. */
int omx_program_loudness_bank_filter_set_form(omx_program_loudness_bank* b, uint32_t form);
/* The form the last filter call ran (1 or 2; 0 before the first). */
int omx_debug_program_loudness_bank_filter_last_form(const omx_program_loudness_bank* b);

#ifdef __cplusplus
}
#endif
#endif

/* Programme loudness bank, PCM formats: integer PCM in and out.  The programmes people measure are 16- or 24-bit files and
 * "-14 LUFS, -1 dBTP" is delivered as one; every earlier pass of the bank takes and gives f32.  With this header the host uploads the
 * file's bytes as they are (import), and turns the limiter's f32 output into the delivery format on the device, with TPDF dither whose
 * values do not depend on how the programme was cut into calls (export).  The host writes no conversion kernel of its own.
 *
 * Additive: this header adds two structures, seven functions and a few constants; nothing declared in the headers it includes changes
 * and OMX_ABI_VERSION stays as it is.  A bank that never calls one of them allocates and launches nothing more.  All work goes on the
 * caller's stream; only fetch_exported synchronises.  No call of this header touches measurement state, gain plans, apply records or
 * the limiter: every record of the earlier headers has the same bytes before and after.
 *
 * FORMATS.  Little-endian, interleaved, [n_streams][frames_capacity][channels]; a row is frames_capacity * channels * bytes bytes, no
 * padding.  OMX_PCM_S16: 2 bytes per sample.  OMX_PCM_S24: 3 bytes per sample, packed (the WAV form).  OMX_PCM_S32: 4 bytes.  The
 * integer buffer's base must be 4-byte aligned (else OMX_ERR_INVALID); rows then start at whatever byte offset follows (an S24 row
 * of 3 x 1001 samples is 9009 bytes: the next row starts on an odd address).  B is the format's bit count.
 *
 * DEFINITION ("PCM formats"; tests/program_pcm_ref.py restates it).
 *   Import   stateless.  S16: x = (float)v * 2^-15, exact.  S24: x = (float)v * 2^-23, exact, v the sign-extended 24-bit value.
 *            S32: x = (float)v * 2^-31: the conversion to f32 rounds to nearest even, the scale is then exact.
 *   Export   for stream s, absolute frame n (frames exported since the stream's last export reset) and channel c:
 *     NaN    a NaN input gives y = 0 and counts in samples_nan, not in samples_clipped and not in the peak.
 *     Scale  sv = (double)x * 2^(B-1), exact.
 *     Dither OMX_DITHER_NONE: d = 0.  OMX_DITHER_TPDF:
 *              mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31   (u64, wrapping)
 *              key_s = mix(seed + 0x9E3779B97F4A7C15 * (s + 1))
 *              h     = mix(key_s + 0x9E3779B97F4A7C15 * (n * 8 + c))
 *              a = h & 0xFFFFFF;  b = (h >> 24) & 0xFFFFFF;  d = (double)((int64)a - (int64)b) * 2^-24
 *            d is triangular on (-1, 1) LSB and a function of (seed, stream, absolute frame, channel) only.
 *     Round  t = sv + d, one f64 add; r = floor(t + 0.5), one more f64 add and a floor (no step is fused).
 *     Clamp  y = clamp(r, -2^(B-1), 2^(B-1) - 1), in f64 before the conversion to an integer; a sample with r outside that range
 *            counts in samples_clipped (infinities too).
 *     Peak   out_peak = max |y| as a u32 (2^31 is possible);
 *            out_peak_db = power_to_db(p * p, floor_db) with p = (float)((double)out_peak / 2^(B-1)), as program_peaks.h.
 *   Every count is a sum and the peak a maximum of integers: the record does not depend on the run, and neither the bytes nor the
 *   record depend, in any bit, on how the programme is cut into calls. */
#ifndef OMX_PROGRAM_PCM_H
#define OMX_PROGRAM_PCM_H

#include "program_limit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_PCM_S16 1u   /* 2 bytes per sample */
#define OMX_PCM_S24 2u   /* 3 bytes per sample, packed */
#define OMX_PCM_S32 3u   /* 4 bytes per sample */

#define OMX_DITHER_NONE 0u
#define OMX_DITHER_TPDF 1u

typedef struct omx_program_export_rule {
    uint32_t format;        /* OMX_PCM_* */
    uint32_t dither;        /* OMX_DITHER_NONE / OMX_DITHER_TPDF */
    uint64_t seed;
    uint32_t flags;         /* must be 0 */
    uint32_t _pad;
} omx_program_export_rule;  /* 24 bytes */

typedef struct omx_program_export_record {
    uint64_t frames_out;        /* exported since the reset: the next dither position */
    uint64_t frames_written;    /* by this call */
    uint64_t samples_clipped;   /* since the reset */
    uint64_t samples_nan;       /* since the reset */
    uint32_t out_peak;          /* max |y| since the reset */
    float    out_peak_db;
    uint32_t format, dither;
} omx_program_export_record;    /* 48 bytes */

/* Host only, needs no device: *bytes = bytes per sample of `format`.  OMX_ERR_INVALID, with nothing written: an unknown format, a
 * null bytes. */
int omx_pcm_format_bytes(uint32_t format, uint32_t* bytes);
/* Host only, needs no device: *d = the dither value, in LSB, of (rule->seed, stream, frame, channel); 0 with OMX_DITHER_NONE.  It runs
 * the inline function the export kernel runs.  OMX_ERR_INVALID, with nothing written: a null rule or d, an unknown format or dither,
 * a flag set, channel above 7. */
int omx_program_dither_evaluate(const omx_program_export_rule* rule, uint64_t stream, uint64_t frame, uint32_t channel, double* d);

/* d_in: device integer PCM of `format`, [n_streams][frames_capacity][channels], base 4-byte aligned.  d_out: device f32 of the same
 * shape, the layout of omx_program_loudness_bank_process.  Out of place: any overlap of the two buffers is OMX_ERR_INVALID.  frames:
 * host array [n_streams] or NULL = frames_capacity for every stream.  Frames at or above frames[s] of d_out are not written.
 * Also OMX_ERR_INVALID, as for apply_gains: channels outside 1 .. 8, frames[s] > frames_capacity, frames_capacity > 2^32 - 1, a null
 * d_in or d_out when any stream brings frames; and an unknown format, a d_in that is not 4-byte aligned.  A refused call changes
 * nothing.  Stateless: the bank lends its stream count and its staging.  Returns OMX_PRODUCED when any stream brought a frame, else
 * OMX_NONE. */
int omx_program_loudness_bank_import_pcm(omx_program_loudness_bank* b, const void* d_in, uint32_t format, float* d_out,
                                         uint64_t frames_capacity, const uint32_t* frames, uint32_t channels, void* stream);

/* Sets the rule and the channel count of the PCM the export takes, allocates the records and leaves every stream at position 0.
 * Allowed only while every stream's position is 0 (a new bank, or every stream reset): otherwise OMX_ERR_INVALID and nothing changes.
 * Also OMX_ERR_INVALID: a null rule, an unknown format or dither, a flag set, channels outside 1 .. 8. */
int omx_program_loudness_bank_export_configure(omx_program_loudness_bank* b, const omx_program_export_rule* rule, uint32_t channels);
/* The flagged streams (host array [n_streams]; NULL: every stream) start over: position and record back to zero, the dither at frame
 * 0 again.  OMX_ERR_INVALID before configure. */
int omx_program_loudness_bank_export_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);

/* d_in: device f32 [n_streams][frames_capacity][channels].  d_out: device integer PCM of the rule's format and the same shape, base
 * 4-byte aligned.  frames: host array [n_streams] or NULL = frames_capacity for every stream; stream s exports frames[s] frames, which
 * take the dither positions frames_out .. frames_out + frames[s] - 1.  Bytes of d_out at or beyond a stream's frames[s] are not
 * written, the bytes that share a dword with the row's last sample or with the next row's first included.  Out of place only: any
 * overlap of d_in and d_out is OMX_ERR_INVALID.
 * Also OMX_ERR_INVALID: a call before configure; frames[s] > frames_capacity; frames_capacity > 2^32 - 1; a null d_in or d_out when any
 * stream brings frames; a d_out that is not 4-byte aligned; a null d_exported.
 * A refused call changes nothing: neither d_out nor the records nor a stream's position.
 * *d_exported: device array [n_streams] of the running records, valid until export_configure or destroy; work on `stream` that reads
 * it has to be ordered behind the call.  The host mirrors every stream's position and hands it to the kernels with the call: there
 * is no device-side position.  Returns OMX_PRODUCED when any stream brought a frame, else OMX_NONE. */
int omx_program_loudness_bank_export_pcm(omx_program_loudness_bank* b, const float* d_in, void* d_out, uint64_t frames_capacity,
                                         const uint32_t* frames, void* stream, const omx_program_export_record** d_exported);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_exported(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_export_record* dst);

#ifdef __cplusplus
}
#endif
#endif

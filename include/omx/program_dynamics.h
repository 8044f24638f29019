/* Programme loudness bank, dynamics: a compressor and expander stage on device PCM.  The bank measures a programme, reshapes it,
 * changes its spectrum and sets its level; the only stage with a time-varying gain is the limiter (program_limit.h), which catches
 * peaks over a ceiling and nothing else.  This header adds the sample-level tool next to it: a gain that follows the level of the
 * programme, or of a side chain, through a transfer curve, with a look-ahead attack, a hold and a release that is linear in dB.
 * It narrows a loudness range, ducks music under a voice stem before mix, and pushes a noise floor down.
 *
 * Additive: this header adds five structures, eleven functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls dynamics_configure allocates and launches nothing more.  All
 * work goes on the caller's stream; only fetch_dynamics and dynamics_configure synchronise.  No call of this header touches
 * measurement state, gain plans or the records of any other stage.
 *
 * DEFINITION ("Dynamics"; tests/program_dynamics_ref.py restates it).  Per stream, x[n][c] is the PCM taken
 * since the stage's last reset, n = 0 .. N-1, and key[n][c] the side-chain PCM of the same frame (d_key, or x where d_key is NULL).
 * The stream's curve gives T[769], detector_mask, A = attack_frames, H = hold_frames and d = release_step.
 *   Level     a[n] = the maximum over the channels c in detector_mask of fabsf(key[n][c]), fmaxf semantics: a NaN is ignored, a
 *             frame whose every detector sample is NaN gives 0.  L[n] is an int32 in units of 2^-16 octave (0 = full scale 1.0):
 *             L_MIN = -40 * 65536 where !(a >= 2^-40) (zeros and f32 denormals land here), L_MAX = 8 * 65536 where a >= 256 (an
 *             infinity lands here); otherwise, from the f32 bits of a with unbiased exponent e and mantissa m: i = m >> 15,
 *             f = m & 0x7FFF, L = e * 65536 + LOG[i] + (((LOG[i+1] - LOG[i]) * f + 2^14) >> 15).
 *   Tables    LOG[i] = floor(65536 * log2(1 + i/256)) and EXP[i] = floor(2^(40 + i/256)), i = 0 .. 256: exact integers, literals in
 *             the source (omx_program_dynamics_tables exports them); no libm at run time.
 *   Curve     T[k] is the gain, in 2^-16 octave, at level L_MIN + 4096 * k; |T[k]| <= 40 * 65536.  k = (L - L_MIN) >> 12,
 *             f = (L - L_MIN) & 4095; Gt[n] = T[k] where f == 0, else T[k] + (((T[k+1] - T[k]) * f + 2048) >> 12), the product in
 *             64 bits, the shift arithmetic.  Gt[n] = T[0] for n < 0, and for n >= N once the stream is flushed: the programme is
 *             preceded and followed by digital silence.
 *   Hold      w[n] = min(Gt[n-W+1 .. n]), W = A + H.
 *   Release   r[n] = min(w[n] * 2^16, r[n-1] + d), an int64 in units of 2^-32 octave; r[n] = T[0] * 2^16 for n < 0.  Because
 *             r <= w * 2^16 <= 40 * 2^32 always holds, the ramp term may be saturated at 40 * 2^32 without changing a bit.
 *   Smooth    S[n] = sum(r[n-A+1 .. n]) as an int64; E[j] = floor(S[j + A - 1] / A), floor division of a signed value.  LA = A - 1
 *             is the latency in frames.  E[j] <= Gt[t] * 2^16 for every t in [j-H, j]; on a constant level E settles to the
 *             curve's value exactly.
 *   Factor    I = E >> 32 (arithmetic), F = E & 0xFFFFFFFF, i = F >> 24, g = F & 0xFFFFFF;
 *             fx = EXP[i] + (((EXP[i+1] - EXP[i]) * g) >> 24) as a u64; k[j] = ldexp((double)fx, I - 40), exact in f64.
 *   Output    out[j][c] = (float)((double)x[j][c] * k[j]): one f64 product, one rounding to f32.  A frame with E[j] == 0 copies its
 *             bits, NaN payloads and -0.0f included.  The gain goes to every channel of the stream.  The bits of a NaN the
 *             arithmetic produces are not defined.
 *   Bypass    A stream on OMX_DYNAMICS_BYPASS copies every frame on bits, delayed by the largest LA of the table's curves, so that
 *             it stays aligned with the active streams of a bank whose curves share one attack.
 *   Trace     d_gain_db, where given, gets (float)((double)E[j] * (6.020599913279624 / 4294967296.0)) for every emitted frame.
 * Every quantity between the f32 level and the f64 factor is an integer, so any parallel schedule gives the same bits, and the
 * output does not depend, in any bit, on how the programme is cut into calls.
 *
 * STREAMING (the limiter's model).  Per stream the host mirrors N frames taken, E frames emitted and a flushed flag.  A call that
 * brings F frames sets N += F and emits frames [E, E') to d_out[s][0 ..): E' = max(E, N > LA ? N - LA : 0) without a flush, E' = N
 * with the stream flagged in flush_mask.  A flushed stream takes no more frames until it is reset.  Out of place only.
 *
 * DESIGN FORMULAS (host only, f64, every step its own operation, no library function but floor).  U = 6.020599913279624 dB is one
 * octave.  Entry k is at x = (double)(L_MIN + 4096 * k) / 65536.0 * U dB; a gain g in dB becomes
 * T[k] = (int32)floor(min(max(g, -40 U), 40 U) / U * 65536.0 + 0.5).
 *   design    c = x - threshold_db.  2c < -knee: gc = 0.  knee > 0 and |2c| <= knee: gc = (1/ratio - 1) * (c + knee/2)^2 / (2 knee).
 *             Else gc = (1/ratio - 1) * c.  ge = 0 where expander_ratio == 1 or x >= expander_threshold_db, else
 *             max((x - expander_threshold_db) * (expander_ratio - 1), -range_db).  g = gc + ge + makeup_db.
 *   points    (in_db, out_db) pairs with strictly increasing in_db.  Below the first pair and above the last the slope is 1:
 *             g = out - in of that pair.  Between pairs p and p+1: y = out[p] + (x - in[p]) * ((out[p+1] - out[p]) / (in[p+1] - in[p])),
 *             g = y - x.  This is the transfer function of sox compand.
 *   gain_db   L = (int32)floor(level_db / U * 65536.0 + 0.5) clamped to [L_MIN, L_MAX], Gt as in Curve, result (double)Gt * (U / 65536.0).
 *   time      A = max(1, floor(attack_ms * fs / 1000 + 0.5)), H = floor(hold_ms * fs / 1000 + 0.5),
 *             d = floor(release_db_per_s / U * 4294967296.0 / fs + 0.5) clamped to [1, 40 * 2^32] (an infinite rate is the maximum).
 *
 * REFUSALS.  A refused call returns OMX_ERR_INVALID, writes nothing and sets omx_last_error() to "program loudness <who>: <why>",
 * where <who> is "dynamics", "dynamics_configure", "dynamics_reset", "fetch_dynamics", "dynamics plan", "dynamics design",
 * "dynamics points", "dynamics check", "dynamics gain", "dynamics time", "dynamics latency" or "dynamics frames".
 *
 * RECORD.  Counts and extrema run since the stream's reset; they are integer sums, integer extrema and a maximum on bit patterns,
 * so the record does not depend on the schedule. */
#ifndef OMX_PROGRAM_DYNAMICS_H
#define OMX_PROGRAM_DYNAMICS_H

#include "program_convolve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_DYNAMICS_CURVE_POINTS 769u       /* entries of a curve: levels L_MIN .. L_MAX in steps of 4096 */
#define OMX_DYNAMICS_TABLE_ENTRIES 257u      /* entries of LOG and of EXP */
#define OMX_DYNAMICS_MAX_CURVES 64u          /* curves of one table */
#define OMX_DYNAMICS_MAX_POINTS 16u          /* pairs omx_program_dynamics_from_points takes */
#define OMX_DYNAMICS_MAX_ATTACK 4096u
#define OMX_DYNAMICS_MAX_HOLD 16384u
#define OMX_DYNAMICS_L_MIN (-40 * 65536)
#define OMX_DYNAMICS_L_MAX (8 * 65536)
#define OMX_DYNAMICS_MAX_GAIN (40 * 65536)   /* |T[k]| is at or below this */
#define OMX_DYNAMICS_MAX_STEP 171798691840ll /* 40 * 2^32: the largest release_step, an instant release */
#define OMX_DYNAMICS_OCTAVE_DB 6.020599913279624
#define OMX_DYNAMICS_BYPASS 0xFFFFFFFFu      /* curve_of_stream: the stream is copied, delayed, not processed */

#define OMX_DYNAMICS_IDLE 0u                 /* omx_program_dynamics_record.state: no frame taken since the reset */
#define OMX_DYNAMICS_RUNNING 1u
#define OMX_DYNAMICS_FLUSHED 2u              /* everything taken has been emitted; the stream takes no more frames until it is reset */

typedef struct omx_program_dynamics_curve {
    int32_t T[769];                 /* gain in 2^-16 octave at level L_MIN + 4096 k */
    uint32_t detector_mask;         /* bit c: channel c takes part in the level; at least one bit, none at or above bit 8 */
    uint32_t attack_frames;         /* A: 1 .. 4096 */
    uint32_t hold_frames;           /* H: 0 .. 16384 */
    int64_t release_step;           /* d: 1 .. OMX_DYNAMICS_MAX_STEP, in 2^-32 octave per frame */
} omx_program_dynamics_curve;       /* 3096 bytes */

typedef struct omx_program_dynamics_spec {
    double threshold_db;            /* compressor: finite, within [-240, 48] */
    double ratio;                   /* >= 1, finite or +infinity (a hard ceiling) */
    double knee_db;                 /* >= 0, finite: the width of the quadratic soft knee */
    double expander_threshold_db;   /* finite, within [-240, 48]; unused when expander_ratio == 1 */
    double expander_ratio;          /* >= 1, finite; 1: no expander */
    double range_db;                /* >= 0: the largest reduction of the expander (+infinity: unbounded) */
    double makeup_db;               /* finite */
} omx_program_dynamics_spec;        /* 56 bytes */

typedef struct omx_program_dynamics_point {
    double in_db, out_db;           /* finite */
} omx_program_dynamics_point;       /* 16 bytes */

typedef struct omx_program_dynamics_info {
    uint32_t level_tile;            /* frames one workgroup of the level pass takes */
    uint32_t hold_tile;             /* values one workgroup of the hold pass takes */
    uint32_t hold_max_window;       /* longest window one hold tile takes; a longer W is the minimum of shifted windows */
    uint32_t release_tile;          /* values one workgroup of the release scan takes: one carry per tile and stream */
    uint32_t smooth_tile;           /* frames one workgroup of the smooth-and-apply pass emits */
    uint32_t chain_threads;         /* threads of the workgroup that scans a stream's tile aggregates */
    uint32_t channels;
    uint32_t _pad;
} omx_program_dynamics_info;        /* 32 bytes */

typedef struct omx_program_dynamics_record {
    uint64_t frames_in;             /* N: frames taken since the reset */
    uint64_t frames_out;            /* E: frames emitted since the reset */
    uint64_t frames_written;        /* frames this call wrote to d_out[s] */
    uint64_t frames_reduced;        /* emitted frames with E[j] < 0, since the reset */
    uint64_t frames_boosted;        /* emitted frames with E[j] > 0, since the reset */
    uint64_t samples_over;          /* samples with |out| > 1.0f (NaN is not counted, infinity is), since the reset */
    uint64_t samples_nonfinite;     /* samples that are NaN or infinite, since the reset */
    int64_t min_gain;               /* the smallest E[j] emitted since the reset, in 2^-32 octave; 0 when none is below 0 */
    int64_t max_gain;               /* the largest E[j] emitted since the reset; 0 when none is above 0 */
    float min_gain_db;              /* (float)((double)min_gain * (U / 2^32)) */
    float max_gain_db;
    float out_sample_peak;          /* max |out|, fmaxf semantics (NaN ignored), since the reset */
    float out_sample_peak_db;       /* power_to_db(p * p, floor_db), as program_peaks.h */
    uint32_t state;                 /* OMX_DYNAMICS_IDLE / RUNNING / FLUSHED */
    uint32_t latency_frames;        /* LA of the stream */
    uint32_t curve_index;           /* the stream's curve, or OMX_DYNAMICS_BYPASS */
    uint32_t _pad;
} omx_program_dynamics_record;      /* 104 bytes */

/* ---- host only, no device needed */

/* The tiles of the passes at a channel count.  OMX_ERR_INVALID: channels outside 1 .. 8, a null info. */
int omx_program_dynamics_plan(uint32_t channels, omx_program_dynamics_info* info);
/* LOG and EXP as the library holds them: log_out[257], exp_out[257]; either may be null. */
int omx_program_dynamics_tables(int32_t* log_out, uint64_t* exp_out);
/* OMX_NONE for a curve the bank takes.  OMX_ERR_INVALID: a null curve, a |T[k]| above OMX_DYNAMICS_MAX_GAIN, a detector_mask of 0 or
 * with a bit at or above bit 8, attack_frames outside 1 .. 4096, hold_frames above 16384, release_step outside 1 ..
 * OMX_DYNAMICS_MAX_STEP. */
int omx_program_dynamics_check(const omx_program_dynamics_curve* curve);
/* *frames = attack_frames - 1 of a curve that check takes.  OMX_ERR_INVALID: what check refuses, a null frames. */
int omx_program_dynamics_latency(const omx_program_dynamics_curve* curve, uint32_t* frames);
/* Writes curve->T from a spec (DESIGN FORMULAS, design); the other fields of *curve are left as they are.  OMX_ERR_INVALID, with
 * nothing written: a null pointer, a threshold that is not finite or outside [-240, 48], ratio below 1 or NaN, knee_db negative or
 * not finite, expander_ratio below 1 or not finite, an expander_threshold_db (where expander_ratio != 1) not finite or outside
 * [-240, 48], range_db negative or NaN, makeup_db not finite. */
int omx_program_dynamics_design(const omx_program_dynamics_spec* spec, omx_program_dynamics_curve* curve);
/* Writes curve->T from n pairs (DESIGN FORMULAS, points).  OMX_ERR_INVALID, with nothing written: a null pointer, n 0 or above
 * OMX_DYNAMICS_MAX_POINTS, a value that is not finite, in_db not strictly increasing. */
int omx_program_dynamics_from_points(const omx_program_dynamics_point* points, uint32_t n, omx_program_dynamics_curve* curve);
/* The curve's gain in dB at a level in dB, evaluated as the kernel evaluates the table (DESIGN FORMULAS, gain_db).  OMX_ERR_INVALID:
 * a null pointer, a |T[k]| above OMX_DYNAMICS_MAX_GAIN, a level that is NaN. */
int omx_program_dynamics_gain_db(const omx_program_dynamics_curve* curve, double level_db, double* gain_db);
/* Times into frames and the release step (DESIGN FORMULAS, time); any result pointer may be null.  OMX_ERR_INVALID, with nothing
 * written: a sample rate that is not finite or not positive, attack_ms or hold_ms negative or not finite, an attack beyond 4096 frames,
 * a hold beyond 16384 frames, release_db_per_s not positive or NaN. */
int omx_program_dynamics_time(double sample_rate, double attack_ms, double hold_ms, double release_db_per_s, uint32_t* attack_frames,
                              uint32_t* hold_frames, int64_t* release_step);
/* *frames_out = E' - E of a stream with latency LA that has taken frames_in_before and emitted frames_out_before frames and now takes
 * `frames` more, with (flush != 0) or without a flush: the STREAMING formula, so that a host can size d_out.  OMX_ERR_INVALID, with
 * nothing written: a null frames_out, a latency above 4095, frames_in_before + frames beyond 2^63, frames_out_before above
 * frames_in_before. */
int omx_program_dynamics_frames(uint32_t latency_frames, uint64_t frames_in_before, uint64_t frames_out_before, uint64_t frames,
                                uint32_t flush, uint64_t* frames_out);

/* ---- the bank */

/* curves: host array [n_curves]; curve_of_stream: host array [n_streams] of table indices or OMX_DYNAMICS_BYPASS, NULL = curve 0 for
 * every stream.  Checks every curve as omx_program_dynamics_check does, uploads the tables, allocates the carried state and the
 * records and leaves every stream idle.  Allowed only while no stream of the stage holds frames: a new bank, or after dynamics_reset
 * of every stream.  Synchronises.
 * OMX_ERR_INVALID, with nothing changed: channels outside 1 .. 8, a null table, n_curves 0 or above OMX_DYNAMICS_MAX_CURVES, a curve
 * that check refuses, a detector_mask with a bit at or above `channels`, an index that is neither below n_curves nor
 * OMX_DYNAMICS_BYPASS, a stream that holds frames. */
int omx_program_loudness_bank_dynamics_configure(omx_program_loudness_bank* b, uint32_t channels, const omx_program_dynamics_curve* curves,
                                                 uint32_t n_curves, const uint32_t* curve_of_stream);
/* The flagged streams (host array [n_streams]; NULL: every stream) forget their frames and their history and are idle again.
 * OMX_ERR_INVALID before configure. */
int omx_program_loudness_bank_dynamics_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_in: device f32 [n_streams][frames_capacity][channels]; d_key: the side chain, same layout, capacity and frame counts, or NULL =
 * d_in; frames: host array [n_streams] or NULL = frames_capacity for every stream.  d_out: device f32 [n_streams][out_capacity]
 * [channels]; d_gain_db: device f32 [n_streams][out_capacity] or NULL; stream s gets its emitted frames at d_out[s][0 ..) and their
 * gains at d_gain_db[s][0 ..), nothing at or beyond frames_written[s] is written.  flush_mask: host array [n_streams] or NULL = no
 * stream.  Out of place only: d_out and d_gain_db may overlap neither each other nor d_in nor d_key.
 * OMX_ERR_INVALID: a call before configure; frames for a flushed stream; a stream that would emit more than out_capacity frames;
 * frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a null d_in when any stream brings frames, a null d_out when any stream
 * emits; an overlap; a null d_records.  OMX_ERR_UNSUPPORTED: a call that needs 2^31 workgroups or more in one launch.
 * A refused call changes nothing: neither d_out nor the trace nor the records nor the stage's state.
 * *d_records: device array [n_streams] of the running records, valid until dynamics_configure or destroy; work on `stream` that reads
 * it has to be ordered behind the call.  Returns OMX_PRODUCED when any stream emitted a frame, else OMX_NONE. */
int omx_program_loudness_bank_dynamics(omx_program_loudness_bank* b, const float* d_in, const float* d_key, uint64_t frames_capacity,
                                       const uint32_t* frames, float* d_out, float* d_gain_db, uint64_t out_capacity,
                                       const uint8_t* flush_mask, void* stream, const omx_program_dynamics_record** d_records);
/* Copy of one stream's record; synchronises.  OMX_ERR_INVALID: before configure, an index out of range, a null dst. */
int omx_program_loudness_bank_fetch_dynamics(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_dynamics_record* dst);

#ifdef __cplusplus
}
#endif
#endif

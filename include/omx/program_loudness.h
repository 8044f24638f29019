/* Programme loudness bank: the EBU R 128 programme figures for S independent streams —
 * integrated loudness with the two gates of ITU-R BS.1770-4, loudness range (EBU Tech 3342) and the
 * maxima of momentary loudness, short-term loudness and true peak.
 *
 * A bank of its own next to omx_loudness_bank (which meters one snapshot per block): it takes PCM in
 * device memory, keeps per-stream state between calls and hands out one record per stream.
 *
 * DEFINITIONS ("Programme loudness bank")
 *   y        = k_weighted(x): f64 transposed direct form II with omx_k_weighting_coefficients(sanitised rate),
 *              rounded to f32; per-sample energy double(y) * double(y), 0 for a non-finite one.
 *   segment  = (uint(fs) + 5) / 10 frames (100 ms);  e[j] = sum over channels of weight * mean energy of the
 *              channel over segment j (weights: 1.0; 1.41 rear / side; 0 LFE, of the call the sample arrived in).
 *   gating block j >= 3  = mean of e[j-3 .. j];  short-term block j >= 29 = mean of e[j-29 .. j].
 *   L(z) = -0.691 + 10 log10(z).  Gates compare energies: absolute z > 10^((-70 + 0.691) / 10); relative
 *   z > 0.1 * (mean of the blocks above the absolute gate) for integrated loudness, 0.01 * for the range.
 *   integrated = L(mean of the gating blocks above both gates); range = L(hi) - L(lo) over the sorted short-term
 *   blocks above both gates, lo = element floor((n-1) * 0.10 + 0.5), hi = element floor((n-1) * 0.95 + 0.5).
 *   No block passes: integrated = the configured floor, range = 0.
 *
 * All work is enqueued on the caller's stream; only the fetch functions synchronise.  No CPU fallback:
 * create returns OMX_ERR_NO_DEVICE without a gfx950 device. */
#ifndef OMX_PROGRAM_LOUDNESS_H
#define OMX_PROGRAM_LOUDNESS_H

#include "../omx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omx_program_loudness_bank omx_program_loudness_bank;

/* One record per stream.  The dB fields follow mean_square_to_lufs: floored at the configured floor_db, f32;
 * the f64 energies are what they were made from (0 where there is no block yet). */
typedef struct omx_program_loudness_record {
    double integrated_energy;         /* mean of the gating blocks above both gates */
    double relative_threshold_energy; /* 0.1 * mean of the gating blocks above the absolute gate */
    double lra_low_energy;            /* the 10 % and 95 % short-term blocks (nearest rank) */
    double lra_high_energy;
    double momentary_energy;          /* latest gating block / short-term block (grid values) */
    double short_term_energy;
    double max_momentary_energy;      /* largest gating block / short-term block seen (not gated) */
    double max_short_term_energy;
    uint64_t frames;                  /* frames taken since the last reset (stops when the stream is full) */
    uint64_t segments;                /* completed 100 ms segments stored */
    uint64_t gating_blocks;           /* max(segments - 3, 0) */
    uint64_t gating_above_absolute;
    uint64_t gating_above_relative;   /* above both gates */
    uint64_t short_term_blocks;       /* max(segments - 29, 0) */
    uint64_t short_term_above_absolute;
    uint64_t short_term_above_relative;
    float integrated_lufs;
    float relative_threshold_lufs;
    float loudness_range_lu;
    float momentary_lufs;
    float short_term_lufs;
    float max_momentary_lufs;
    float max_short_term_lufs;
    float max_true_peak_db;           /* running maximum folded in by omx_program_loudness_bank_note_snapshots */
    uint32_t overflow;                /* 1: the segment storage is full, the stream takes no more samples */
    uint32_t _pad;
} omx_program_loudness_record;

/* capacity_seconds: segment storage per stream, fixed at creation (10 f64 per second: 24 h = 6.9 MB per stream).
 * `channels` is the expected channel count (storage is sized for OMX_MAX_CHANNELS; each call names its own).
 * cfg->sample_rate is the rate the first call is expected at; cfg->floor_db floors every dB field. */
int omx_program_loudness_bank_create(const omx_loudness_config* cfg, uint32_t n_streams, uint32_t channels,
                                     uint32_t capacity_seconds, omx_program_loudness_bank** out);
void omx_program_loudness_bank_destroy(omx_program_loudness_bank* b);
/* R 128 start / reset.  reset_mask: host array [n_streams], non-zero = reset that stream; NULL = every stream. */
int omx_program_loudness_bank_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_pcm: device f32 [n_streams][frames_capacity][channels].  frames: host array [n_streams] of per-stream frame counts
 * (<= frames_capacity, 0 allowed), NULL = frames_capacity for every stream.  reset_mask: host array or NULL; flagged streams are
 * reset before their samples are taken.  A rate or channel count other than the one the running programmes started with is refused
 * with OMX_ERR_INVALID unless every stream that has taken samples is reset in the same call.
 * channels is the stride of d_pcm and must be 1 .. OMX_MAX_CHANNELS: anything else is OMX_ERR_INVALID (no clamping).
 * Rates (after sanitising: at most 768 kHz) below 3364 Hz: OMX_ERR_UNSUPPORTED.  The K-weighting shelf sits at 1681.97 Hz, and up to
 * twice that the filter has poles outside the unit circle; 3364 Hz is the first whole rate from which every rate is stable.
 * Also OMX_ERR_INVALID: frames[s] > frames_capacity, frames_capacity > 2^32 - 1, a null d_pcm when any stream brings frames.
 * A refused call changes nothing.  Returns OMX_PRODUCED when any stream took a frame, else OMX_NONE. */
int omx_program_loudness_bank_process(omx_program_loudness_bank* b, const float* d_pcm, uint64_t frames_capacity,
                                      const uint32_t* frames, const uint8_t* reset_mask, uint32_t channels, float sample_rate,
                                      const uint8_t positions[OMX_MAX_CHANNELS], void* stream);
/* Folds the true_peak_db fields (channels below channel_count) of the snapshots an omx_loudness_bank call left on the device —
 * d_snapshots [n_streams][n_blocks]; d_n_blocks: device array of per-stream block counts (a ragged call's d_n_blocks) or NULL =
 * n_blocks for every stream — into the per-stream running maximum. */
int omx_program_loudness_bank_note_snapshots(omx_program_loudness_bank* b, const omx_loudness_snapshot* d_snapshots,
                                             uint64_t n_blocks, const uint32_t* d_n_blocks, void* stream);
/* Runs the result pass on `stream`; *d_records: device array [n_streams], valid until the next call on the bank. */
int omx_program_loudness_bank_results(omx_program_loudness_bank* b, void* stream, const omx_program_loudness_record** d_records);
/* Result pass (when something changed since the last one), copy, synchronise. */
int omx_program_loudness_bank_fetch(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_loudness_record* dst);
/* Stored segment energies e[first .. first + count) of one stream (first + count <= segments). */
int omx_program_loudness_bank_fetch_segments(omx_program_loudness_bank* b, uint64_t stream_index, uint64_t first, uint64_t count,
                                             double* dst);
/* OMX_OPT_KERNEL_FORM: 0 = by call shape (default), 1 = reference-order segment pass (bit-identical segment energies however the
 * programme is cut into calls), 2 = time-parallel segment pass.  Other options / values: OMX_ERR_INVALID.
 * The time-parallel pass holds 1e-4 dB against the reference order up to 384 kHz.  Above that rate the bank runs the reference-order
 * pass whatever form is set, 2 included, and omx_debug_program_loudness_bank_last_form reports 1: it never returns looser numbers. */
int omx_program_loudness_bank_set_option(omx_program_loudness_bank* b, uint32_t option, uint64_t value);
/* 1 = the last process call ran the reference-order pass, 2 = the time-parallel one, 0 = none yet */
int omx_debug_program_loudness_bank_last_form(const omx_program_loudness_bank* b);

#ifdef __cplusplus
}
#endif
#endif

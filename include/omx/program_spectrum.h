/* Programme loudness bank, long-term spectrum: what does a programme look like in the frequency domain?  A delivery check asks whether
 * a "48 kHz" file holds anything above 16 kHz, whether there is mains hum at 50 or 60 Hz and its harmonics, what the octave and
 * third-octave levels of a stem are; filter and convolve change a spectrum and nothing in the bank measured one.  This stage keeps,
 * per stream and channel, the long-term average power spectrum (Welch's method on a fixed frame grid, periodic Hann, half overlap),
 * measured on the device, and the host-only functions below turn it into what a person reads: density, fractional-octave band
 * levels, a QC summary and a match-EQ FIR for convolve.
 *
 * Additive: this header adds six structures, fourteen functions and a few constants; nothing declared in the headers it includes
 * changes and OMX_ABI_VERSION stays as it is.  A bank that never calls spectrum_configure allocates and launches nothing more.  All
 * work goes on the caller's stream; only fetch_spectrum synchronises (and spectrum_configure).  No call of this header touches the
 * state or the records of the earlier headers.
 *
 * DEFINITION ("Spectrum"; tests/program_spectrum_ref.py restates it).
 *   Rule     N = fft_size is 2048, 4096 or 8192 (default 4096), the hop is H = N / 2, the window is the periodic Hann
 *            w[n] = (float)(0.5 - 0.5 cos(2 pi n / N)), made in C double and rounded once (omx_program_spectrum_window gives the table).
 *   Grid     x[n][c] is the f32 PCM a stream took since its reset.  Transform k covers the frames [k H, k H + N) and is taken as soon
 *            as the stream holds frame k H + N - 1.  A stream flagged in finish_mask completes every transform with k H < frames that
 *            is still open with zeros behind its last frame and then takes no frames until spectrum_reset.
 *   One      for channel c: y[n] = w[n] * x[k H + n][c] in f32, Y = the N-point real transform of y in f32, p_k[c][b] = re^2 + im^2 in
 *            f32 for b = 0 .. N/2.  Every transform is of ONE channel's ONE frame (an N/2-point complex transform of (y[2m], y[2m+1])
 *            and an untangling pass): nothing of another channel or another frame rides in it.  A transform of a channel whose N
 *            samples hold a NaN or an infinity is left out of that channel's sums and counted in skipped[c]; every other one is
 *            counted in transforms[c].
 *   Sums     S[c][b] in f64.  The transforms of a stream fall into runs of OMX_SPECTRUM_RUN consecutive indices, run j = [R j, R j + R).
 *            A run's sum is the chain ((0 + p_k0) + p_k1) + ... over its transforms that are not skipped, in ascending k, every p
 *            converted to f64 first; S is the chain ((0 + run_0) + run_1) + ... over the runs in ascending j, the last run with as many
 *            transforms as the stream has taken.  The grouping is part of the definition: a call that ends inside a run keeps the
 *            run's partial chain and the next call continues it, so S has the same bytes however the programme is cut into calls.
 *   Limit    a stream takes at most 2^32 - 1 frames between resets.
 *
 * HOST ONLY (C double, no device; each refuses bad arguments with its outputs untouched).  df = sample_rate / N, K = N/2 + 1 bins.
 *   transforms  frames >= N ? (frames - N) / H + 1 : 0 while not finished; ceil(frames / H) when finished
 *   density     D[b] = (g S[b]) / (((double)transforms * N) * W2), g = 1 at b = 0 and N/2, else 2; W2 = sum of (double)w[n]^2 in
 *               ascending n.  The one-sided mean square per bin: by Parseval the sum over b is the mean square of the windowed
 *               signal over W2 / N.  With transforms == 0 every entry is 0.
 *   bands       the base-ten bands of IEC 61260-1: centre = 1000 * pow(10, 0.3 x / fraction) for integer x, edges centre *
 *               pow(10, -+0.15 / fraction).  Bin b owns [max(0, (b - 1/2) df), min(fs/2, (b + 1/2) df)] and gives a band the share
 *               of that interval inside the band's edges; power = the sum of D[b] * share in ascending b over all bins.  Listed, in
 *               ascending x: the bands with lower edge >= 4 df and upper edge <= fs/2.  level = max(10 log10(2 power), floor), the
 *               floor itself when power is 0: a full-scale sine reads 0 dB.
 *   summarize   total = sum of D in ascending b, total_db its level as above.  Peak: the first largest bin pk; with 0 < pk < N/2 and
 *               its neighbours positive, a = 10 log10 D[pk-1], m = 10 log10 D[pk], c = 10 log10 D[pk+1], q = a - 2 m + c, d = q < 0 ?
 *               0.5 (a - c) / q : 0, clamped to [-1/2, 1/2], else d = 0; peak_hz = (pk + d) df, peak_db = max(10 log10(2 D[pk]) -
 *               0.25 (a - c) d, floor).  occupied_hz: with c_b the running sum of D, the first b with c_b >= occupied_fraction *
 *               total gives min((b + 1/2) df, fs/2); 0 when total is 0.  For probe frequency f (0 < f < fs/2): bc = floor(f / df +
 *               1/2), strongest = the largest D of bc - 1 .. bc + 1 inside 0 .. N/2; med = the median of D[b] over the bins 1 <= b <=
 *               N/2 with |b - bc| > 2 (outside the window's main lobe) and either f pow(10, -0.1) <= b df <= f pow(10, 0.1) or |b -
 *               bc| <= 6 (at hum frequencies a third octave is a bin or two), the mean of the middle two for an even count;
 *               prominence_db = dB(strongest) - dB(med), dB(v) = v > 0 ? max(10 log10 v, floor) : floor; 0 where no such bin
 *               exists or f >= fs/2.
 *               OMX_SPECTRUM_BANDLIMITED: total > 0 and occupied_hz < bandwidth_min_ratio * fs/2.  OMX_SPECTRUM_TONE: a prominence
 *               above tone_db.
 *   match       a linear-phase FIR of n_taps taps for convolve that brings the source's tonal balance to the target's.  Smoothing: with
 *               P the running sum of D, Ds[0] = D[0] and for b >= 1 Ds[b] = (P[hi + 1] - P[lo]) / (hi - lo + 1), lo = max(1, ceil(b
 *               pow(10, -0.05))), hi = min(N/2, floor(b pow(10, 0.05))): a boxcar of one third octave in log frequency.
 *               gain_db[b] = dB(Dt_s[b]) - dB(Ds_s[b]), clamped to [-max_cut_db, max_boost_db]: the filter's gain in dB.  D is a
 *               power, so the difference of two dB(D) is already 20 log10 of the amplitude ratio the filter has to apply.  Below
 *               b_lo = max(1, ceil(low_hz / df)) the gain is held at gain_db[b_lo], above b_hi = min(N/2, floor(high_hz / df)) at
 *               gain_db[b_hi].  A[b] = pow(10, gain_db[b] / 20), the square root of the power ratio.
 *               With M = (n_taps - 1) / 2 and C[i] = cos(2 pi i / N): h[m] = (A[0] + 2 sum_{b=1}^{N/2-1} A[b] C[(b m) mod N] +
 *               A[N/2] C[((N/2) m) mod N]) / N, the sum in ascending b; taps[M + m] = taps[M - m] = (float)(h[m] (0.5 + 0.5 cos(pi m
 *               / (M + 1)))) for m = 0 .. M: the halves mirror on bits. */
#ifndef OMX_PROGRAM_SPECTRUM_H
#define OMX_PROGRAM_SPECTRUM_H

#include "program_convolve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMX_SPECTRUM_DEFAULT_FFT_SIZE 4096u
#define OMX_SPECTRUM_MIN_FFT_SIZE 2048u
#define OMX_SPECTRUM_MAX_FFT_SIZE 8192u
#define OMX_SPECTRUM_RUN 16u                  /* R: transforms of one run of the sums' inner chain */
#define OMX_SPECTRUM_MAX_BANDS 48u            /* no rule lists more bands than this */
#define OMX_SPECTRUM_MAX_PROBES 8u
#define OMX_SPECTRUM_MAX_TAPS 4095u           /* of a match FIR; odd, and below fft_size */
#define OMX_SPECTRUM_DB_FLOOR -400.0          /* as OMX_INSPECT_DB_FLOOR */
#define OMX_SPECTRUM_DEFAULT_OCCUPIED_FRACTION 0.9999
#define OMX_SPECTRUM_DEFAULT_BANDWIDTH_MIN_RATIO 0.8
#define OMX_SPECTRUM_DEFAULT_TONE_DB 20.0
#define OMX_SPECTRUM_DEFAULT_MAX_BOOST_DB 12.0
#define OMX_SPECTRUM_DEFAULT_MAX_CUT_DB 12.0
#define OMX_SPECTRUM_DEFAULT_LOW_HZ 40.0
#define OMX_SPECTRUM_DEFAULT_HIGH_RATIO 0.45  /* high_hz = 0.45 * sample_rate */
/* omx_program_spectrum_summary.verdict */
#define OMX_SPECTRUM_BANDLIMITED 1u
#define OMX_SPECTRUM_TONE 2u

typedef struct omx_program_spectrum_rule {
    uint32_t fft_size;              /* 2048, 4096 or 8192 */
    uint32_t flags;                 /* must be 0 */
} omx_program_spectrum_rule;        /* 8 bytes */

typedef struct omx_program_spectrum_info {
    uint32_t fft_size;
    uint32_t hop;                   /* fft_size / 2 */
    uint32_t bins;                  /* fft_size / 2 + 1 */
    uint32_t threads;               /* threads per workgroup of the transform kernel */
    uint32_t transforms_per_workgroup;  /* transforms a workgroup runs side by side: 4, 2 or 1 */
    uint32_t run;                   /* OMX_SPECTRUM_RUN */
    uint32_t lds_bytes;             /* of one workgroup of the transform kernel */
    uint32_t channels;
    uint64_t scratch_bytes;         /* an upper bound of the run rows a call of `frames` frames per stream needs */
    uint64_t state_bytes;           /* sums, run state and carried frames of the whole bank */
} omx_program_spectrum_info;        /* 48 bytes */

typedef struct omx_program_spectrum_record {
    uint64_t frames;                /* taken since the reset */
    uint64_t transforms[OMX_MAX_CHANNELS];  /* in the channel's sums; entries at and beyond `channels` are zero */
    uint64_t skipped[OMX_MAX_CHANNELS];     /* left out: a NaN or an infinity among the N samples */
    uint32_t fft_size;
    uint32_t channels;
    uint32_t finished;
    uint32_t _pad;
} omx_program_spectrum_record;      /* 152 bytes */

typedef struct omx_program_spectrum_qc {
    double occupied_fraction;       /* in (0, 1] */
    double bandwidth_min_ratio;     /* in [0, 1] */
    double tone_db;                 /* finite, >= 0 */
    double probe_hz[OMX_SPECTRUM_MAX_PROBES];  /* the first n_probes: finite, > 0 */
    uint32_t n_probes;              /* 0 .. 8 */
    uint32_t flags;                 /* must be 0 */
} omx_program_spectrum_qc;          /* 96 bytes */

typedef struct omx_program_spectrum_summary {
    uint32_t verdict;               /* OMX_SPECTRUM_* bits */
    uint32_t n_probes;
    double total_db;
    double peak_hz;
    double peak_db;
    double occupied_hz;
    double prominence_db[OMX_SPECTRUM_MAX_PROBES];  /* entries at and beyond n_probes are zero */
} omx_program_spectrum_summary;     /* 104 bytes */

typedef struct omx_program_spectrum_match_spec {
    double max_boost_db;            /* finite, >= 0 */
    double max_cut_db;              /* finite, >= 0 */
    double low_hz;                  /* finite, >= 0 */
    double high_hz;                 /* finite, > low_hz, <= sample_rate / 2, with a bin in [low_hz, high_hz] */
    uint32_t flags;                 /* must be 0 */
    uint32_t _pad;
} omx_program_spectrum_match_spec;  /* 40 bytes */

/* Host only, need no device: the header's defaults.  OMX_ERR_INVALID: a null pointer; match_spec_default: a sample rate that is not
 * finite or not above 200 Hz. */
int omx_program_spectrum_rule_default(omx_program_spectrum_rule* rule);
int omx_program_spectrum_qc_default(omx_program_spectrum_qc* qc);
int omx_program_spectrum_match_spec_default(double sample_rate, omx_program_spectrum_match_spec* spec);
/* Host only: the transform kernel's tile and the memory of a bank of n_streams streams whose calls bring up to `frames` frames per
 * stream.  OMX_ERR_INVALID, with nothing written: a bad rule, channels outside 1 .. 8, frames beyond 2^32 - 1, a null pointer. */
int omx_program_spectrum_plan(const omx_program_spectrum_rule* rule, uint32_t channels, uint64_t n_streams, uint64_t frames,
                              omx_program_spectrum_info* info);
/* Host only: the window, fft_size floats.  OMX_ERR_INVALID: a size that is not 2048, 4096 or 8192, a null pointer. */
int omx_program_spectrum_window(uint32_t fft_size, float* window);
/* Host only: the transforms a stream of `frames` frames has taken.  OMX_ERR_INVALID: a bad size, frames beyond 2^32 - 1, a null count. */
int omx_program_spectrum_transforms(uint64_t frames, uint32_t finished, uint32_t fft_size, uint64_t* count);
/* Host only: DEFINITION, density; sums is one channel-major array [record->channels][fft_size / 2 + 1] as fetch_spectrum gives it,
 * D takes fft_size / 2 + 1 doubles.  OMX_ERR_INVALID, with nothing written: a null pointer, a record whose fft_size or channels is
 * out of range, channel at or above record->channels. */
int omx_program_spectrum_density(const omx_program_spectrum_record* record, const double* sums, uint32_t channel, double* density);
/* Host only: DEFINITION, bands.  On entry *n is the capacity of centre_hz and level_db, on return the number of bands written.
 * OMX_ERR_INVALID, with nothing written: a null pointer, a bad size, a sample rate that is not finite or not above 200 Hz, a fraction
 * other than 1 or 3, a density entry that is negative or not finite, a capacity below the number of bands. */
int omx_program_spectrum_bands(const double* density, uint32_t fft_size, double sample_rate, uint32_t fraction, double* centre_hz,
                               double* level_db, uint32_t* n);
/* Host only: DEFINITION, summarize.  OMX_ERR_INVALID, with nothing written: a null pointer, a bad qc rule (the ranges above), a bad
 * size or sample rate, a density entry that is negative or not finite. */
int omx_program_spectrum_summarize(const omx_program_spectrum_qc* qc, const double* density, uint32_t fft_size, double sample_rate,
                                   omx_program_spectrum_summary* summary);
/* Host only: DEFINITION, match; the taps suit omx_program_convolve_check.  OMX_ERR_INVALID, with nothing written: a null pointer, a
 * bad size, sample rate or spec, a density entry that is negative or not finite, n_taps even, 0, above OMX_SPECTRUM_MAX_TAPS or not
 * below fft_size. */
int omx_program_spectrum_match(const double* density_source, const double* density_target, uint32_t fft_size, double sample_rate,
                               const omx_program_spectrum_match_spec* spec, float* taps, uint32_t n_taps);

/* Sets the rule and the channel count of the PCM, allocates the records, the sums and the carried frames and resets every stream.
 * Allowed only while no stream of the stage holds frames: a new bank, or after spectrum_reset of every stream.  The device pointers
 * of an earlier call are invalid afterwards.
 * OMX_ERR_INVALID, with nothing changed: a bad rule (a null rule, a flag set, a size that is not 2048, 4096 or 8192: 16384 points and
 * more need the 512- and 1024-thread transforms and come next), channels outside 1 .. 8, a stream that holds frames. */
int omx_program_loudness_bank_spectrum_configure(omx_program_loudness_bank* b, const omx_program_spectrum_rule* rule, uint32_t channels);
/* The flagged streams start over with a zero record, zero sums and no carried frames (reset_mask: host array [n_streams], NULL = every
 * stream).  OMX_ERR_INVALID: before configure. */
int omx_program_loudness_bank_spectrum_reset(omx_program_loudness_bank* b, const uint8_t* reset_mask);
/* d_in: device f32 [n_streams][frames_capacity][channels]; the call reads it and writes nothing into it.  frames: host array
 * [n_streams] or NULL = frames_capacity for every stream.  finish_mask: host array [n_streams] or NULL = no stream finishes.
 * OMX_ERR_INVALID: a call before configure; frames[s] > frames_capacity; a capacity beyond 2^32 - 1; a stream that would hold more
 * than 2^32 - 1 frames since its reset; frames for a stream that is finished; a null d_in when any stream brings frames; a null
 * d_records or d_sums.  A refused call changes nothing.
 * *d_records: device array [n_streams] of the running records; *d_sums: device f64 [n_streams][channels][fft_size / 2 + 1], S above.
 * Both are valid until spectrum_configure or destroy; work on `stream` that reads them has to be ordered behind the call.  Returns
 * OMX_PRODUCED when any stream brought a frame or was finished by this call, else OMX_NONE. */
int omx_program_loudness_bank_spectrum(omx_program_loudness_bank* b, const float* d_in, uint64_t frames_capacity, const uint32_t* frames,
                                       const uint8_t* finish_mask, void* stream, const omx_program_spectrum_record** d_records,
                                       const double** d_sums);
/* Copy of one stream's running record and of its sums ([channels][fft_size / 2 + 1] doubles); synchronises.  OMX_ERR_INVALID: before
 * configure, an index out of range, a null record or sums. */
int omx_program_loudness_bank_fetch_spectrum(omx_program_loudness_bank* b, uint64_t stream_index, omx_program_spectrum_record* record,
                                             double* sums);

#ifdef __cplusplus
}
#endif
#endif

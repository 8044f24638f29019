/* Plain C99 host of the programme bank's sample-rate conversion (include/omx/program_resample.h): one stereo S16 programme of two
 * seconds at 44.1 kHz (noise at a quarter of full scale from a 32-bit LCG, three times as loud for 50 ms twice a second) goes through
 * the whole chain on the device: import, the conversion to 48 kHz (in two calls, the second one flushing), process at 48 kHz,
 * plan_gains to -10 LUFS, apply_limited under -1 dBTP, export as S24 with TPDF dither.  Prints the records and a checksum of the
 * exported bytes.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_resample.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, FS_IN = 44100, FS_OUT = 48000, FRAMES_IN = 88200, FRAMES_OUT = 96000, FIRST = 50000, N_IN = FRAMES_IN * CH, N_OUT = FRAMES_OUT * CH };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 60, &bank));
    uint8_t positions[OMX_MAX_CHANNELS];
    omx_positions_fallback(CH, positions);

    omx_program_resample_rule rule;
    memset(&rule, 0, sizeof rule);
    rule.rate_in = FS_IN;
    rule.rate_out = FS_OUT;
    rule.half_width = OMX_RESAMPLE_DEFAULT_HALF_WIDTH;
    rule.beta = OMX_RESAMPLE_DEFAULT_BETA;
    rule.cutoff = OMX_RESAMPLE_DEFAULT_CUTOFF;
    omx_program_resample_info info;
    CHECK(omx_program_resample_plan(&rule, &info));
    uint64_t first_out = 0, second_out = 0;
    CHECK(omx_program_resample_frames(&rule, 0, 0, FIRST, 0, &first_out));
    CHECK(omx_program_resample_frames(&rule, FIRST, first_out, FRAMES_IN - FIRST, 1, &second_out));
    if (first_out + second_out != FRAMES_OUT) return 1;

    int16_t* host = (int16_t*)malloc(sizeof(int16_t) * N_IN);
    unsigned char* exported = (unsigned char*)malloc((size_t)3 * N_OUT);
    void *d_pcm = NULL, *d_f32 = NULL, *d_48k = NULL, *d_limited = NULL, *d_out = NULL;
    if (!host || !exported || hipMalloc(&d_pcm, sizeof(int16_t) * N_IN) != 0 || hipMalloc(&d_f32, sizeof(float) * N_IN) != 0 ||
        hipMalloc(&d_48k, sizeof(float) * N_OUT) != 0 || hipMalloc(&d_limited, sizeof(float) * N_OUT) != 0 || hipMalloc(&d_out, (size_t)3 * N_OUT) != 0)
        return 1;
    uint32_t state = 12345u;
    for (long i = 0; i < N_IN; ++i) {
        state = state * 1664525u + 1013904223u;
        const int v = (int)((state >> 16) & 0x3FFFu) - 8192;
        host[i] = (int16_t)(((i / CH) % 22050 < 2205) ? 3 * v : v);
    }
    if (hipMemcpy(d_pcm, host, sizeof(int16_t) * N_IN, 1) != 0) return 1;

    CHECK(omx_program_loudness_bank_import_pcm(bank, d_pcm, OMX_PCM_S16, (float*)d_f32, FRAMES_IN, NULL, CH, NULL));
    CHECK(omx_program_loudness_bank_resampler_configure(bank, &rule, CH));
    const omx_program_resample_record* d_resample_records = NULL;
    uint32_t frames = FIRST;
    CHECK(omx_program_loudness_bank_resample(bank, (const float*)d_f32, FRAMES_IN, &frames, (float*)d_48k, FRAMES_OUT, NULL, NULL,
                                             &d_resample_records));
    frames = FRAMES_IN - FIRST;
    const uint8_t flush = 1;
    CHECK(omx_program_loudness_bank_resample(bank, (const float*)d_f32 + (size_t)FIRST * CH, FRAMES_IN - FIRST, &frames,
                                             (float*)d_48k + first_out * CH, FRAMES_OUT - first_out, &flush, NULL, &d_resample_records));
    CHECK(omx_program_loudness_bank_process(bank, (const float*)d_48k, FRAMES_OUT, NULL, NULL, CH, (float)FS_OUT, positions, NULL));
    omx_program_gain_rule gain_rule;
    memset(&gain_rule, 0, sizeof gain_rule);
    gain_rule.target_lufs = -10.0f;
    gain_rule.true_peak_ceiling_db = -1.0f;
    gain_rule.min_gain_db = -60.0f;
    gain_rule.max_gain_db = 60.0f;
    const omx_program_gain_record* d_gains = NULL;
    CHECK(omx_program_loudness_bank_plan_gains(bank, &gain_rule, NULL, &d_gains));
    omx_program_limit_rule limit_rule;
    limit_rule.ceiling_db = -1.0f;
    limit_rule.attack_frames = 64;
    limit_rule.release_hold_frames = 0;
    limit_rule.flags = 0;
    CHECK(omx_program_loudness_bank_limiter_configure(bank, &limit_rule, CH, (float)FS_OUT));
    const omx_program_limit_record* d_limit_records = NULL;
    CHECK(omx_program_loudness_bank_apply_limited(bank, (const float*)d_48k, FRAMES_OUT, NULL, (float*)d_limited, FRAMES_OUT, &flush, d_gains, 1,
                                                  NULL, NULL, &d_limit_records));
    omx_program_export_rule export_rule;
    memset(&export_rule, 0, sizeof export_rule);
    export_rule.format = OMX_PCM_S24;
    export_rule.dither = OMX_DITHER_TPDF;
    export_rule.seed = 2024;
    CHECK(omx_program_loudness_bank_export_configure(bank, &export_rule, CH));
    const omx_program_export_record* d_export_records = NULL;
    CHECK(omx_program_loudness_bank_export_pcm(bank, (const float*)d_limited, d_out, FRAMES_OUT, NULL, NULL, &d_export_records));

    omx_program_resample_record s;
    omx_program_loudness_record r;
    omx_program_gain_record g;
    omx_program_limit_record l;
    omx_program_export_record e;
    CHECK(omx_program_loudness_bank_fetch_resampled(bank, 0, &s));
    CHECK(omx_program_loudness_bank_fetch(bank, 0, &r));
    CHECK(omx_program_loudness_bank_fetch_gains(bank, 0, 1, &g));
    CHECK(omx_program_loudness_bank_fetch_limited(bank, 0, &l));
    CHECK(omx_program_loudness_bank_fetch_exported(bank, 0, &e));
    if (hipMemcpy(exported, d_out, (size_t)3 * N_OUT, 2) != 0) return 1;
    uint64_t checksum = 1469598103934665603ull; /* FNV-1a over the exported bytes */
    for (size_t i = 0; i < (size_t)3 * N_OUT; ++i) checksum = (checksum ^ exported[i]) * 1099511628211ull;
    printf("L %u M %u taps %u latency %u resampled_in %lu resampled_out %lu resampled_written %lu resampled_over %lu resampled_peak %.6f state %u "
           "integrated_lufs %.4f gain_db %.4f frames_limited %lu min_envelope %.6f frames_out %lu samples_clipped %lu out_peak %u format %u "
           "checksum %lu\n",
           info.L, info.M, info.taps, info.latency_frames, (unsigned long)s.frames_in, (unsigned long)s.frames_out, (unsigned long)s.frames_written,
           (unsigned long)s.samples_over, (double)s.out_sample_peak, s.state, (double)r.integrated_lufs, (double)g.gain_db,
           (unsigned long)l.frames_limited, (double)l.min_envelope, (unsigned long)e.frames_out, (unsigned long)e.samples_clipped, e.out_peak,
           e.format, (unsigned long)checksum);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    hipFree(d_f32);
    hipFree(d_48k);
    hipFree(d_limited);
    hipFree(d_out);
    free(host);
    free(exported);
    return 0;
}

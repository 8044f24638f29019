/* Plain C99 host of the programme bank's PCM formats (include/omx/program_pcm.h): one stereo S16 programme of two seconds (noise at a
 * quarter of full scale from a 32-bit LCG, three times as loud for 50 ms twice a second) goes through the whole chain on the device:
 * import, process, plan_gains to -10 LUFS, apply_limited under -1 dBTP, export as S16 with TPDF dither.  Prints the records and a
 * checksum of the exported bytes.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_pcm.h"

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

enum { CH = 2, FS = 48000, FRAMES = 96000, N = FRAMES * CH };

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

    int16_t* host = (int16_t*)malloc(sizeof(int16_t) * N);
    void *d_pcm = NULL, *d_f32 = NULL, *d_limited = NULL, *d_out = NULL;
    if (!host || hipMalloc(&d_pcm, sizeof(int16_t) * N) != 0 || hipMalloc(&d_f32, sizeof(float) * N) != 0 ||
        hipMalloc(&d_limited, sizeof(float) * N) != 0 || hipMalloc(&d_out, sizeof(int16_t) * N) != 0)
        return 1;
    uint32_t state = 12345u;
    for (long i = 0; i < N; ++i) {
        state = state * 1664525u + 1013904223u;
        const int v = (int)((state >> 16) & 0x3FFFu) - 8192;
        host[i] = (int16_t)(((i / CH) % 24000 < 2400) ? 3 * v : v);
    }
    if (hipMemcpy(d_pcm, host, sizeof(int16_t) * N, 1) != 0) return 1;

    CHECK(omx_program_loudness_bank_import_pcm(bank, d_pcm, OMX_PCM_S16, (float*)d_f32, FRAMES, NULL, CH, NULL));
    CHECK(omx_program_loudness_bank_process(bank, (const float*)d_f32, FRAMES, NULL, NULL, CH, (float)FS, positions, NULL));
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
    CHECK(omx_program_loudness_bank_limiter_configure(bank, &limit_rule, CH, (float)FS));
    const uint8_t flush = 1;
    const omx_program_limit_record* d_limit_records = NULL;
    CHECK(omx_program_loudness_bank_apply_limited(bank, (const float*)d_f32, FRAMES, NULL, (float*)d_limited, FRAMES, &flush, d_gains, 1, NULL,
                                                  NULL, &d_limit_records));
    omx_program_export_rule export_rule;
    memset(&export_rule, 0, sizeof export_rule);
    export_rule.format = OMX_PCM_S16;
    export_rule.dither = OMX_DITHER_TPDF;
    export_rule.seed = 2024;
    CHECK(omx_program_loudness_bank_export_configure(bank, &export_rule, CH));
    const omx_program_export_record* d_export_records = NULL;
    CHECK(omx_program_loudness_bank_export_pcm(bank, (const float*)d_limited, d_out, FRAMES, NULL, NULL, &d_export_records));

    omx_program_loudness_record r;
    omx_program_gain_record g;
    omx_program_limit_record l;
    omx_program_export_record e;
    CHECK(omx_program_loudness_bank_fetch(bank, 0, &r));
    CHECK(omx_program_loudness_bank_fetch_gains(bank, 0, 1, &g));
    CHECK(omx_program_loudness_bank_fetch_limited(bank, 0, &l));
    CHECK(omx_program_loudness_bank_fetch_exported(bank, 0, &e));
    if (hipMemcpy(host, d_out, sizeof(int16_t) * N, 2) != 0) return 1;
    uint64_t checksum = 1469598103934665603ull; /* FNV-1a over the exported bytes */
    const unsigned char* bytes = (const unsigned char*)host;
    for (size_t i = 0; i < sizeof(int16_t) * N; ++i) checksum = (checksum ^ bytes[i]) * 1099511628211ull;
    printf("integrated_lufs %.4f gain_db %.4f frames_limited %lu min_envelope %.6f limiter_peak %.6f frames_out %lu frames_written %lu "
           "samples_clipped %lu samples_nan %lu out_peak %u out_peak_db %.4f format %u dither %u checksum %lu\n",
           (double)r.integrated_lufs, (double)g.gain_db, (unsigned long)l.frames_limited, (double)l.min_envelope, (double)l.out_sample_peak,
           (unsigned long)e.frames_out, (unsigned long)e.frames_written, (unsigned long)e.samples_clipped, (unsigned long)e.samples_nan,
           e.out_peak, (double)e.out_peak_db, e.format, e.dither, (unsigned long)checksum);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    hipFree(d_f32);
    hipFree(d_limited);
    hipFree(d_out);
    free(host);
    return 0;
}

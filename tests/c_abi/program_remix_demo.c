/* Plain C99 host of the programme bank's channel remix (include/omx/program_remix.h): one 5.1 programme (L R C LFE Ls Rs) of two
 * seconds at 48 kHz as packed S24 (noise at a quarter of full scale from a 32-bit LCG, three times as loud for 50 ms twice a second,
 * the LFE at full level throughout) goes through the whole chain on the device: import, the fold-down to Lo/Ro (BS.775 levels, LFE
 * dropped), process at 48 kHz as stereo, plan_gains to -16 LUFS, apply_limited under -1 dBTP, export as S16 stereo with TPDF dither.
 * Prints the records and a checksum of the exported bytes.  The HIP runtime's C entry points are declared by hand: a C host needs no
 * HIP headers.
 * Exit code 0 = every call succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_remix.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char remix_info_is_16_bytes[sizeof(omx_program_remix_info) == 16 ? 1 : -1];
typedef char downmix_rule_is_20_bytes[sizeof(omx_program_downmix_rule) == 20 ? 1 : -1];
typedef char remix_record_is_32_bytes[sizeof(omx_program_remix_record) == 32 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH_IN = 6, CH_OUT = 2, FS = 48000, FRAMES = 96000, N_IN = FRAMES * CH_IN, N_OUT = FRAMES * CH_OUT };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH_OUT, 60, &bank));

    uint8_t positions_in[OMX_MAX_CHANNELS], positions_out[OMX_MAX_CHANNELS];
    omx_positions_fallback(CH_IN, positions_in);
    omx_program_downmix_rule fold;
    memset(&fold, 0, sizeof fold);
    fold.kind = OMX_REMIX_KIND_STEREO;
    fold.center_level = OMX_REMIX_DEFAULT_CENTER;
    fold.surround_level = OMX_REMIX_DEFAULT_SURROUND;
    fold.lfe_level = OMX_REMIX_DEFAULT_LFE;
    float matrix[2 * OMX_MAX_CHANNELS];
    uint32_t channels_out = 0;
    CHECK(omx_program_remix_downmix(&fold, CH_IN, positions_in, matrix, &channels_out, positions_out));
    if (channels_out != CH_OUT) return 1;
    omx_program_remix_info info;
    CHECK(omx_program_remix_plan(CH_IN, CH_OUT, &info));

    unsigned char* host = (unsigned char*)malloc((size_t)3 * N_IN);
    int16_t* exported = (int16_t*)malloc(sizeof(int16_t) * N_OUT);
    void *d_pcm = NULL, *d_f32 = NULL, *d_lo_ro = NULL, *d_limited = NULL, *d_out = NULL;
    if (!host || !exported || hipMalloc(&d_pcm, (size_t)3 * N_IN) != 0 || hipMalloc(&d_f32, sizeof(float) * N_IN) != 0 ||
        hipMalloc(&d_lo_ro, sizeof(float) * N_OUT) != 0 || hipMalloc(&d_limited, sizeof(float) * N_OUT) != 0 ||
        hipMalloc(&d_out, sizeof(int16_t) * N_OUT) != 0)
        return 1;
    uint32_t state = 12345u;
    for (long i = 0; i < N_IN; ++i) {
        state = state * 1664525u + 1013904223u;
        int v = (int)((state >> 10) & 0x3FFFFFu) - 2097152; /* a quarter of the S24 range */
        const long frame = i / CH_IN;
        if (i % CH_IN == 3) v = 4 * v;                      /* the LFE, at full scale: the fold drops it */
        else if (frame % 24000 < 2400) v = 3 * v;
        const uint32_t u = (uint32_t)v;                     /* two's complement, low 24 bits */
        host[3 * i] = (unsigned char)(u & 0xFFu);
        host[3 * i + 1] = (unsigned char)((u >> 8) & 0xFFu);
        host[3 * i + 2] = (unsigned char)((u >> 16) & 0xFFu);
    }
    if (hipMemcpy(d_pcm, host, (size_t)3 * N_IN, 1) != 0) return 1;

    CHECK(omx_program_loudness_bank_import_pcm(bank, d_pcm, OMX_PCM_S24, (float*)d_f32, FRAMES, NULL, CH_IN, NULL));
    CHECK(omx_program_loudness_bank_remix_configure(bank, CH_IN, CH_OUT, matrix, 1));
    const omx_program_remix_record* d_remix_records = NULL;
    CHECK(omx_program_loudness_bank_remix(bank, (const float*)d_f32, FRAMES, NULL, (float*)d_lo_ro, NULL, NULL, &d_remix_records));
    CHECK(omx_program_loudness_bank_process(bank, (const float*)d_lo_ro, FRAMES, NULL, NULL, CH_OUT, (float)FS, positions_out, NULL));
    omx_program_gain_rule gain_rule;
    memset(&gain_rule, 0, sizeof gain_rule);
    gain_rule.target_lufs = -16.0f;
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
    CHECK(omx_program_loudness_bank_limiter_configure(bank, &limit_rule, CH_OUT, (float)FS));
    const omx_program_limit_record* d_limit_records = NULL;
    const uint8_t flush = 1;
    CHECK(omx_program_loudness_bank_apply_limited(bank, (const float*)d_lo_ro, FRAMES, NULL, (float*)d_limited, FRAMES, &flush, d_gains, 1, NULL,
                                                  NULL, &d_limit_records));
    omx_program_export_rule export_rule;
    memset(&export_rule, 0, sizeof export_rule);
    export_rule.format = OMX_PCM_S16;
    export_rule.dither = OMX_DITHER_TPDF;
    export_rule.seed = 2025;
    CHECK(omx_program_loudness_bank_export_configure(bank, &export_rule, CH_OUT));
    const omx_program_export_record* d_export_records = NULL;
    CHECK(omx_program_loudness_bank_export_pcm(bank, (const float*)d_limited, d_out, FRAMES, NULL, NULL, &d_export_records));

    omx_program_remix_record m;
    omx_program_loudness_record r;
    omx_program_gain_record g;
    omx_program_limit_record l;
    omx_program_export_record e;
    CHECK(omx_program_loudness_bank_fetch_remixed(bank, 0, &m));
    CHECK(omx_program_loudness_bank_fetch(bank, 0, &r));
    CHECK(omx_program_loudness_bank_fetch_gains(bank, 0, 1, &g));
    CHECK(omx_program_loudness_bank_fetch_limited(bank, 0, &l));
    CHECK(omx_program_loudness_bank_fetch_exported(bank, 0, &e));
    if (hipMemcpy(exported, d_out, sizeof(int16_t) * N_OUT, 2) != 0) return 1;
    uint64_t checksum = 1469598103934665603ull; /* FNV-1a over the exported bytes */
    const unsigned char* bytes = (const unsigned char*)exported;
    for (size_t i = 0; i < sizeof(int16_t) * N_OUT; ++i) checksum = (checksum ^ bytes[i]) * 1099511628211ull;
    printf("tile %u channels_in %u channels_out %u remixed_frames %lu remixed_over %lu remixed_peak %.6f matrix %u terms %u "
           "integrated_lufs %.4f gain_db %.4f frames_limited %lu min_envelope %.6f frames_out %lu samples_clipped %lu out_peak %u format %u "
           "checksum %lu\n",
           info.tile_frames, info.channels_in, info.channels_out, (unsigned long)m.frames, (unsigned long)m.samples_over,
           (double)m.out_sample_peak, m.matrix_index, m.terms, (double)r.integrated_lufs, (double)g.gain_db, (unsigned long)l.frames_limited,
           (double)l.min_envelope, (unsigned long)e.frames_out, (unsigned long)e.samples_clipped, e.out_peak, e.format,
           (unsigned long)checksum);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    hipFree(d_f32);
    hipFree(d_lo_ro);
    hipFree(d_limited);
    hipFree(d_out);
    free(host);
    free(exported);
    return 0;
}

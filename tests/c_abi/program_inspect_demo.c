/* Plain C99 host of the programme bank's signal QC (include/omx/program_inspect.h): one stereo programme of two seconds at 48 kHz
 * (noise at a quarter of full scale from a 32-bit LCG) with three delivery defects goes to the device and through the inspector in two
 * calls: the right channel is the inverted left one (a pair out of phase), frames 10000 .. 10399 sit at positive and frames
 * 30000 .. 30399 at negative full scale (two clipped passages, flat tops of 400 samples that leave no DC offset between them) and
 * frames 50000 .. 50999 are digital silence (a dropout).  Prints the record's figures and the summary.  The HIP runtime's C entry
 * points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_inspect.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char inspect_rule_is_28_bytes[sizeof(omx_program_inspect_rule) == 28 ? 1 : -1];
typedef char inspect_record_is_704_bytes[sizeof(omx_program_inspect_record) == 704 ? 1 : -1];
typedef char inspect_summary_is_120_bytes[sizeof(omx_program_inspect_summary) == 120 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, FRAMES = 96000, FIRST_CALL = 50500 /* the cut lies inside the dropout */ };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 60, &bank));

    float* host = (float*)malloc(sizeof(float) * FRAMES * CH);
    void* d_pcm = NULL;
    if (!host || hipMalloc(&d_pcm, sizeof(float) * FRAMES * CH) != 0) return 1;
    uint32_t state = 2024u;
    for (long f = 0; f < FRAMES; ++f) {
        state = state * 1664525u + 1013904223u;
        const int v = (int)((state >> 8) & 0xFFFFFFu) - 8388608; /* 24 bits, signed */
        float left = (float)v / 33554432.0f;                    /* a quarter of full scale, exact in f32 */
        if (f >= 10000 && f < 10400) left = 1.0f;
        if (f >= 30000 && f < 30400) left = -1.0f;
        if (f >= 50000 && f < 51000) left = 0.0f;
        host[CH * f] = left;
        host[CH * f + 1] = -left;
    }
    if (hipMemcpy(d_pcm, host, sizeof(float) * FRAMES * CH, 1) != 0) return 1;

    omx_program_inspect_rule rule;
    CHECK(omx_program_inspect_rule_default(&rule));
    omx_program_inspect_info info;
    CHECK(omx_program_inspect_plan(CH, &info));
    const uint32_t pairs[2] = {0, 1};
    CHECK(omx_program_loudness_bank_inspect_configure(bank, &rule, CH, pairs, 1));
    const omx_program_inspect_record* d_records = NULL;
    const uint32_t first = FIRST_CALL, second = FRAMES - FIRST_CALL;
    CHECK(omx_program_loudness_bank_inspect(bank, (const float*)d_pcm, FRAMES, &first, NULL, &d_records));
    CHECK(omx_program_loudness_bank_inspect(bank, (const float*)d_pcm + (size_t)CH * FIRST_CALL, second, &second, NULL, &d_records));
    omx_program_inspect_record r;
    CHECK(omx_program_loudness_bank_fetch_inspected(bank, 0, &r));
    omx_program_inspect_summary s;
    CHECK(omx_program_inspect_summarize(&rule, &r, &s));

    printf("tile %u frames %lu silent_frames %lu silent_runs %lu longest_silent_run %lu longest_silent_start %lu leading %lu trailing %lu "
           "clipped_left %lu clip_runs_left %lu longest_clip_run_left %lu longest_clip_start_left %lu clip_runs_right %lu dc_sum_left %ld "
           "sum_ab %ld sum_aa %lu interior_silent_runs %lu correlation %.6f correlation_valid %u dc_offset_left %.9g verdict %u "
           "nan %u clipped %u dropout %u all_silent %u dc %u antiphase %u\n",
           info.tile_frames, (unsigned long)r.frames, (unsigned long)r.silent_frames, (unsigned long)r.silent_runs,
           (unsigned long)r.longest_silent_run, (unsigned long)r.longest_silent_start, (unsigned long)r.leading_silence,
           (unsigned long)r.trailing_silence, (unsigned long)r.channel[0].clipped_samples, (unsigned long)r.channel[0].clip_runs,
           (unsigned long)r.channel[0].longest_clip_run, (unsigned long)r.channel[0].longest_clip_start,
           (unsigned long)r.channel[1].clip_runs, (long)r.channel[0].dc_sum, (long)r.pair[0].sum_ab, (unsigned long)r.pair[0].sum_aa,
           (unsigned long)s.interior_silent_runs, (double)s.correlation[0], s.correlation_valid[0], (double)s.dc_offset[0], s.verdict,
           (s.verdict & OMX_INSPECT_NAN) != 0, (s.verdict & OMX_INSPECT_CLIPPED) != 0, (s.verdict & OMX_INSPECT_DROPOUT) != 0,
           (s.verdict & OMX_INSPECT_ALL_SILENT) != 0, (s.verdict & OMX_INSPECT_DC) != 0, (s.verdict & OMX_INSPECT_ANTIPHASE) != 0);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    free(host);
    return 0;
}

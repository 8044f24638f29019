/* Plain C99 host of the programme bank's edit pass (include/omx/program_edit.h): two stereo tracks of half a second at 48 kHz (noise
 * at a quarter of full scale from a 32-bit LCG), each with digital silence in front of it and behind it (1000 and 500 frames, 300 and
 * 700 frames), go to the device.  The inspector finds the silence, omx_program_edit_trim turns each record into the clip that cuts it
 * away, with equal-power fades of 10 ms, and the two clips are joined into ONE output in which the second track starts 480 frames
 * before the first one ends: a crossfade.  Prints the clips and the record of the call, and the bits of three output samples.  The HIP
 * runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_edit.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char edit_clip_is_48_bytes[sizeof(omx_program_edit_clip) == 48 ? 1 : -1];
typedef char trim_rule_is_48_bytes[sizeof(omx_program_trim_rule) == 48 ? 1 : -1];
typedef char edit_record_is_64_bytes[sizeof(omx_program_edit_record) == 64 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, TRACKS = 2, FRAMES = 24000, FADE = 480 };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, TRACKS, CH, 60, &bank));

    static const long lead[TRACKS] = {1000, 300}, trail[TRACKS] = {500, 700};
    const size_t floats = (size_t)TRACKS * FRAMES * CH;
    float* host = (float*)malloc(sizeof(float) * floats);
    void *d_in = NULL, *d_out = NULL;
    if (!host || hipMalloc(&d_in, sizeof(float) * floats) != 0 || hipMalloc(&d_out, sizeof(float) * floats) != 0) return 1;
    uint32_t state = 2025u;
    for (long t = 0; t < TRACKS; ++t)
        for (long f = 0; f < FRAMES; ++f)
            for (long c = 0; c < CH; ++c) {
                state = state * 1664525u + 1013904223u;
                const int v = (int)((state >> 8) & 0xFFFFFFu) - 8388608;              /* 24 bits, signed */
                const int silent = f < lead[t] || f >= FRAMES - trail[t];
                const float x = v == 0 ? 0.25f : (float)v / 33554432.0f;              /* a quarter of full scale, exact in f32, never zero */
                host[((size_t)t * FRAMES + f) * CH + c] = silent ? 0.0f : x;
            }
    if (hipMemcpy(d_in, host, sizeof(float) * floats, 1) != 0) return 1;

    /* where does the silence lie? */
    omx_program_inspect_rule qc;
    CHECK(omx_program_inspect_rule_default(&qc));
    CHECK(omx_program_loudness_bank_inspect_configure(bank, &qc, CH, NULL, 0));
    const omx_program_inspect_record* d_inspected = NULL;
    CHECK(omx_program_loudness_bank_inspect(bank, (const float*)d_in, FRAMES, NULL, NULL, &d_inspected));

    /* the clips that cut it away, joined with a crossfade */
    omx_program_trim_rule rule;
    memset(&rule, 0, sizeof(rule));
    rule.fade_in_frames = FADE;
    rule.fade_out_frames = FADE;
    rule.fade_in_curve = OMX_EDIT_CURVE_EQUAL_POWER;
    rule.fade_out_curve = OMX_EDIT_CURVE_EQUAL_POWER;
    omx_program_edit_clip clips[TRACKS];
    uint64_t kept[TRACKS];
    for (uint32_t t = 0; t < TRACKS; ++t) {
        omx_program_inspect_record r;
        CHECK(omx_program_loudness_bank_fetch_inspected(bank, t, &r));
        CHECK(omx_program_edit_trim(&r, &rule, t, 0, &clips[t], &kept[t]));
    }
    clips[1].dst_first = clips[0].frames - FADE;
    const uint32_t frames_in[TRACKS] = {FRAMES, FRAMES};
    uint64_t extent = 0;
    CHECK(omx_program_edit_extent(clips, TRACKS, TRACKS, frames_in, 1, &extent));

    omx_program_edit_info info;
    CHECK(omx_program_edit_plan(CH, &info));
    CHECK(omx_program_loudness_bank_edit_configure(bank, CH, 1));
    const omx_program_edit_record* d_edited = NULL;
    const uint32_t out_frames = (uint32_t)extent;
    CHECK(omx_program_loudness_bank_edit(bank, (const float*)d_in, FRAMES, NULL, clips, TRACKS, (float*)d_out, (uint64_t)TRACKS * FRAMES, 1, NULL,
                                         &out_frames, NULL, &d_edited));
    omx_program_edit_record e;
    CHECK(omx_program_loudness_bank_fetch_edited(bank, 0, &e));
    uint32_t bits[3];
    const uint64_t at[3] = {0, clips[1].dst_first + 7, extent - 1}; /* in the fade-in, in the crossfade, the last frame */
    for (int i = 0; i < 3; ++i)
        if (hipMemcpy(&bits[i], (const float*)d_out + at[i] * CH + 1, sizeof(uint32_t), 2) != 0) return 1;
    uint32_t peak_bits;
    memcpy(&peak_bits, &e.out_sample_peak, sizeof(peak_bits));

    printf("tile %u src_first_0 %lu frames_0 %lu src_first_1 %lu frames_1 %lu dst_first_1 %lu fade_in_0 %u fade_out_1 %u extent %lu "
           "out_first %lu frames %lu silent_frames %lu faded_frames %lu mixed_frames %lu samples_over %lu peak_bits %u peak_db %.6f clips %u "
           "first_bits %u crossfade_bits %u last_bits %u\n",
           info.tile_frames, (unsigned long)clips[0].src_first, (unsigned long)clips[0].frames, (unsigned long)clips[1].src_first,
           (unsigned long)clips[1].frames, (unsigned long)clips[1].dst_first, clips[0].fade_in_frames, clips[1].fade_out_frames,
           (unsigned long)extent, (unsigned long)e.out_first, (unsigned long)e.frames, (unsigned long)e.silent_frames,
           (unsigned long)e.faded_frames, (unsigned long)e.mixed_frames, (unsigned long)e.samples_over, peak_bits, (double)e.out_sample_peak_db,
           e.clips, bits[0], bits[1], bits[2]);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_in);
    hipFree(d_out);
    free(host);
    return 0;
}

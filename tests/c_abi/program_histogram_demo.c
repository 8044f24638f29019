/* Plain C99 host of the programme bank's bounded storage (include/omx/program_histogram.h): one stream of a stereo 1 kHz sine, 3 s at
 * -20 dBFS then 3 s at -30 dBFS, fed from device memory in calls of 0.37 s to a bounded bank and, next to it, to a stored bank of
 * capacity_seconds = 1.  The stored bank is full after the first second (overflow = 1, frames stop at 48000); the bounded bank takes
 * all six and prints its record and the bins it filled.  The HIP runtime's C entry points are declared by hand: a C host needs no
 * HIP headers.
 * Exit code 0 = every call succeeded and the two banks behaved as described. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "omx/program_histogram.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device */

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, FS = 48000, CALL = 17760, HALF_SECONDS = 3 };

int main(void) {
    static double boundaries[OMX_PROGRAM_HISTOGRAM_BINS + 1];
    static omx_program_histogram h;
    CHECK(omx_program_histogram_boundaries(boundaries));
    printf("bin 0 starts at %.17g, the top bin at %.17g\n", boundaries[0], boundaries[OMX_PROGRAM_HISTOGRAM_BINS - 1]);
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank *bounded = NULL, *stored = NULL;
    CHECK(omx_program_loudness_bank_create_bounded(&cfg, 1, CH, &bounded));
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 1, &stored));
    if (omx_program_loudness_bank_is_bounded(bounded) != 1 || omx_program_loudness_bank_is_bounded(stored) != 0) return 1;
    uint8_t positions[OMX_MAX_CHANNELS];
    omx_positions_fallback(CH, positions);
    float* host = (float*)malloc(sizeof(float) * CALL * CH);
    void* dev = NULL;
    if (!host || hipMalloc(&dev, sizeof(float) * CALL * CH) != 0) return 1;
    const double pi = 3.14159265358979323846;
    const long total = (long)FS * 2 * HALF_SECONDS;
    for (long t0 = 0; t0 < total; t0 += CALL) {
        const uint32_t frames = (uint32_t)(total - t0 < CALL ? total - t0 : CALL);
        for (long k = 0; k < (long)frames; ++k) {
            const double amplitude = pow(10.0, (t0 + k < (long)FS * HALF_SECONDS ? -20.0 : -30.0) / 20.0);
            const float v = (float)(amplitude * sin(2.0 * pi * 1000.0 * ((double)(t0 + k) / (double)FS)));
            host[k * CH] = v;
            host[k * CH + 1] = v;
        }
        if (hipMemcpy(dev, host, sizeof(float) * CALL * CH, 1) != 0) return 1;
        CHECK(omx_program_loudness_bank_process(bounded, (const float*)dev, CALL, &frames, NULL, CH, (float)FS, positions, NULL));
        CHECK(omx_program_loudness_bank_process(stored, (const float*)dev, CALL, &frames, NULL, CH, (float)FS, positions, NULL));
    }
    omx_program_loudness_record r, full;
    CHECK(omx_program_loudness_bank_fetch(bounded, 0, &r));
    CHECK(omx_program_loudness_bank_fetch(stored, 0, &full));
    printf("stored  capacity 1 s: overflow %u frames %lu segments %lu I %.4f\n", full.overflow, (unsigned long)full.frames,
           (unsigned long)full.segments, (double)full.integrated_lufs);
    printf("bounded             : overflow %u frames %lu segments %lu I %.4f LRA %.4f M %.4f S %.4f maxM %.4f maxS %.4f above %lu %lu\n",
           r.overflow, (unsigned long)r.frames, (unsigned long)r.segments, (double)r.integrated_lufs, (double)r.loudness_range_lu,
           (double)r.momentary_lufs, (double)r.short_term_lufs, (double)r.max_momentary_lufs, (double)r.max_short_term_lufs,
           (unsigned long)r.gating_above_absolute, (unsigned long)r.gating_above_relative);
    CHECK(omx_program_loudness_bank_fetch_histogram(bounded, 0, &h));
    for (int i = 0; i < OMX_PROGRAM_HISTOGRAM_BINS; ++i)
        if (h.gating_count[i])
            printf("gating bin %d (%.1f LUFS upwards): %lu blocks, mean %.4f LUFS\n", i, -70.0 + i / 10.0, (unsigned long)h.gating_count[i],
                   -0.691 + 10.0 * log10(h.gating_sum[i] / (double)h.gating_count[i]));
    printf("histogram: segments %lu tail %u\n", (unsigned long)h.segments, h.tail_count);
    if (full.overflow != 1 || full.frames != (uint64_t)FS || r.overflow != 0 || r.frames != (uint64_t)total || h.segments != 20u * HALF_SECONDS ||
        h.tail_count != OMX_PROGRAM_HISTOGRAM_TAIL)
        return 1;
    /* what needs the stored segments is refused on a bounded bank, and a stored bank has no histogram */
    double e[1];
    if (omx_program_loudness_bank_fetch_segments(bounded, 0, 0, 1, e) != OMX_ERR_UNSUPPORTED) return 1;
    if (omx_program_loudness_bank_fetch_histogram(stored, 0, &h) != OMX_ERR_INVALID) return 1;
    omx_program_loudness_bank_destroy(bounded);
    omx_program_loudness_bank_destroy(stored);
    hipFree(dev);
    free(host);
    return 0;
}

/* Plain C99 host of the programme bank's timeline and intervals (include/omx/program_timeline.h): one stream of a stereo 1 kHz sine,
 * 6 s at -20 dBFS then 6 s at -30 dBFS, fed from device memory in calls of 0.37 s; prints the loudness log once per second (momentary,
 * short-term, running integrated) and the records of the two halves measured as programmes of their own.  The HIP runtime's C entry
 * points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_timeline.h"

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

enum { CH = 2, FS = 48000, CALL = 17760, HALF_SECONDS = 6, ROWS = 2 * HALF_SECONDS };

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
        CHECK(omx_program_loudness_bank_process(bank, (const float*)dev, CALL, &frames, NULL, CH, (float)FS, positions, NULL));
    }
    /* the row at the end of every second: j = 9, 19, ... */
    omx_program_timeline_row rows[ROWS];
    CHECK(omx_program_loudness_bank_fetch_timeline(bank, 0, 9, 10, ROWS, rows));
    for (int i = 0; i < ROWS; ++i)
        printf("row %d valid %u M %.4f S %.4f I %.4f above %u %u\n", 9 + 10 * i, rows[i].valid, (double)rows[i].momentary_lufs,
               (double)rows[i].short_term_lufs, (double)rows[i].integrated_lufs, rows[i].gating_above_absolute, rows[i].gating_above_relative);
    omx_program_interval halves[2];
    memset(halves, 0, sizeof(halves));
    halves[0].first_segment = 0;
    halves[0].segment_count = 10 * HALF_SECONDS;
    halves[1].first_segment = 10 * HALF_SECONDS;
    halves[1].segment_count = 10 * HALF_SECONDS;
    omx_program_loudness_record r[2];
    CHECK(omx_program_loudness_bank_fetch_intervals(bank, halves, 2, r));
    for (int i = 0; i < 2; ++i)
        printf("interval %d segments %lu frames %lu I %.4f LRA %.4f maxM %.4f maxS %.4f\n", i, (unsigned long)r[i].segments,
               (unsigned long)r[i].frames, (double)r[i].integrated_lufs, (double)r[i].loudness_range_lu, (double)r[i].max_momentary_lufs,
               (double)r[i].max_short_term_lufs);
    /* an interval that runs past the stored segments is refused */
    halves[1].segment_count = 10 * HALF_SECONDS + 1;
    if (omx_program_loudness_bank_fetch_intervals(bank, halves, 2, r) != OMX_ERR_INVALID) return 1;
    omx_program_loudness_bank_destroy(bank);
    hipFree(dev);
    free(host);
    return 0;
}

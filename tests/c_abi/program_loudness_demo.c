/* Plain C99 host of the programme loudness bank (include/omx/program_loudness.h): two streams of a stereo 1 kHz sine at -23 and
 * -33 dBFS, 20 s each (EBU Tech 3341 cases 1 and 2), fed from device memory in calls of 0.37 s; prints the integrated loudness of
 * both, their loudness range and counts.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_loudness.h"

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

enum { S = 2, CH = 2, FS = 48000, CALL = 17760, SECONDS = 20 };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, S, CH, 60, &bank));
    uint8_t positions[OMX_MAX_CHANNELS];
    omx_positions_fallback(CH, positions);
    float* host = (float*)malloc(sizeof(float) * S * CALL * CH);
    void* dev = NULL;
    if (!host || hipMalloc(&dev, sizeof(float) * S * CALL * CH) != 0) return 1;
    const double pi = 3.14159265358979323846;
    const long total = (long)FS * SECONDS;
    for (long t0 = 0; t0 < total; t0 += CALL) {
        uint32_t frames[S];
        for (int s = 0; s < S; ++s) {
            const double amp = pow(10.0, (s == 0 ? -23.0 : -33.0) / 20.0);
            frames[s] = (uint32_t)(total - t0 < CALL ? total - t0 : CALL);
            for (long k = 0; k < (long)frames[s]; ++k) {
                const float v = (float)(amp * sin(2.0 * pi * 1000.0 * (double)(t0 + k) / FS));
                host[((long)s * CALL + k) * CH] = v;
                host[((long)s * CALL + k) * CH + 1] = v;
            }
        }
        if (hipMemcpy(dev, host, sizeof(float) * S * CALL * CH, 1) != 0) return 1;
        CHECK(omx_program_loudness_bank_process(bank, (const float*)dev, CALL, frames, NULL, CH, (float)FS, positions, NULL));
    }
    omx_program_loudness_record r[S];
    for (int s = 0; s < S; ++s) CHECK(omx_program_loudness_bank_fetch(bank, (uint64_t)s, &r[s]));
    double first[4];
    CHECK(omx_program_loudness_bank_fetch_segments(bank, 0, 0, 4, first));
    printf("integrated0 %.6f integrated1 %.6f lra0 %.6f segments %lu gating %lu above_rel %lu overflow %u e0 %.9e form %d\n",
           (double)r[0].integrated_lufs, (double)r[1].integrated_lufs, (double)r[0].loudness_range_lu, (unsigned long)r[0].segments,
           (unsigned long)r[0].gating_blocks, (unsigned long)r[0].gating_above_relative, r[0].overflow, first[0],
           omx_debug_program_loudness_bank_last_form(bank));
    omx_program_loudness_bank_destroy(bank);
    hipFree(dev);
    free(host);
    return 0;
}

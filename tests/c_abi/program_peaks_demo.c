/* Plain C99 host of the programme bank's peaks (include/omx/program_peaks.h): two streams of a stereo sine at fs/4 starting at 45
 * degrees, amplitude 0.5 (the EBU Tech 3341 true-peak tone: sample peak -9.03 dBFS, true peak -6.0 dBTP), one second each, fed from
 * device memory in calls of 0.37 s; prints the sample peak and the true peak of both and the maximum true peak the loudness record
 * reports.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_peaks.h"

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

enum { S = 2, CH = 2, FS = 48000, CALL = 17760, SECONDS = 1 };

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, S, CH, 60, &bank));
    omx_program_peak_record p[S];
    if (omx_program_loudness_bank_fetch_peaks(bank, 0, &p[0]) != OMX_ERR_INVALID) return 1; /* off by default */
    CHECK(omx_program_loudness_bank_set_peaks(bank, 1));
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
            frames[s] = (uint32_t)(total - t0 < CALL ? total - t0 : CALL);
            for (long k = 0; k < (long)frames[s]; ++k) {
                const float v = (float)(0.5 * sin(2.0 * pi * (double)((t0 + k) % 4) / 4.0 + pi / 4.0));
                host[((long)s * CALL + k) * CH] = v;
                host[((long)s * CALL + k) * CH + 1] = v;
            }
        }
        if (hipMemcpy(dev, host, sizeof(float) * S * CALL * CH, 1) != 0) return 1;
        CHECK(omx_program_loudness_bank_process(bank, (const float*)dev, CALL, frames, NULL, CH, (float)FS, positions, NULL));
    }
    omx_program_loudness_record r[S];
    for (int s = 0; s < S; ++s) {
        CHECK(omx_program_loudness_bank_fetch_peaks(bank, (uint64_t)s, &p[s]));
        CHECK(omx_program_loudness_bank_fetch(bank, (uint64_t)s, &r[s]));
    }
    printf("sample_peak0 %.6f true_peak0 %.6f sample_peak1 %.6f true_peak1 %.6f record_true_peak0 %.6f frames %lu oversampling %u channels %u\n",
           (double)p[0].max_sample_peak_db, (double)p[0].max_true_peak_db, (double)p[1].max_sample_peak_db, (double)p[1].max_true_peak_db,
           (double)r[0].max_true_peak_db, (unsigned long)p[0].frames, p[0].oversampling, p[0].channels);
    omx_program_loudness_bank_destroy(bank);
    hipFree(dev);
    free(host);
    return 0;
}

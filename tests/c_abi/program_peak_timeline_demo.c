/* Plain C99 host of the programme bank's peak timeline (include/omx/program_peak_timeline.h): one stereo stream of a sine at fs/4
 * starting at 45 degrees (the EBU Tech 3341 true-peak tone), two seconds, amplitude 0.25 in the first and 0.5 in the second, fed from
 * device memory in calls of 0.37 s.  Prints the peak log per second (two rows of stride 10: the second reads sample peak -9.03 dBFS
 * and true peak -6.0 dBTP, the first 6.02 dB less), the interval peak of the second second and the whole-programme peak.
 * The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_peak_timeline.h"

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

enum { CH = 2, FS = 48000, CALL = 17760, SECONDS = 2 };

static double db(float peak) { return 20.0 * log10((double)peak); }

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 60, &bank));
    omx_program_peak_row rows[2];
    if (omx_program_loudness_bank_set_peak_timeline(bank, 1) != OMX_ERR_INVALID) return 1; /* needs the peaks */
    CHECK(omx_program_loudness_bank_set_peaks(bank, 1));
    if (omx_program_loudness_bank_fetch_peak_rows(bank, 0, 0, 10, 2, rows) != OMX_ERR_INVALID) return 1; /* off by default */
    CHECK(omx_program_loudness_bank_set_peak_timeline(bank, 1));
    uint8_t positions[OMX_MAX_CHANNELS];
    omx_positions_fallback(CH, positions);
    float* host = (float*)malloc(sizeof(float) * CALL * CH);
    void* dev = NULL;
    if (!host || hipMalloc(&dev, sizeof(float) * CALL * CH) != 0) return 1;
    const double pi = 3.14159265358979323846;
    const long total = (long)FS * SECONDS;
    for (long t0 = 0; t0 < total; t0 += CALL) {
        uint32_t frames = (uint32_t)(total - t0 < CALL ? total - t0 : CALL);
        for (long k = 0; k < (long)frames; ++k) {
            const double amplitude = t0 + k < FS ? 0.25 : 0.5;
            const float v = (float)(amplitude * sin(2.0 * pi * (double)((t0 + k) % 4) / 4.0 + pi / 4.0));
            host[k * CH] = v;
            host[k * CH + 1] = v;
        }
        if (hipMemcpy(dev, host, sizeof(float) * CALL * CH, 1) != 0) return 1;
        CHECK(omx_program_loudness_bank_process(bank, (const float*)dev, CALL, &frames, NULL, CH, (float)FS, positions, NULL));
    }
    CHECK(omx_program_loudness_bank_fetch_peak_rows(bank, 0, 0, 10, 2, rows));
    omx_program_interval second;
    memset(&second, 0, sizeof(second));
    second.first_segment = 10;
    second.segment_count = OMX_PROGRAM_TO_END;
    omx_program_part_peak part;
    omx_program_peak_record whole;
    CHECK(omx_program_loudness_bank_fetch_interval_peaks(bank, &second, 1, &part));
    CHECK(omx_program_loudness_bank_fetch_peaks(bank, 0, &whole));
    printf("row0_true_peak %.6f row0_sample_peak %.6f row1_true_peak %.6f row1_sample_peak %.6f row1_frames %u row1_valid %u "
           "part_true_peak %.6f part_frames %lu part_first_frame %lu whole_true_peak %.6f\n",
           db(rows[0].true_peak[0]), db(rows[0].sample_peak[0]), db(rows[1].true_peak[1]), db(rows[1].sample_peak[1]), rows[1].frames,
           rows[1].valid, (double)part.max_true_peak_db, (unsigned long)part.frames, (unsigned long)part.true_peak_frame[0],
           (double)whole.max_true_peak_db);
    omx_program_loudness_bank_destroy(bank);
    hipFree(dev);
    free(host);
    return 0;
}

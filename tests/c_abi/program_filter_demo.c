/* Plain C99 host of the programme bank's filter stage (include/omx/program_filter.h): one stereo programme of two seconds at 48 kHz, a
 * 1 kHz tone at a quarter of full scale on a DC offset of 0.25, goes to the device and through a 20 Hz fourth-order Butterworth
 * high-pass, in place and in two calls.  Prints the filter's response, the plan, the record of the second call and what is left of
 * the offset in the last tenth of a second.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "omx/program_filter.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char filter_section_is_40_bytes[sizeof(omx_program_filter_section) == 40 ? 1 : -1];
typedef char filter_is_88_bytes[sizeof(omx_program_filter) == 88 ? 1 : -1];
typedef char filter_spec_is_48_bytes[sizeof(omx_program_filter_spec) == 48 ? 1 : -1];
typedef char filter_record_is_48_bytes[sizeof(omx_program_filter_record) == 48 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, FRAMES = 96000, FIRST_CALL = 50001, TAIL = 4800 };

int main(void) {
    const double fs = 48000.0;
    omx_program_filter_spec spec = {OMX_FILTER_HIGHPASS, 4, 20.0, 0.0, 0.0, 0.0, 0.0};
    omx_program_filter filter;
    CHECK(omx_program_filter_design(&spec, fs, &filter));
    CHECK(omx_program_filter_check(&filter));
    double at_corner = 0.0, at_tone = 0.0;
    CHECK(omx_program_filter_response(&filter, fs, 20.0, &at_corner, NULL));
    CHECK(omx_program_filter_response(&filter, fs, 1000.0, &at_tone, NULL));
    omx_program_filter_info info;
    CHECK(omx_program_filter_plan(CH, fs, &info));
    printf("sections %u corner_db %.6f tone_db %.6f chunk %u tile %u ", filter.n_sections, at_corner, at_tone, info.chunk_frames,
           info.tile_frames);
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
    for (long f = 0; f < FRAMES; ++f) {
        const float v = (float)(0.25 + 0.25 * sin(2.0 * 3.14159265358979323846 * 1000.0 * (double)f / fs));
        host[CH * f] = v;
        host[CH * f + 1] = -v;
    }
    if (hipMemcpy(d_pcm, host, sizeof(float) * FRAMES * CH, 1) != 0) return 1;

    CHECK(omx_program_loudness_bank_filter_configure(bank, CH, fs, &filter, 1, NULL));
    const omx_program_filter_record* d_records = NULL;
    const uint32_t first = FIRST_CALL, second = FRAMES - FIRST_CALL;
    float* d_second = (float*)d_pcm + (size_t)CH * FIRST_CALL;
    CHECK(omx_program_loudness_bank_filter(bank, (const float*)d_pcm, FRAMES, &first, (float*)d_pcm, NULL, &d_records));
    CHECK(omx_program_loudness_bank_filter(bank, d_second, second, &second, d_second, NULL, &d_records));
    omx_program_filter_record r;
    CHECK(omx_program_loudness_bank_fetch_filtered(bank, 0, &r));
    if (hipMemcpy(host, d_pcm, sizeof(float) * FRAMES * CH, 2) != 0) return 1;
    double mean = 0.0;
    for (long f = FRAMES - TAIL; f < FRAMES; ++f) mean += (double)host[CH * f];
    mean /= (double)TAIL;

    printf("frames %lu frames_total %lu samples_over %lu samples_nonfinite %lu peak %.9g peak_db %.6f form %u last_form %d offset_left %.3e\n",
           (unsigned long)r.frames, (unsigned long)r.frames_total, (unsigned long)r.samples_over, (unsigned long)r.samples_nonfinite,
           (double)r.out_sample_peak, (double)r.out_sample_peak_db, r.form, omx_debug_program_loudness_bank_filter_last_form(bank), mean);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    free(host);
    return 0;
}

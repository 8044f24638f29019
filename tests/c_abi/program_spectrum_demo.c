/* Plain C99 host of the programme bank's long-term spectrum (include/omx/program_spectrum.h): one mono programme of two seconds at
 * 48 kHz, a sine of amplitude 0.5 at 1 kHz, goes to the device and through the spectrum stage in two calls, the second of which
 * finishes the stream.  Prints the record, the third-octave table (the 1 kHz band reads about -6 dB) and the QC summary, checks
 * them and ends with "ok".  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded and every figure is what a sine of that level gives. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "omx/program_spectrum.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char spectrum_rule_is_8_bytes[sizeof(omx_program_spectrum_rule) == 8 ? 1 : -1];
typedef char spectrum_record_is_152_bytes[sizeof(omx_program_spectrum_record) == 152 ? 1 : -1];
typedef char spectrum_summary_is_104_bytes[sizeof(omx_program_spectrum_summary) == 104 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { FRAMES = 96000, FIRST_CALL = 50500 /* the cut lies inside a transform */ };

int main(void) {
    if (!omx_device_available()) {
        printf("no device: ok\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, 1, 60, &bank));

    omx_program_spectrum_rule rule;
    CHECK(omx_program_spectrum_rule_default(&rule));
    omx_program_spectrum_info info;
    CHECK(omx_program_spectrum_plan(&rule, 1, 1, FRAMES, &info));
    float* host = (float*)malloc(sizeof(float) * FRAMES);
    double* sums = (double*)malloc(sizeof(double) * info.bins);
    double* density = (double*)malloc(sizeof(double) * info.bins);
    void* d_pcm = NULL;
    if (!host || !sums || !density || hipMalloc(&d_pcm, sizeof(float) * FRAMES) != 0) return 1;
    for (long f = 0; f < FRAMES; ++f) host[f] = (float)(0.5 * sin(2.0 * 3.14159265358979323846 * 1000.0 * (double)f / 48000.0));
    if (hipMemcpy(d_pcm, host, sizeof(float) * FRAMES, 1) != 0) return 1;

    CHECK(omx_program_loudness_bank_spectrum_configure(bank, &rule, 1));
    const omx_program_spectrum_record* d_records = NULL;
    const double* d_sums = NULL;
    const uint32_t first = FIRST_CALL, second = FRAMES - FIRST_CALL;
    const uint8_t finish = 1;
    CHECK(omx_program_loudness_bank_spectrum(bank, (const float*)d_pcm, FRAMES, &first, NULL, NULL, &d_records, &d_sums));
    CHECK(omx_program_loudness_bank_spectrum(bank, (const float*)d_pcm + FIRST_CALL, second, &second, &finish, NULL, &d_records, &d_sums));
    omx_program_spectrum_record r;
    CHECK(omx_program_loudness_bank_fetch_spectrum(bank, 0, &r, sums));
    uint64_t expected = 0;
    CHECK(omx_program_spectrum_transforms(FRAMES, 1, rule.fft_size, &expected));
    CHECK(omx_program_spectrum_density(&r, sums, 0, density));

    printf("fft_size %u transforms_per_workgroup %u run %u frames %lu transforms %lu expected %lu skipped %lu finished %u\n", info.fft_size,
           info.transforms_per_workgroup, info.run, (unsigned long)r.frames, (unsigned long)r.transforms[0], (unsigned long)expected,
           (unsigned long)r.skipped[0], r.finished);
    double centre[OMX_SPECTRUM_MAX_BANDS], level[OMX_SPECTRUM_MAX_BANDS];
    uint32_t n = OMX_SPECTRUM_MAX_BANDS;
    CHECK(omx_program_spectrum_bands(density, rule.fft_size, 48000.0, 3, centre, level, &n));
    for (uint32_t i = 0; i < n; ++i) printf("band %8.1f Hz %8.2f dB\n", centre[i], level[i]);
    omx_program_spectrum_qc qc;
    CHECK(omx_program_spectrum_qc_default(&qc));
    omx_program_spectrum_summary s;
    CHECK(omx_program_spectrum_summarize(&qc, density, rule.fft_size, 48000.0, &s));
    printf("total %.2f dB peak %.1f Hz %.2f dB occupied %.1f Hz verdict %u bandlimited %u tone %u\n", s.total_db, s.peak_hz, s.peak_db,
           s.occupied_hz, s.verdict, (s.verdict & OMX_SPECTRUM_BANDLIMITED) != 0, (s.verdict & OMX_SPECTRUM_TONE) != 0);
    /* the demo checks its own figures: the grid's transform count, the sine's band within 0.1 dB of 20 log10(0.5), every other
     * band 30 dB under it, the peak at 1 kHz within a bin, a spectrum that ends far below fs/2 and no hum */
    int failed = 0;
    double tone_level = OMX_SPECTRUM_DB_FLOOR, other_level = OMX_SPECTRUM_DB_FLOOR;
    for (uint32_t i = 0; i < n; ++i) {
        if (fabs(centre[i] - 1000.0) < 1e-6) tone_level = level[i];
        else if (level[i] > other_level) other_level = level[i];
    }
    if (r.frames != FRAMES || r.transforms[0] != expected || r.skipped[0] != 0 || r.finished != 1 || r.fft_size != rule.fft_size) failed |= 1;
    if (fabs(tone_level + 6.0206) > 0.1 || other_level > tone_level - 30.0) failed |= 2;
    if (fabs(s.peak_hz - 1000.0) > 48000.0 / rule.fft_size || fabs(s.total_db + 6.0206) > 0.1) failed |= 4;
    if (!(s.verdict & OMX_SPECTRUM_BANDLIMITED) || (s.verdict & OMX_SPECTRUM_TONE)) failed |= 8;
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_pcm);
    free(host);
    free(sums);
    free(density);
    if (failed) {
        printf("FAILED checks %d\n", failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}

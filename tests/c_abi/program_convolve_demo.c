/* Plain C99 host of the programme bank's convolve stage (include/omx/program_convolve.h): designs a 255-tap low-pass at 8 kHz for
 * 48 kHz PCM (host only, no device needed) and prints its response in the passband, at the corner and in the stopband.  Where a device
 * is present it then filters a unit impulse at frame 300 of a stereo stream with the delay compensated (D = 127), the second channel
 * bypassed, in two cuts of 200 and 312 frames and a flush: the first channel comes out as the taps, centred on frame 300 (1.0f times a
 * tap plus zeros is the tap, on bits), the second as the impulse where it was.  The HIP runtime's C entry points are declared by hand:
 * a C host needs no HIP headers.
 * Exit code 0 = every call succeeded and, with a device, the output is the taps. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_convolve.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char fir_is_16_bytes[sizeof(omx_program_fir) == 16 ? 1 : -1];
typedef char convolve_spec_is_32_bytes[sizeof(omx_program_convolve_spec) == 32 ? 1 : -1];
typedef char convolve_info_is_16_bytes[sizeof(omx_program_convolve_info) == 16 ? 1 : -1];
typedef char convolve_record_is_64_bytes[sizeof(omx_program_convolve_record) == 64 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, TAPS = 255, DELAY = 127, FRAMES = 512, CUT = 200, AT = 300 };

int main(void) {
    static float taps[TAPS];
    omx_program_convolve_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.kind = OMX_CONVOLVE_LOWPASS;
    spec.n_taps = TAPS;
    spec.f_hi_hz = 8000.0;
    spec.beta = 9.0;
    CHECK(omx_program_convolve_design(&spec, 48000.0, taps, TAPS));
    omx_program_fir fir;
    fir.taps = taps;
    fir.n_taps = TAPS;
    fir.flags = 0;
    CHECK(omx_program_convolve_check(&fir));
    const double at_hz[3] = {1000.0, 8000.0, 12000.0};
    for (int i = 0; i < 3; ++i) {
        double db = 0.0, phase = 0.0;
        CHECK(omx_program_convolve_response(&fir, 48000.0, at_hz[i], &db, &phase));
        printf("response %.0f Hz %.4f dB %.6f rad\n", at_hz[i], db, phase);
    }
    omx_program_convolve_info info;
    CHECK(omx_program_convolve_plan(CH, TAPS, &info));
    uint64_t first = 0, second = 0, tail = 0;
    CHECK(omx_program_convolve_frames(DELAY, 0, 0, CUT, 0, &first));
    CHECK(omx_program_convolve_frames(DELAY, CUT, first, FRAMES - CUT, 0, &second));
    CHECK(omx_program_convolve_frames(DELAY, FRAMES, first + second, 0, 1, &tail));
    printf("tile %u frames_per_thread %u tap_block %u emits %lu %lu %lu\n", info.tile_frames, info.frames_per_thread, info.tap_block,
           (unsigned long)first, (unsigned long)second, (unsigned long)tail);
    if (first + second + tail != FRAMES) return 2;

    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 60, &bank));
    const uint32_t fir_of_channel[CH] = {0, OMX_CONVOLVE_BYPASS};
    CHECK(omx_program_loudness_bank_convolve_configure(bank, CH, &fir, 1, fir_of_channel, DELAY));

    static float host[FRAMES * CH], out[FRAMES * CH];
    host[AT * CH] = 1.0f;
    host[AT * CH + 1] = 1.0f;
    void *d_in = NULL, *d_out = NULL;
    if (hipMalloc(&d_in, sizeof(host)) != 0 || hipMalloc(&d_out, sizeof(out)) != 0) return 1;
    if (hipMemcpy(d_in, host, sizeof(host), 1) != 0) return 1;
    const omx_program_convolve_record* d_records = NULL;
    omx_program_convolve_record rec;
    const uint8_t flush = 1;
    uint32_t frames = CUT;
    uint64_t done = 0;
    /* cut 1: frames 0 .. 199; cut 2: the rest; then a call that brings nothing and flushes */
    CHECK(omx_program_loudness_bank_convolve(bank, (const float*)d_in, FRAMES, &frames, (float*)d_out, FRAMES, NULL, NULL, &d_records));
    CHECK(omx_program_loudness_bank_fetch_convolved(bank, 0, &rec));
    if (hipMemcpy(out, d_out, sizeof(float) * CH * rec.frames_written, 2) != 0) return 1;
    done = rec.frames_written;
    frames = FRAMES - CUT;
    CHECK(omx_program_loudness_bank_convolve(bank, (const float*)d_in + (size_t)CUT * CH, FRAMES - CUT, &frames, (float*)d_out, FRAMES, NULL,
                                             NULL, &d_records));
    CHECK(omx_program_loudness_bank_fetch_convolved(bank, 0, &rec));
    if (hipMemcpy(out + done * CH, d_out, sizeof(float) * CH * rec.frames_written, 2) != 0) return 1;
    done += rec.frames_written;
    frames = 0;
    CHECK(omx_program_loudness_bank_convolve(bank, NULL, 0, &frames, (float*)d_out, FRAMES, &flush, NULL, &d_records));
    CHECK(omx_program_loudness_bank_fetch_convolved(bank, 0, &rec));
    if (hipMemcpy(out + done * CH, d_out, sizeof(float) * CH * rec.frames_written, 2) != 0) return 1;
    done += rec.frames_written;

    int wrong = 0;
    for (int m = 0; m < FRAMES; ++m) {
        const int k = m - AT + DELAY; /* out[m] = h[m + D - 300] */
        const float want = k >= 0 && k < TAPS ? taps[k] : 0.0f;
        if (memcmp(&out[m * CH], &want, sizeof(float)) != 0 && !(want == 0.0f && out[m * CH] == 0.0f)) ++wrong;
        if (out[m * CH + 1] != host[m * CH + 1]) ++wrong;
    }
    printf("frames_in %lu frames_out %lu state %u delay %u max_taps %u peak %.9g peak_db %.4f wrong %d\n", (unsigned long)rec.frames_in,
           (unsigned long)rec.frames_out, rec.state, rec.delay_frames, rec.max_taps, (double)rec.out_sample_peak,
           (double)rec.out_sample_peak_db, wrong);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_in);
    hipFree(d_out);
    return done == FRAMES && rec.state == OMX_CONVOLVE_FLUSHED && wrong == 0 ? 0 : 2;
}

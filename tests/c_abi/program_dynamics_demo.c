/* Plain C99 host of the programme bank's dynamics stage (include/omx/program_dynamics.h): designs a 4:1 compressor at -20 dB (host
 * only, no device needed), prints its gain at a few levels, and turns 1 ms, 10 ms and 60 dB/s at 48 kHz into frames and a release
 * step.  Where a device is present it then runs a stereo stream of 0.5 DC through the stage in two cuts and a flush, with the gain
 * trace: a 0.5 DC input settles to exactly the curve's gain at -6.02 dB, about -10.4845 dB, and every output sample of the settled
 * part is the same value.  The HIP runtime's C entry points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded and, with a device, the output settled where the curve says.  The last line says "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_dynamics.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char curve_is_3096_bytes[sizeof(omx_program_dynamics_curve) == 3096 ? 1 : -1];
typedef char dynamics_spec_is_56_bytes[sizeof(omx_program_dynamics_spec) == 56 ? 1 : -1];
typedef char dynamics_info_is_32_bytes[sizeof(omx_program_dynamics_info) == 32 ? 1 : -1];
typedef char dynamics_record_is_104_bytes[sizeof(omx_program_dynamics_record) == 104 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, FRAMES = 3000, CUT = 1100 };

int main(void) {
    static omx_program_dynamics_curve curve;
    omx_program_dynamics_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.threshold_db = -20.0;
    spec.ratio = 4.0;
    spec.expander_ratio = 1.0;
    CHECK(omx_program_dynamics_design(&spec, &curve));
    curve.detector_mask = 3;
    CHECK(omx_program_dynamics_time(48000.0, 1.0, 10.0, 60.0, &curve.attack_frames, &curve.hold_frames, &curve.release_step));
    CHECK(omx_program_dynamics_check(&curve));
    uint32_t latency = 0;
    CHECK(omx_program_dynamics_latency(&curve, &latency));
    const double at_db[4] = {-60.0, -20.0, -6.020599913279624, 0.0};
    double settled_db = 0.0;
    for (int i = 0; i < 4; ++i) {
        double g = 0.0;
        CHECK(omx_program_dynamics_gain_db(&curve, at_db[i], &g));
        printf("gain at %.2f dB: %.6f dB\n", at_db[i], g);
        if (i == 2) settled_db = g;
    }
    omx_program_dynamics_info info;
    CHECK(omx_program_dynamics_plan(CH, &info));
    uint64_t first = 0, second = 0, tail = 0;
    CHECK(omx_program_dynamics_frames(latency, 0, 0, CUT, 0, &first));
    CHECK(omx_program_dynamics_frames(latency, CUT, first, FRAMES - CUT, 0, &second));
    CHECK(omx_program_dynamics_frames(latency, FRAMES, first + second, 0, 1, &tail));
    printf("attack %u hold %u step %lld latency %u release tile %u smooth tile %u emits %lu %lu %lu\n", curve.attack_frames, curve.hold_frames,
           (long long)curve.release_step, latency, info.release_tile, info.smooth_tile, (unsigned long)first, (unsigned long)second,
           (unsigned long)tail);
    if (first + second + tail != FRAMES) return 2;

    if (!omx_device_available()) {
        printf("no device: ok\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, 1, CH, 60, &bank));
    CHECK(omx_program_loudness_bank_dynamics_configure(bank, CH, &curve, 1, NULL));

    static float host[FRAMES * CH], out[FRAMES * CH], gains[FRAMES];
    for (int i = 0; i < FRAMES * CH; ++i) host[i] = 0.5f;
    void *d_in = NULL, *d_out = NULL, *d_gain = NULL;
    if (hipMalloc(&d_in, sizeof(host)) != 0 || hipMalloc(&d_out, sizeof(out)) != 0 || hipMalloc(&d_gain, sizeof(gains)) != 0) return 1;
    if (hipMemcpy(d_in, host, sizeof(host), 1) != 0) return 1;
    const omx_program_dynamics_record* d_records = NULL;
    omx_program_dynamics_record rec;
    const uint8_t flush = 1;
    uint64_t done = 0;
    /* cut 1: frames 0 .. 1099; cut 2: the rest; then a call that brings nothing and flushes */
    for (int call = 0; call < 3; ++call) {
        uint32_t frames = call == 0 ? CUT : (call == 1 ? FRAMES - CUT : 0);
        const float* in = call == 2 ? NULL : (const float*)d_in + (size_t)(call == 0 ? 0 : CUT) * CH;
        CHECK(omx_program_loudness_bank_dynamics(bank, in, NULL, frames, &frames, (float*)d_out, (float*)d_gain, FRAMES, call == 2 ? &flush : NULL,
                                                 NULL, &d_records));
        CHECK(omx_program_loudness_bank_fetch_dynamics(bank, 0, &rec));
        if (hipMemcpy(out + done * CH, d_out, sizeof(float) * CH * rec.frames_written, 2) != 0) return 1;
        if (hipMemcpy(gains + done, d_gain, sizeof(float) * rec.frames_written, 2) != 0) return 1;
        done += rec.frames_written;
    }
    int wrong = 0;
    for (int m = 1000; m < 2000; ++m) { /* settled: past the attack, in front of the silence behind the flush */
        if ((double)gains[m] - settled_db > 1e-5 || settled_db - (double)gains[m] > 1e-5) ++wrong;
        if (memcmp(&out[m * CH], &out[1000 * CH], sizeof(float)) != 0 || out[m * CH] != out[m * CH + 1]) ++wrong;
    }
    printf("frames_in %lu frames_out %lu reduced %lu state %u latency %u min_gain_db %.4f settled %.6f dB out %.9g wrong %d\n",
           (unsigned long)rec.frames_in, (unsigned long)rec.frames_out, (unsigned long)rec.frames_reduced, rec.state, rec.latency_frames,
           (double)rec.min_gain_db, (double)gains[1500], (double)out[1500 * CH], wrong);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_gain);
    if (done != FRAMES || rec.state != OMX_DYNAMICS_FLUSHED || wrong != 0) return 2;
    printf("ok\n");
    return 0;
}

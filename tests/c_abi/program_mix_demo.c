/* Plain C99 host of the programme bank's mix pass (include/omx/program_mix.h): three stereo stems of a quarter of a second at 48 kHz
 * (noise from a 32-bit LCG on a 2^-16 lattice inside +-0.25) and their printmaster, the sum of the three, which is exact on that
 * lattice.  One call sums the stems into bus 0 and runs the null test on bus 1: every stem at +1, then the printmaster at -1
 * (omx_program_mix_null).  The residual's level is the floor: the stems explain the printmaster to the last bit.  Then stem 1 is moved
 * by one step of the lattice at one sample and the call repeated: the residual's peak is 2^-16, -96.33 dB.  The HIP runtime's C entry
 * points are declared by hand: a C host needs no HIP headers.
 * Exit code 0 = every call succeeded and the clean null test left nothing. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omx/program_mix.h"

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1 = host to device, 2 = device to host */

typedef char mix_send_is_40_bytes[sizeof(omx_program_mix_send) == 40 ? 1 : -1];
typedef char mix_info_is_16_bytes[sizeof(omx_program_mix_info) == 16 ? 1 : -1];
typedef char mix_record_is_64_bytes[sizeof(omx_program_mix_record) == 64 ? 1 : -1];

#define CHECK(expr)                                                           \
    do {                                                                      \
        int rc_ = (expr);                                                     \
        if (rc_ < 0) {                                                        \
            fprintf(stderr, "%s -> %d (%s)\n", #expr, rc_, omx_last_error()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

enum { CH = 2, STEMS = 3, STREAMS = 4, FRAMES = 12000, BUSES = 2, OFF_FRAME = 777 };

static uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
}

int main(void) {
    if (!omx_device_available()) {
        printf("no device\n");
        return 0;
    }
    omx_loudness_config cfg;
    omx_loudness_config_default(&cfg);
    omx_program_loudness_bank* bank = NULL;
    CHECK(omx_program_loudness_bank_create(&cfg, STREAMS, CH, 60, &bank));

    const size_t row = (size_t)FRAMES * CH, floats = (size_t)STREAMS * row;
    float* host = (float*)malloc(sizeof(float) * floats);
    void *d_in = NULL, *d_out = NULL;
    if (!host || hipMalloc(&d_in, sizeof(float) * floats) != 0 || hipMalloc(&d_out, sizeof(float) * BUSES * row) != 0) return 1;
    uint32_t state = 2026u;
    for (size_t i = 0; i < (size_t)STEMS * row; ++i) {
        state = state * 1664525u + 1013904223u;
        host[i] = (float)((int)((state >> 8) & 0x7FFFu) - 16384) / 65536.0f; /* a multiple of 2^-16 in [-0.25, 0.25) */
    }
    for (size_t i = 0; i < row; ++i) host[STEMS * row + i] = host[i] + host[row + i] + host[2 * row + i]; /* the printmaster: exact */
    if (hipMemcpy(d_in, host, sizeof(float) * floats, 1) != 0) return 1;

    /* bus 0: the stems, summed; bus 1: the null test */
    omx_program_mix_send sends[STEMS + STEMS + 1];
    const uint32_t stems[STEMS] = {0, 1, 2};
    memset(sends, 0, sizeof(sends));
    for (uint32_t s = 0; s < STEMS; ++s) {
        sends[s].src_stream = s;
        sends[s].frames = FRAMES;
        sends[s].gain = 1.0f;
    }
    CHECK(omx_program_mix_null(stems, STEMS, STEMS, FRAMES, 1, sends + STEMS));
    const uint32_t frames_in[STREAMS] = {FRAMES, FRAMES, FRAMES, FRAMES};
    uint64_t extent[BUSES] = {0, 0};
    CHECK(omx_program_mix_extent(sends, STEMS + STEMS + 1, STREAMS, frames_in, BUSES, extent));

    omx_program_mix_info info;
    CHECK(omx_program_mix_plan(CH, &info));
    CHECK(omx_program_loudness_bank_mix_configure(bank, CH, BUSES));
    const uint32_t out_frames[BUSES] = {(uint32_t)extent[0], (uint32_t)extent[1]};
    const omx_program_mix_record* d_mixed = NULL;
    omx_program_mix_record sum, clean, off;
    CHECK(omx_program_loudness_bank_mix(bank, (const float*)d_in, FRAMES, NULL, sends, STEMS + STEMS + 1, (float*)d_out, FRAMES, BUSES, NULL,
                                        out_frames, NULL, &d_mixed));
    CHECK(omx_program_loudness_bank_fetch_mixed(bank, 0, &sum));
    CHECK(omx_program_loudness_bank_fetch_mixed(bank, 1, &clean));
    float sample = 0.0f;
    if (hipMemcpy(&sample, (const float*)d_out + (size_t)OFF_FRAME * CH + 1, sizeof(float), 2) != 0) return 1;

    /* one stem one step of the lattice off, at one sample */
    host[row + (size_t)OFF_FRAME * CH + 1] += 1.0f / 65536.0f;
    if (hipMemcpy(d_in, host, sizeof(float) * floats, 1) != 0) return 1;
    CHECK(omx_program_loudness_bank_mix(bank, (const float*)d_in, FRAMES, NULL, sends, STEMS + STEMS + 1, (float*)d_out, FRAMES, BUSES, NULL,
                                        out_frames, NULL, &d_mixed));
    CHECK(omx_program_loudness_bank_fetch_mixed(bank, 1, &off));

    printf("tile %u batch %u extent_0 %lu extent_1 %lu sum_frames %lu sum_mixed %lu sum_sends %u sum_layers %u sum_peak_bits %u "
           "sum_sample_bits %u null_sends %u null_layers %u null_mixed %lu null_nonfinite %lu null_peak_bits %u null_peak_db %.6f "
           "floor_db %.6f off_peak_bits %u off_peak_db %.6f\n",
           info.tile_frames, info.layers_per_batch, (unsigned long)extent[0], (unsigned long)extent[1], (unsigned long)sum.frames,
           (unsigned long)sum.mixed_frames, sum.sends, sum.max_layers, bits_of(sum.out_sample_peak), bits_of(sample), clean.sends,
           clean.max_layers, (unsigned long)clean.mixed_frames, (unsigned long)clean.samples_nonfinite, bits_of(clean.out_sample_peak),
           (double)clean.out_sample_peak_db, (double)cfg.floor_db, bits_of(off.out_sample_peak), (double)off.out_sample_peak_db);
    omx_program_loudness_bank_destroy(bank);
    hipFree(d_in);
    hipFree(d_out);
    free(host);
    return clean.out_sample_peak == 0.0f && clean.out_sample_peak_db == cfg.floor_db && off.out_sample_peak > 0.0f ? 0 : 2;
}

// Peaks of the programme loudness bank (include/omx/program_peaks.h states the definition): maximum true peak and maximum sample
// peak per (stream, channel) with the frame they first occur at.  program_peaks_kernels.hip holds the two kernels, program_peaks.cpp
// the host side (members of ProgramLoudnessBank) and the C ABI.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_peaks.h"

namespace omx {

struct PlStreamCall;

constexpr uint32_t kPkTile = 1024;    // frames per work item (stream, tile) of the peak pass
constexpr uint32_t kPkRun = 16;       // frames per lane: a wavefront covers one channel of a tile
constexpr uint32_t kPkMaxDelay = 24;  // taps of the 2x interpolator; the 4x one has 12

struct PkPartial {  // one (stream, channel, tile): frames count from the start of the call
    float true_peak;
    uint32_t true_peak_frame;
    float sample_peak;
    uint32_t sample_peak_frame;
};

struct PkArgs {
    const float* pcm;  // [n_streams][frames_capacity][channels]
    uint64_t frames_capacity;
    uint32_t n_streams, channels;
    uint32_t n_tiles;    // tiles of the longest stream of the call (row length of `partials`)
    uint32_t delay_len;  // 12 (4x), 24 (2x) or 0 (sample peak only)
    float floor_db;
    const PlStreamCall* calls;  // [n_streams]
    float* delay;               // [n_streams][8][kPkMaxDelay]: entry j < delay_len - 1 = x[N - (delay_len - 1) + j], the history of the next call
    PkPartial* partials;        // [n_streams][channels][n_tiles]
    omx_program_peak_record* records;  // [n_streams]: the running records (the fold reads and rewrites them)
    float fir4[12][3];          // TRUE_PEAK_FIRS.0 (loudness/processor.rs:90-97)
    float fir2[24];             // TRUE_PEAK_FIRS.1
    // the peak timeline (program_peak_timeline.hpp), read by the timeline form of the tile kernel alone; null: the timeline is off
    unsigned long long* tl_keys;  // [n_streams][tl_rows][channels][2]
    uint64_t tl_rows;             // rows per stream: capacity in segments + 1
    uint32_t seg;                 // frames per segment
};
void launch_pk_tiles(const PkArgs& a, hipStream_t stream);
void launch_pk_fold(const PkArgs& a, hipStream_t stream);
void launch_pk_clear(omx_program_peak_record* records, float* delay, uint32_t n_streams, float floor_db, hipStream_t stream);

}  // namespace omx

// The convolve stage of the programme loudness bank (include/omx/program_convolve.h states the definition): a FIR per channel on device
// PCM, f64 accumulation in the order of the taps.  program_convolve_kernels.hip holds the kernels, program_convolve_plan.hpp the
// host-only half (plan, design, check, response, the streaming formula), program_convolve.cpp the host side (members of
// ProgramLoudnessBank) and the C ABI.
//
// One call runs, per stream and on the caller's stream: begin (counters, state) -> main (tiles of output frames: per block of taps the
// input span goes to LDS, a thread computes R consecutive frames of one channel; the record's reductions) -> carry (the newest
// max_taps - 1 input frames into the ring the next call reads) -> finish (the record's dB field).
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_convolve_plan.hpp"

namespace omx {

// What one call does to one stream: made on the host (which mirrors N, E and the flushed flag), uploaded per call.
struct CvStreamCall {
    uint64_t n_old;     // N before the call
    uint64_t e_old;     // E before the call
    int64_t rel_e;      // e_old + D - n_old: the newest input frame the call's first emitted frame reads, counted from the call's first
    uint32_t frames;    // F: frames taken in this call
    uint32_t emit;      // E' - E: frames written to d_out[s]
    uint32_t ring;      // n_old mod (max_taps - 1): the ring's slot of frame n_old
    uint32_t flags;     // kCarryFlag*
    uint32_t reach;     // taps the stream's channels reach back over: its longest FIR, D + 1 where a channel is bypassed
    uint32_t _pad;
};

// The FIR of one (stream, channel): where its f64 taps start in the table and how many they are; n_taps 0: bypass
struct CvChannel {
    uint32_t tap_first, n_taps;
};

struct CvArgs {
    const float* in;            // [n_streams][frames_capacity][channels]
    float* out;                 // [n_streams][out_capacity][channels]
    uint64_t frames_capacity, out_capacity;
    uint32_t n_streams, channels;
    uint32_t delay;             // D
    uint32_t max_taps;
    uint32_t history;           // max_taps - 1: frames of the ring
    float floor_db;
    const double* taps;         // the FIRs' taps as f64 (the conversion is exact), each FIR from a multiple of 8
    const CvChannel* chan;      // [n_streams][OMX_MAX_CHANNELS]
    const CvStreamCall* calls;  // [n_streams]
    omx_program_convolve_record* records;  // [n_streams]: the running records
    float* ring;                // [n_streams][history][channels]: x[n] at slot n mod history
    uint32_t max_frames, max_emit;  // the longest of the call
};
// whole_call: a convolve call (the counters and the state are written); else only the clears of a reset
void launch_cv_begin(const CvArgs& a, bool whole_call, hipStream_t stream);
void launch_cv_main(const CvArgs& a, hipStream_t stream);
void launch_cv_carry(const CvArgs& a, hipStream_t stream);
void launch_cv_finish(const CvArgs& a, hipStream_t stream);

// The stage's state: made by convolve_configure, nothing of it exists before.
struct ProgramConvolve {
    uint32_t channels = 0, delay = 0, max_taps = 1;
    std::vector<CarryLedger> h_streams;
    std::vector<uint32_t> h_reach;  // [n_streams]
    std::vector<CvStreamCall> h_calls;
    DeviceBuffer<CvStreamCall> calls;
    DeviceBuffer<omx_program_convolve_record> records;
    DeviceBuffer<double> taps;
    DeviceBuffer<CvChannel> chan;
    DeviceBuffer<float> ring;
    BlobStaging staging;
};

}  // namespace omx

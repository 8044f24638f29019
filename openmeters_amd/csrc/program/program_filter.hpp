// Filter stage of the programme loudness bank (include/omx/program_filter.h states the definition): cascades of up to two biquad
// sections on device PCM, per (stream, channel).  program_filter_kernels.hip holds the kernels, program_filter_plan.hpp the host-only
// functions and the tables, program_filter.cpp the host side (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, on the caller's stream, in one of two evaluation orders (the machine of the loudness pass, program_loudness.hpp, with
// the caller's coefficients, writing the samples instead of their energies):
//   reference order : pass (one work item per stream = the whole call, state carried from call to call) -> fold (the record)
//   time-parallel   : zero-state end states of the full work items -> scan of the zero-input transition -> the items again from their
//                     start states -> fold
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_filter_plan.hpp"

namespace omx {

constexpr uint32_t kFlSlots = OMX_MAX_CHANNELS;  // state is laid out [stream][8 channel slots] whatever the channel count

// What one call does to one stream: made on the host, uploaded per call.
struct FlStreamCall {
    uint32_t frames;        // frames of this call (reset: the flag)
    uint32_t _pad;
    uint64_t frames_total;  // frames since the stream's reset, this call included
};

// What a work item saw of its lane's output
struct FlPartial {
    uint32_t over, nonfinite;
    float peak;
    uint32_t _pad;
};

struct FlArgs {
    const float* in;   // [n_streams][frames_capacity][channels]
    float* out;        // the same layout; may be `in`
    uint64_t frames_capacity;
    uint32_t n_streams, channels, slot_shift;  // lane = (stream << slot_shift) + channel
    uint32_t chunk;     // frames per work item: the whole call (reference order) or kFlChunkFrames
    uint32_t n_chunks;  // work items per stream
    uint32_t form;      // what the record says: 1 or 2
    float floor_db;
    const FlStreamCall* calls;           // [n_streams]
    const uint32_t* lane_filter;         // [n_streams][8]: table index or OMX_FILTER_BYPASS (slots behind the channels: bypass)
    const omx_program_filter* filters;   // [n_filters]
    double* state;      // [n_streams][8][4]: s1, s2 of section 0, s1, s2 of section 1
    double* starts;     // [n_streams][8][n_chunks][4] start state of every work item (reference order: `state` itself)
    FlPartial* partials;  // [n_streams][8][n_chunks]
    const double* zs_weights;   // [n_filters][weights_stride]: [chunk][4], the weight of sample k of a work item on its zero-state end state
    const double* transition;   // [n_filters][2][4][4]: zero-input transition over `chunk` frames, high parts then low parts
    uint64_t weights_stride;    // doubles per filter in zs_weights
    omx_program_filter_record* records;  // [n_streams]
};
void launch_fl_reset(const FlArgs& a, hipStream_t stream);  // a.calls[s].frames != 0: stream s gets zero state and a zero record
void launch_fl_reference_order(const FlArgs& a, hipStream_t stream);
void launch_fl_time_parallel(const FlArgs& a, hipStream_t stream);
void launch_fl_fold(const FlArgs& a, hipStream_t stream);

// The filter stage's state: made by filter_configure, nothing of it exists before.
struct ProgramFilter {
    uint32_t channels = 0, n_filters = 0;
    double sample_rate = 0.0;
    bool time_parallel_ok = false;     // every filter of the table holds the parity bar (fl_time_parallel_ok)
    uint64_t weights_stride = 0;
    std::vector<uint64_t> h_total;     // the host's mirror of frames_total
    std::vector<FlStreamCall> h_calls;
    DeviceBuffer<FlStreamCall> calls;
    DeviceBuffer<uint32_t> lane_filter;
    DeviceBuffer<omx_program_filter> filters;
    DeviceBuffer<double> state, starts, zs_weights, transition;
    DeviceBuffer<FlPartial> partials;
    DeviceBuffer<omx_program_filter_record> records;
    BlobStaging staging;
};

}  // namespace omx

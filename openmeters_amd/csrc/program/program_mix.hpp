// Mix pass of the programme loudness bank (include/omx/program_mix.h states the definition): stem mix buses, many streams into one.
// program_mix_plan.hpp holds everything that needs no device (validation, spans, the null-test table), program_mix_kernels.hip the
// kernels, program_mix.cpp the host side (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per bus and on the caller's stream: begin (the fresh record, its counts from the host's table) -> main (tiles of the
// bus window: a tile finds its spans and zero-fills each or sums its layers in f64, in table order; the record's reductions) ->
// finish (the record's dB field).
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_mix_plan.hpp"

namespace omx {

struct MxArgs {
    const float* in;   // [n_streams][frames_capacity][channels]
    float* out;        // [n_out][out_capacity][channels]
    uint64_t out_capacity;
    uint32_t n_out, channels;
    uint32_t max_frames;             // the longest window of the call
    float floor_db;
    const MxBusCall* calls;          // [n_out]; null: every bus gets the record of a call that brought nothing
    const MxSpan* spans;             // the call's span list
    const MxSend* sends;             // [n_sends] by table index
    const uint32_t* list;            // the call's index list: the table indices of the sends over each span, in table order
    omx_program_mix_record* records;   // [max_buses]
};
void launch_mx_begin(const MxArgs& a, hipStream_t stream);
void launch_mx_main(const MxArgs& a, hipStream_t stream);
void launch_mx_finish(const MxArgs& a, hipStream_t stream);

// The mixer's state: made by mix_configure, nothing of it exists before.
struct ProgramMix {
    uint32_t channels = 0, max_buses = 0;
    DeviceBuffer<omx_program_mix_record> records;
    DeviceBuffer<uint8_t> tables;    // the call's blob: [MxBusCall x n_out][MxSpan x spans][MxSend x n_sends][u32 x layers]; grown on demand
    std::vector<uint8_t> h_tables;
    std::vector<MxSpan> h_spans;     // host scratch of a call
    std::vector<uint32_t> h_list, h_span_begin;
    BlobStaging staging;
};

}  // namespace omx

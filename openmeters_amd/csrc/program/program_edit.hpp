// Edit pass of the programme loudness bank (include/omx/program_edit.h states the definition): clips, trims, fades and crossfades on
// device PCM.  program_edit_plan.hpp holds everything that needs no device (validation, spans, the phase and curve function, the
// trim helper), program_edit_kernels.hip the kernels, program_edit.cpp the host side (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per output stream and on the caller's stream: begin (the fresh record, its counts from the host's table) -> main
// (tiles of the output window: a tile finds its spans and zero-fills, copies, scales, sums or fades each; the record's reductions) ->
// finish (the record's dB field).
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_edit_plan.hpp"

namespace omx {

constexpr uint64_t kEdMaxClips = 1ull << 26;  // of one table: span indices are 32 bits, a clip makes at most four spans and a gap

struct EdArgs {
    const float* in;   // [n_streams][frames_capacity][channels]
    float* out;        // [n_out][out_capacity][channels]
    uint64_t out_capacity;
    uint32_t n_out, channels;
    uint32_t max_frames;             // the longest window of the call
    float floor_db;
    const float* tabs;               // [3][4097] the curve tables
    const EdStreamCall* calls;       // [n_out]; null: every output gets the record of a call that brought nothing
    const EdSpan* spans;             // the call's span list
    const EdClip* clips;             // [n_clips] by table index
    omx_program_edit_record* records;  // [max_outputs]
};
void launch_ed_begin(const EdArgs& a, hipStream_t stream);
void launch_ed_main(const EdArgs& a, hipStream_t stream);
void launch_ed_finish(const EdArgs& a, hipStream_t stream);

// The editor's state: made by edit_configure, nothing of it exists before.
struct ProgramEdit {
    uint32_t channels = 0, max_outputs = 0;
    DeviceBuffer<float> tabs;
    DeviceBuffer<omx_program_edit_record> records;
    DeviceBuffer<uint8_t> tables;    // the call's blob: [EdStreamCall x n_out][EdSpan x spans][EdClip x n_clips]; grown on demand
    std::vector<uint8_t> h_tables;
    std::vector<EdSpan> h_spans;     // host scratch of a call
    std::vector<uint32_t> h_span_begin;
    BlobStaging staging;
};

}  // namespace omx

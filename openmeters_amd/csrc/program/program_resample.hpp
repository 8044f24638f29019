// Sample-rate conversion of the programme loudness bank (include/omx/program_resample.h states the definition): a rational polyphase
// FIR on device PCM.  program_resample_kernels.hip holds the kernels, program_resample.cpp the plan, the table, the host side
// (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per stream and on the caller's stream: begin (counters, state) -> main (tiles of output frames: the input frames a
// tile reaches go to LDS, a thread computes one output frame for all channels; the record's reductions) -> carry (the newest T - 1
// input frames into the ring the next call reads) -> finish (the record's dB field).
#pragma once
#include <memory>

#include "../common.hpp"
#include "../../../include/omx/program_resample.h"
#include "program_carried.hpp"

namespace omx {

constexpr uint32_t kRsThreads = 256;          // threads per workgroup of the main kernel: at most one output frame each
// Input frames one tile may stage.  2048 frames x 8 channels x 4 bytes = 64 KiB, what a workgroup gets without opting in to more; the
// tile of a plan is the longest (at most kRsThreads) whose reach, (tile - 1) * M / L + 1 + T frames, fits: 256 for every common pair
// (44.1 -> 48 kHz reaches 299 frames, 96 -> 48 kHz 639), 16 at the far end (L = 1, M = 64, T = 1024).
constexpr uint32_t kRsStageFrames = 2048;

// What one call does to one stream: made on the host (which mirrors N, E and the flushed flag), uploaded per call.
struct RsStreamCall {
    uint64_t n_old;     // N before the call
    uint64_t e_old;     // E before the call
    int64_t rel_e;      // (e_old * M) / L - n_old: i0 of the call's first emitted frame, counted from the call's first input frame
    uint32_t phase_e;   // (e_old * M) % L
    uint32_t frames;    // F: frames taken in this call
    uint32_t emit;      // E' - E: frames written to d_out[s]
    uint32_t ring;      // n_old mod (T - 1): the ring's slot of frame n_old
    uint32_t flags;     // kCarryFlag*
    uint32_t _pad;
};

struct RsArgs {
    const float* in;            // [n_streams][frames_capacity][channels]
    float* out;                 // [n_streams][out_capacity][channels]
    uint64_t frames_capacity, out_capacity;
    uint32_t n_streams, channels;
    uint32_t L, M, taps, half;  // T, H
    uint32_t tile;              // output frames per workgroup
    uint32_t history;           // T - 1: frames of the ring
    float floor_db;
    const float* table;         // [T / 4][L][4]: tap k of phase p at ((k / 4) * L + p) * 4 + k % 4
    const RsStreamCall* calls;  // [n_streams]
    omx_program_resample_record* records;  // [n_streams]: the running records
    float* ring;                // [n_streams][history][channels]: x[n] at slot n mod history
    uint32_t max_frames, max_emit;  // the longest of the call
};
// whole_call: a resample call (the counters and the state are written); else only the clears of a reset
void launch_rs_begin(const RsArgs& a, bool whole_call, hipStream_t stream);
void launch_rs_main(const RsArgs& a, hipStream_t stream);
void launch_rs_carry(const RsArgs& a, hipStream_t stream);
void launch_rs_finish(const RsArgs& a, hipStream_t stream);

// The plan of a rule (host): OMX_NONE, OMX_ERR_INVALID or OMX_ERR_UNSUPPORTED
int rs_plan(const omx_program_resample_rule* rule, omx_program_resample_info* info);
// The [L][T] table of a valid rule, the one function behind omx_program_resample_taps and resampler_configure
void rs_build_taps(const omx_program_resample_rule& rule, const omx_program_resample_info& info, float* dst);
// E' of a stream with N frames taken (E emitted before), flushed or not
uint64_t rs_emitted(const omx_program_resample_info& info, uint64_t n, uint64_t e, bool flush);

// The resampler's state: made by resampler_configure, nothing of it exists before.
struct ProgramResampler {
    omx_program_resample_rule rule{};
    omx_program_resample_info info{};
    uint32_t channels = 0;
    std::vector<CarryLedger> h_streams;
    std::vector<RsStreamCall> h_calls;
    DeviceBuffer<RsStreamCall> calls;
    DeviceBuffer<omx_program_resample_record> records;
    DeviceBuffer<float> table, ring;
    BlobStaging staging;
};

}  // namespace omx

// Long-term spectrum of the programme loudness bank (include/omx/program_spectrum.h states the definition): Welch sums of every stream
// and channel on a fixed frame grid.  program_spectrum_kernels.hip holds the kernels, program_spectrum_plan.hpp the host-only
// functions, program_spectrum.cpp the host side (members of ProgramLoudnessBank) and the C ABI.
//
// The host mirrors every count of a stream (frames held, transforms taken, frames carried, which carry buffer is current), so a call
// goes up as one table of SpCall entries and runs, on the caller's stream: begin (streams: the records' counters) -> transform (stream
// x channel x run of R transforms: window, N/2-point complex transform in LDS, untangle, power, the run's chain in f64 registers; every
// run goes to a scratch row) -> chain (stream x channel x bins: the call's complete runs onto the closed sum in ascending run order,
// the row of an open run into the stream's state, S = closed + open run) -> carry (the frames the next transform starts with).
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_spectrum_plan.hpp"

namespace omx {

// One stream's part of a call, made on the host.  A call sees the stream as its carried frames followed by the frames it brings:
// "logical" frame i is carry[i] for i < carried, d_in[i - carried] for i < carried + frames, zero behind (a finish).  Transform
// k0 + t starts at logical frame t * H.
struct SpCall {
    uint32_t frames;       // brought by this call (reset: the flag)
    uint32_t carried;      // frames in the current carry buffer, < N
    uint32_t k0;           // index of the first transform the call takes
    uint32_t nk;           // transforms the call takes
    uint32_t shift;        // logical frame the carry starts at after the call (0: the new frames are appended in place)
    uint32_t keep;         // frames the carry holds after the call
    uint32_t parity;       // the carry buffer the call reads
    uint32_t finish;       // the call finishes the stream
};
static_assert(sizeof(SpCall) == 32, "SpCall goes up as two 16-byte vectors per stream");

struct SpArgs {
    const float* in;                // [n_streams][frames_capacity][channels]
    uint64_t frames_capacity;
    uint32_t n_streams, channels, fft_size;
    const SpCall* calls;            // [n_streams]
    omx_program_spectrum_record* records;  // [n_streams]
    double* sums;                   // [n_streams][channels][bins]: S
    double* closed;                 // [n_streams][channels][bins]: the chain over the complete runs
    double* open;                   // [n_streams][channels][bins]: the chain of the run that is still open (zero: none)
    double* rows;                   // [n_streams][channels][max_rows][bins]: the runs the call touches, complete or open
    float* carry;                   // [2][n_streams][fft_size][channels]
    const float* window;            // [fft_size]
    const float* tw256;             // exp(-2 pi i k / 256), k < 256
    const float* tw_half;           // exp(-2 pi i k / (N/2)), k < N/2
    const float* tw_full;           // exp(-2 pi i k / N), k < N/2
    uint32_t max_rows;              // rows of the stream that touches the most runs
    uint32_t max_units;             // (run, channel) pairs of the stream with the most runs touched
    uint32_t max_move;              // floats the carry pass moves for the stream that moves the most
};
void launch_sp_reset(const SpArgs& a, hipStream_t stream);  // a.calls[s].frames != 0: stream s starts over
void launch_sp_begin(const SpArgs& a, hipStream_t stream);
void launch_sp_transform(const SpArgs& a, hipStream_t stream);
void launch_sp_chain(const SpArgs& a, hipStream_t stream);
void launch_sp_carry(const SpArgs& a, hipStream_t stream);

// The stage's state: made by spectrum_configure, nothing of it exists before.
struct ProgramSpectrum {
    omx_program_spectrum_rule rule{};
    uint32_t channels = 0;
    std::vector<uint64_t> h_frames;   // the host's mirror of the frames a stream holds
    std::vector<uint64_t> h_taken;    // ... of the transforms it has taken
    std::vector<uint32_t> h_carried;  // ... of the frames it carries
    std::vector<uint8_t> h_parity, h_finished;
    std::vector<SpCall> h_call;       // [n_streams] host scratch of a call
    DeviceBuffer<SpCall> call;
    DeviceBuffer<omx_program_spectrum_record> records;
    DeviceBuffer<double> sums, closed, open;
    DeviceBuffer<double> rows;        // grown on demand
    DeviceBuffer<float> carry, window, tw256, tw_half, tw_full;
    BlobStaging staging;
};

}  // namespace omx

// Dynamics stage of the programme loudness bank (include/omx/program_dynamics.h states the definition): a compressor and expander on
// device PCM.  program_dynamics_kernels.hip holds the kernels, program_dynamics.cpp the host side (members of ProgramLoudnessBank)
// and the C ABI, program_dynamics_plan.hpp the host-only functions and the tables of constants.
//
// One call runs, per stream and on the caller's stream: begin (counters) -> level (key PCM -> one int32 Gt per frame) -> hold (sliding
// minimum) -> release (min-plus scan inside tiles, one aggregate per tile) -> chain (the carry into every tile of a stream) -> apply
// (r from the tile's carry, exact boxcar, floor division, factor by table, out = x * k, the trace, the record's reductions) -> carry
// (the rings the next call reads) -> finish (the record's dB fields).  What lies between the f32 level and the f64 factor is integer,
// so tiles with halos give the bits of the sample-by-sample definition.
#pragma once
#include <memory>

#include "../common.hpp"
#include "program_dynamics_plan.hpp"

namespace omx {

// What one call does to one stream: made on the host (which mirrors N, E and the flushed flag), uploaded per call.
struct DyStreamCall {
    uint64_t n_old;       // N before the call
    int64_t step;         // d of the stream's curve
    uint32_t frames;      // F: frames taken in this call
    uint32_t emit;        // E' - E: frames written to d_out[s]
    uint32_t held;        // N - E before the call (<= LA): emitted frame f of the call is x[n_old - held + f]
    uint32_t scan;        // values of r the call computes: F, and LA more with the flush
    uint32_t flags;       // kCarryFlag*
    uint32_t curve;       // row of the curve table (a bypassed stream: the row of zeros), and what the record reports in curve_index
    uint32_t curve_index;
    uint32_t mask;        // detector_mask
    uint32_t attack;      // A
    uint32_t window;      // W = A + H
    uint32_t ring_x;      // n_old mod LA: the PCM ring's slot of frame n_old (also the slot of r[n_old])
    uint32_t ring_g;      // n_old mod (W - 1): the Gt ring's slot
};

struct DyArgs {
    const float* in;            // [n_streams][frames_capacity][channels]
    const float* key;           // the side chain, as in (never null on the device: the host passes in)
    float* out;                 // [n_streams][out_capacity][channels]
    float* gain_db;             // [n_streams][out_capacity] or null
    uint64_t frames_capacity, out_capacity;
    uint32_t n_streams, channels;
    uint32_t max_latency;       // the largest LA: row length of the PCM and r rings (at least 1)
    uint32_t max_history;       // the largest W - 1: row length of the Gt ring (at least 1)
    float floor_db;
    const DyStreamCall* calls;  // [n_streams]
    omx_program_dynamics_record* records;  // [n_streams]: the running records
    const int32_t* curves;      // [n_curves + 1][772]: T of every curve, then a row of zeros for bypassed streams
    const int32_t* log_table;   // [257]
    const unsigned long long* exp_table;  // [257]
    long long* carry;           // [n_streams]: r[N - 1]
    float* ring_x;              // [n_streams][max_latency][channels]: x[n] at slot n mod LA
    int32_t* ring_g;            // [n_streams][max_history]: Gt[n] at slot n mod (W - 1)
    long long* ring_r;          // [n_streams][max_latency]: r[n] at slot n mod LA
    int32_t* gt;                // [n_streams][g_row]: Gt of the call's frames
    int32_t* held_min;          // [n_streams][m_row]: window-L minima (program_dynamics_kernels.hip)
    long long* r_local;         // [n_streams][r_row]: r of the call's values as if every tile began the stream
    long long* tile_agg;        // [n_streams][t_row]: the last r_local of every tile
    long long* tile_carry;      // [n_streams][t_row]: r in front of every tile
    uint32_t g_row, m_row, r_row, t_row;
    uint32_t max_frames, max_emit, max_scan;  // the longest of the call
    uint32_t max_attack;        // the largest A of the bank: sizes the apply pass's LDS
};
constexpr uint32_t kDyCurveRow = 772;   // int32 per row of the curve table (769 and padding to 16 bytes)

// whole_call: a dynamics call (the counters and the state are written); else only the clears of a reset
void launch_dy_begin(const DyArgs& a, bool whole_call, hipStream_t stream);
void launch_dy_level(const DyArgs& a, hipStream_t stream);
void launch_dy_hold(const DyArgs& a, hipStream_t stream);
void launch_dy_release(const DyArgs& a, hipStream_t stream);
void launch_dy_chain(const DyArgs& a, hipStream_t stream);
void launch_dy_apply(const DyArgs& a, hipStream_t stream);
void launch_dy_carry(const DyArgs& a, hipStream_t stream);
void launch_dy_finish(const DyArgs& a, hipStream_t stream);

// The stage's state: made by dynamics_configure, nothing of it exists before.
struct ProgramDynamics {
    uint32_t channels = 0, n_curves = 0, max_attack = 1, max_latency = 1, max_history = 1;
    struct Stream : CarryLedger {
        uint32_t curve = 0, curve_index = 0, mask = 1, attack = 1, hold = 0;
        int64_t step = 1;
    };
    std::vector<Stream> h_streams;
    std::vector<DyStreamCall> h_calls;
    DeviceBuffer<DyStreamCall> calls;
    DeviceBuffer<omx_program_dynamics_record> records;
    DeviceBuffer<int32_t> curves, log_table, ring_g, gt, held_min;
    DeviceBuffer<unsigned long long> exp_table;
    DeviceBuffer<long long> carry, ring_r, r_local, tile_agg, tile_carry;
    DeviceBuffer<float> ring_x;
    BlobStaging staging;
};

}  // namespace omx

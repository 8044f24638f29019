// Limiter of the programme loudness bank (include/omx/program_limit.h states the definition): a look-ahead true-peak limiter on device
// PCM.  program_limit_kernels.hip holds the kernels, program_limit.cpp the host side (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per stream and on the caller's stream: begin (latch, counters) -> level (PCM -> one u32 q per frame) -> hold (sliding
// minimum) -> smooth (exact boxcar, the f32 envelope) -> apply (out = x * (g * Gf), the record's reductions) -> carry (the rings the
// next call reads) -> finish (the record's dB fields).  What lies between the f32 level and the f32 envelope is integer, so tiles
// with halos give the bits of the sample-by-sample definition.
#pragma once
#include <memory>

#include "../common.hpp"
#include "../../../include/omx/program_limit.h"
#include "program_carried.hpp"

namespace omx {

constexpr uint32_t kLmLevelTile = 1024, kLmLevelThreads = 256;  // frames per workgroup of the level pass (four per thread)
constexpr uint32_t kLmHoldTile = 2048;    // frames per workgroup of the hold pass
constexpr uint32_t kLmHoldMaxWindow = 2048;  // longest window one hold tile takes in LDS; a longer W is the minimum of shifted windows
constexpr uint32_t kLmSmoothTile = 2048;  // frames per workgroup of the smooth pass
constexpr uint32_t kLmApplyThreads = 256, kLmApplyInFlight = 4;
constexpr uint32_t kLmApplyTileVecs = kLmApplyThreads * kLmApplyInFlight, kLmApplyTileFloats = kLmApplyTileVecs * 4;
constexpr uint32_t kLmHistory = 23;       // frames in front of a frame that its level reads (the 2x interpolator has 24 taps)
constexpr uint32_t kLmUnity = 1u << 24;   // q of a frame at or below the ceiling

constexpr uint32_t kLmFlagLatch = 4u;     // the stream takes its first frame: the gain is read (beside kCarryFlag*)

// What one call does to one stream: made on the host (which mirrors N, E and the flushed flag), uploaded per call.
struct LmStreamCall {
    uint64_t n_old;       // N before the call
    uint32_t frames;      // F: frames taken in this call
    uint32_t emit;        // E' - E: frames written to d_out[s]
    uint32_t held;        // N - E before the call (<= LA): emitted frame f of the call is x[n_old - held + f]
    uint32_t gain_index;  // read with kLmFlagLatch
    uint32_t flags;       // kCarryFlag*, kLmFlagLatch
    uint32_t ring_x;      // n_old mod LA: the PCM ring's slot of frame n_old
    uint32_t ring_q;      // n_old mod history length of q
    uint32_t _pad;
};

struct LmArgs {
    const float* in;            // [n_streams][frames_capacity][channels]
    float* out;                 // [n_streams][out_capacity][channels]
    uint64_t frames_capacity, out_capacity;
    uint32_t n_streams, channels;
    uint32_t attack, window;    // A, W = A + 24 + R
    uint32_t latency;           // LA = A + 23: frames of the PCM ring
    uint32_t q_history;         // W + A - 2: entries of the q ring (what the hold and the smooth pass read in front of a call)
    uint32_t hold_len;          // L = min(W, kLmHoldMaxWindow): the window of the hold pass
    uint32_t delay_len;         // 12 (4x), 24 (2x) or 0 (sample peak only)
    float ceiling, floor_db;
    const LmStreamCall* calls;  // [n_streams]
    const omx_program_gain_record* gains;
    omx_program_limit_record* records;  // [n_streams]: the running records
    float* ring_x;              // [n_streams][latency][channels]: x[n] at slot n mod latency
    uint32_t* ring_q;           // [n_streams][q_history]: q[n] at slot n mod q_history
    uint32_t* q;                // [n_streams][q_row]: q of the call's frames
    uint32_t* held_min;         // [n_streams][m_row]: window-L minima, entry i = index n_old' + i (program_limit_kernels.hip)
    float* envelope;            // [n_streams][e_row]: Gf of the call's emitted frames
    uint32_t q_row, m_row, e_row;
    uint32_t max_frames, max_emit;  // the longest of the call
    float fir4[12][3];          // as PkArgs
    float fir2[24];
};
// whole_call: an apply_limited call (the counters and the state are written); else only the clears of a reset
void launch_lm_begin(const LmArgs& a, bool whole_call, hipStream_t stream);
void launch_lm_level(const LmArgs& a, hipStream_t stream);
void launch_lm_hold(const LmArgs& a, hipStream_t stream);
void launch_lm_smooth(const LmArgs& a, hipStream_t stream);
void launch_lm_apply(const LmArgs& a, hipStream_t stream);
void launch_lm_carry(const LmArgs& a, hipStream_t stream);
void launch_lm_finish(const LmArgs& a, hipStream_t stream);

// The limiter's state: made by limiter_configure, nothing of it exists before.
struct ProgramLimiter {
    omx_program_limit_rule rule{};
    uint32_t channels = 0;
    float rate = 0.0f, ceiling = 0.0f;
    std::vector<CarryLedger> h_streams;
    std::vector<LmStreamCall> h_calls;
    DeviceBuffer<LmStreamCall> calls;
    DeviceBuffer<omx_program_limit_record> records;
    DeviceBuffer<float> ring_x, envelope;
    DeviceBuffer<uint32_t> ring_q, q, held_min;
    BlobStaging staging;
};

}  // namespace omx

// Normalisation of the programme loudness bank (include/omx/program_normalize.h): gains planned on the device from the bank's own
// records (program_gain_device.hpp is the definition, shared with the host) and the pass that scales PCM by them.
// program_normalize_kernels.hip holds the kernels; program_normalize.cpp validates on the host and uploads one small table per call.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_normalize.h"
#include "program_groups.hpp"

namespace omx {

// per-stream source records -> gains[n]
void launch_pn_plan(const omx_program_gain_rule& rule, const omx_program_loudness_record* records, omx_program_gain_record* gains, uint32_t n,
                    float floor_db, hipStream_t stream);
// group records + the member streams' peaks -> gains[n_groups]; one wavefront per group
void launch_pn_plan_groups(const omx_program_gain_rule& rule, const omx_program_loudness_record* group_records,
                           const omx_program_loudness_record* stream_records, const PgMember* members, const PgGroup* groups,
                           omx_program_gain_record* gains, uint32_t n_groups, float floor_db, hipStream_t stream);

// What one apply_gains call does to one stream: made on the host, uploaded per call.
struct PnStreamCall {
    uint64_t n;           // floats to scale: frames * channels
    uint32_t gain_index;  // OMX_PROGRAM_UNITY_GAIN: factor 1
    uint32_t _pad;
};

// The pass moves a row in tiles of kPnTileFloats floats: 256 threads, kPnInFlight accesses of 16 bytes each.
constexpr uint32_t kPnThreads = 256, kPnInFlight = 4;
constexpr uint32_t kPnTileVecs = kPnThreads * kPnInFlight, kPnTileFloats = kPnTileVecs * 4;

struct PnApplyArgs {
    const float* in;
    float* out;
    uint64_t row;                       // floats per row: frames_capacity * channels
    const PnStreamCall* calls;          // [n_streams]
    const omx_program_gain_record* gains;
    omx_program_apply_record* applied;  // [n_streams]
    uint32_t n_streams, channels;
    float floor_db;
};
// begin: the apply records written fresh (frames, the factor, the index; count and peak cleared).  tiles: the pass, max_n = the
// longest row of the call in floats (not launched for 0).  finish: the peak's dB field.
void launch_pn_begin(const PnApplyArgs& a, hipStream_t stream);
void launch_pn_tiles(const PnApplyArgs& a, uint64_t max_n, bool non_temporal, hipStream_t stream);
void launch_pn_finish(const PnApplyArgs& a, hipStream_t stream);

}  // namespace omx

// Signal QC of the programme loudness bank (include/omx/program_inspect.h states the definition): DC, clipping runs, dropouts,
// leading and trailing silence, NaN samples and pair correlation of device PCM.  program_inspect_kernels.hip holds the kernels,
// program_inspect.cpp the host-only functions, the host side (members of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per stream and on the caller's stream: main (tiles of frames: the integer sums of a tile go into the call's table
// of tile sums, the predicates leave as ballot words that the workgroup itself folds into one run summary per predicate and tile) ->
// fold (one workgroup per stream adds up the tile sums, composes the tile summaries in order and folds both into the running record
// with plain stores).
#pragma once
#include <memory>

#include "../common.hpp"
#include "../../../include/omx/program_inspect.h"

namespace omx {

constexpr uint32_t kInThreads = 256;  // threads per workgroup of the main kernel
constexpr uint32_t kInFoldMaxThreads = 1024;  // of the fold kernel, at the most

// Frames one thread takes; a tile is kInThreads times as many: 2048 frames with up to 2 channels, else 1024, that is 32 or 16 ballot
// words per predicate and 8 to 32 KiB of PCM per workgroup.  More frames per thread spread the wavefront reductions of the sums
// (one per channel and three per pair) over more samples.
constexpr uint32_t in_frames_per_thread(uint32_t channels) { return channels <= 2 ? 8 : 4; }
constexpr uint32_t in_tile_frames(uint32_t channels) { return kInThreads * in_frames_per_thread(channels); }

// The runs of one predicate over a stretch of frames.  Summaries compose associatively (in_compose, program_inspect_kernels.hip);
// every field fits 32 bits because a stream holds at most 2^32 - 1 frames between resets.
struct InRuns {
    uint32_t len;     // frames of the stretch
    uint32_t head;    // set frames at its start (len when all are set)
    uint32_t tail;    // set frames at its end (len when all are set)
    uint32_t best;    // the longest run inside it
    uint32_t start;   // where the earliest run of that length starts, from the stretch's first frame
    uint32_t reach;   // frames at which a run reached the minimum length, counted with no run open at the stretch's start
    uint32_t set;     // set frames
    uint32_t _pad;
};
static_assert(sizeof(InRuns) == 32, "InRuns is stored as two 16-byte vectors");

struct InArgs {
    const float* in;  // [n_streams][frames_capacity][channels]
    uint64_t frames_capacity;
    uint32_t n_streams, channels, n_pairs;
    uint32_t clip_min_run, silence_min_run;
    float clip_level, silence_level;
    uint32_t pair_a[OMX_INSPECT_MAX_PAIRS], pair_b[OMX_INSPECT_MAX_PAIRS];
    const uint32_t* frames;          // [n_streams]: frames of this call (reset: the flags)
    omx_program_inspect_record* records;  // [n_streams]
    InRuns* runs;                    // [n_streams][tiles][channels + 1]: the call's tile summaries, the quiet predicate last
    long long* sums;                 // [n_streams][2 * channels + 3 * n_pairs][tiles]: the call's tile sums (dc and NaN count per
                                     // channel, then ab, aa, bb per pair)
    uint32_t tiles;                  // tiles of the longest stream of the call
    uint32_t max_frames;
};
void launch_in_reset(const InArgs& a, hipStream_t stream);  // a.frames[s] != 0: stream s gets a zero record
void launch_in_main(const InArgs& a, hipStream_t stream);
void launch_in_fold(const InArgs& a, hipStream_t stream);

// The host-only functions of the header (no device): OMX_NONE or OMX_ERR_INVALID
int in_rule_default(omx_program_inspect_rule* rule);
int in_plan(uint32_t channels, omx_program_inspect_info* info);
int in_summarize(const omx_program_inspect_rule* rule, const omx_program_inspect_record* record, omx_program_inspect_summary* summary);

// The inspector's state: made by inspect_configure, nothing of it exists before.
struct ProgramInspector {
    omx_program_inspect_rule rule{};
    uint32_t channels = 0, n_pairs = 0;
    uint32_t pair_a[OMX_INSPECT_MAX_PAIRS] = {}, pair_b[OMX_INSPECT_MAX_PAIRS] = {};
    std::vector<uint64_t> h_frames;  // the host's mirror of N
    std::vector<uint32_t> h_call;    // [n_streams] host scratch of a call
    DeviceBuffer<uint32_t> call;
    DeviceBuffer<omx_program_inspect_record> records;
    DeviceBuffer<InRuns> runs;       // grown on demand
    DeviceBuffer<long long> sums;    // grown on demand
    BlobStaging staging;
};

}  // namespace omx

// Channel remix of the programme loudness bank (include/omx/program_remix.h states the definition): a static matrix on device PCM.
// program_remix_kernels.hip holds the kernels, program_remix.cpp the presets, the compaction of the matrices, the host side (members
// of ProgramLoudnessBank) and the C ABI.
//
// One call runs, per stream and on the caller's stream: begin (the fresh record) -> main (tiles of frames: the tile's input goes to
// LDS, a thread mixes whole frames by walking the matrix's term lists, the output leaves through LDS; the record's reductions) ->
// finish (the record's dB field).
#pragma once
#include <memory>

#include "../common.hpp"
#include "../../../include/omx/program_remix.h"

namespace omx {

constexpr uint32_t kRmThreads = 256;         // threads per workgroup of the main kernel
constexpr uint32_t kRmStageBytes = 40 * 1024;  // LDS a tile may stage (input and output together): four workgroups share a CU's 160 KiB
constexpr uint32_t kRmMaxTerms = OMX_MAX_CHANNELS * OMX_MAX_CHANNELS;

// Frame strides of the two stagings in dwords (program_remix_kernels.hip says why): odd for the input, channels_out + 1 for 4 and 8
constexpr uint32_t rm_in_stride(uint32_t channels_in) { return channels_in | 1u; }
constexpr uint32_t rm_out_stride(uint32_t channels_out) { return (channels_out == 4 || channels_out == 8) ? channels_out + 1 : channels_out; }
// Frames one thread mixes; a tile is kRmThreads times as many.  A workgroup should move some tens of KiB, so few channels take more
// frames: 8 with up to 2 input channels, 4 with up to 4, else 2; halved while the stagings exceed kRmStageBytes.
constexpr uint32_t rm_frames_per_thread(uint32_t channels_in, uint32_t channels_out) {
    uint32_t fpt = channels_in <= 2 ? 8 : (channels_in <= 4 ? 4 : 2);
    while (fpt > 2 && kRmThreads * fpt * (rm_in_stride(channels_in) + rm_out_stride(channels_out)) * 4 > kRmStageBytes) fpt >>= 1;
    return fpt;
}

// A matrix as the kernel walks it: per output channel the list of its non-zero coefficients, input channels in increasing order.
// The lists lie one behind the other; a workgroup copies the header and the 2 * terms dwords in use to LDS.
struct RmMatrix {
    uint32_t start[OMX_MAX_CHANNELS + 1];  // output o owns terms start[o] .. start[o + 1] - 1
    uint32_t terms;                        // start[channels_out]
    uint32_t _pad[2];
    struct Term {
        uint32_t in;   // input channel
        float coef;
    } term[kRmMaxTerms];
};
constexpr uint32_t kRmHeaderDwords = 12;
static_assert(sizeof(RmMatrix) == (kRmHeaderDwords + 2 * kRmMaxTerms) * 4, "RmMatrix is read as dwords");

// What one call does to one stream: made on the host, uploaded per call.
struct RmStreamCall {
    uint32_t frames;
    uint32_t matrix;
    uint32_t terms;  // of that matrix (the host's copy: the begin kernel and the tiles need not read the table for it)
    uint32_t _pad;
};

struct RmArgs {
    const float* in;   // [n_streams][frames_capacity][channels_in]
    float* out;        // [n_streams][frames_capacity][channels_out]
    uint64_t frames_capacity;
    uint32_t n_streams, channels_in, channels_out;
    float floor_db;
    const RmMatrix* matrices;       // [n_matrices]
    const RmStreamCall* calls;      // [n_streams]
    omx_program_remix_record* records;  // [n_streams]
    uint32_t max_frames;            // the longest stream of the call
};
void launch_rm_begin(const RmArgs& a, hipStream_t stream);
void launch_rm_main(const RmArgs& a, hipStream_t stream);
void launch_rm_finish(const RmArgs& a, hipStream_t stream);

// The host-only functions of the header (no device): OMX_NONE or OMX_ERR_INVALID
int rm_plan(uint32_t channels_in, uint32_t channels_out, omx_program_remix_info* info);
int rm_downmix(const omx_program_downmix_rule* rule, uint32_t channels_in, const uint8_t* positions_in, float* matrix, uint32_t* channels_out,
               uint8_t* positions_out);
int rm_select(uint32_t channels_in, const uint8_t* positions_in, uint32_t channels_out, const uint8_t* positions_out, float* matrix,
              uint32_t* missing_mask);

// The remix's state: made by remix_configure, nothing of it exists before.
struct ProgramRemix {
    uint32_t channels_in = 0, channels_out = 0, n_matrices = 0;
    std::vector<uint32_t> h_terms;  // [n_matrices]
    std::vector<RmStreamCall> h_calls;
    DeviceBuffer<RmMatrix> matrices;
    DeviceBuffer<RmStreamCall> calls;
    DeviceBuffer<omx_program_remix_record> records;
    BlobStaging staging;
};

}  // namespace omx

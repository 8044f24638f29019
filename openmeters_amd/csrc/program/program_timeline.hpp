// Timeline and intervals of the programme loudness bank (include/omx/program_timeline.h): loudness on the 100 ms grid and the record
// of parts of a programme, both from the stored segment energies.  program_timeline_kernels.hip holds the timeline kernels; the
// interval kernel is the result pass itself (program_loudness_kernels.hip) behind a descriptor.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_timeline.h"

namespace omx {

constexpr uint32_t kTlThreads = 256;    // lanes per workgroup of both timeline kernels: one output row per lane in the all-pairs pass
constexpr uint32_t kTlScanItems = 8;    // consecutive blocks per lane and tile of the scan: the tile grid (2048 blocks) is anchored at k = 0
constexpr uint32_t kTlMaxStreams = 65535;  // the all-pairs pass carries the stream in the second grid dimension
constexpr uint32_t kTlTile = 2048;      // gated blocks per LDS tile of the all-pairs pass: 16 KiB, so several workgroups stay resident per CU

struct PlStreamMeta;

struct TlArgs {
    const double* segments;    // [n_streams][capacity]
    uint64_t capacity;
    const PlStreamMeta* meta;  // [n_streams]: segments[s]
    uint64_t first, stride;    // row i is j = first + i * stride
    uint32_t count;            // rows per stream
    uint32_t pitch;            // row length of the three scratch arrays: 1 + the largest j any stream needs
    uint32_t n_streams;        // streams worked on
    uint32_t stream_base;      // first stream worked on (fetch_timeline: that stream alone, n_streams = 1); scratch and rows start there
    float floor_db;
    double absolute_gate;
    double* gated;             // [n_streams][pitch] g[k] where it exceeds the absolute gate, else 0
    double* threshold;         // [n_streams][pitch] 0.1 * mean of the blocks k' <= k above the absolute gate
    uint32_t* above;           // [n_streams][pitch] their count
    omx_program_timeline_row* rows;  // [n_streams][count]
};
void launch_tl_scan(const TlArgs& a, hipStream_t stream);
void launch_tl_rows(const TlArgs& a, hipStream_t stream);

// One interval of measure_intervals, made on the host from h_meta_: where its energies start, how many, what `frames` reads
struct PlIntervalDesc {
    uint64_t offset;  // index into `segments` (stream * capacity + first_segment)
    uint64_t frames;
    uint32_t n, _pad;
};
struct PlResultArgs;
void launch_pl_intervals(const PlResultArgs& a, const PlIntervalDesc* descs, uint32_t n, hipStream_t stream);

}  // namespace omx

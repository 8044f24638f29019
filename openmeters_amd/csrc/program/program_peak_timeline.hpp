// Peak timeline of the programme loudness bank (include/omx/program_peak_timeline.h states the definition): per (stream, segment,
// channel, kind) one 64-bit key, value bits above the complemented frame in the segment — the form of the peak pass's own keys, so a
// larger key is a larger value or the same value at an earlier frame, and a cleared key (0) is a peak of 0.  The timeline form of the
// peak pass (program_peaks_kernels.hip) merges into them with one vector atomic maximum per (segment of the tile, channel, kind) and
// workgroup; program_peak_timeline_kernels.hip reads them: rows, parts (intervals and groups), the clear of a reset, the part gains.
// program_peak_timeline.cpp holds the host side (members of ProgramLoudnessBank) and the C ABI.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_peak_timeline.h"

namespace omx {

struct PlStreamCall;
struct PlStreamMeta;

constexpr uint32_t kPtKinds = 2;          // true peak, sample peak: keys [..][channel][kind]
constexpr uint32_t kPtThreads = 256;      // lanes per workgroup of the row and part kernels
constexpr uint32_t kPtRowsPerBlock = 16;  // rows per workgroup of the row kernel: one lane per (row, channel slot, kind)
constexpr uint32_t kPtMaxStreams = 65535; // the row kernel carries the stream in the second grid dimension

struct PtRowArgs {
    const unsigned long long* keys;  // [n_streams][rows_capacity][channels][2]
    uint64_t rows_capacity;
    const PlStreamMeta* meta;        // [n_streams]: frames[s]
    uint64_t first, stride;          // row i covers the segments [first + i * stride, first + (i + 1) * stride)
    uint32_t count;                  // rows per stream
    uint32_t n_streams, stream_base; // streams worked on (fetch_peak_rows: one); rows start at stream_base
    uint32_t channels, seg;
    omx_program_peak_row* rows;      // [n_streams][count]
};
void launch_pt_rows(const PtRowArgs& a, hipStream_t stream);

// One resolved member and one part (an interval: a part of one member), made on the host from its own counters
struct PtMember {
    uint64_t first, n;  // stored segments [first, first + n) of `stream`
    uint32_t stream, _pad;
};
struct PtPart {
    uint32_t first, count;  // members[first .. first + count)
    uint64_t frames;        // the record's count: the sum over the members
};
struct PtPartArgs {
    const unsigned long long* keys;
    uint64_t rows_capacity;
    const PtMember* members;
    const PtPart* parts;
    omx_program_part_peak* records;  // [n_parts]
    uint32_t channels, seg;
    float floor_db;
};
void launch_pt_parts(const PtPartArgs& a, uint32_t n_parts, hipStream_t stream);

// The stored keys of the streams a call resets, back to zero.  The host lists them from its own counters, rows [0, ceil(frames / L))
// of every reset stream that held frames, cut into runs of at most kPtClearChunk keys: one workgroup per run, so the work is
// proportional to what the reset streams had stored, whatever the size of the bank.
constexpr uint32_t kPtClearChunk = 16384;
struct PtClearItem {
    uint64_t at;       // keys [at, at + n) of the whole array
    uint32_t n, _pad;
};
void launch_pt_clear(unsigned long long* keys, const PtClearItem* items, uint64_t n_items, hipStream_t stream);

// gains[k] = pn_gain(rule, group record k's loudness, part peak k's max_true_peak_db)
void launch_pt_plan(const omx_program_gain_rule& rule, const omx_program_loudness_record* group_records, const omx_program_part_peak* peaks,
                    omx_program_gain_record* gains, uint32_t n_groups, float floor_db, hipStream_t stream);

}  // namespace omx

// Groups of the programme loudness bank (include/omx/program_groups.h): the record of several streams or parts of streams measured
// as one programme.  program_groups_kernels.hip holds the two kernels: the result pass of the stored mode over a member list
// (program_result_device.hpp with a group source) and, for a bank with bounded storage, the sum of the members' histograms followed
// by the histogram result pass (program_histogram_device.hpp).  program_groups.cpp validates against the host's counters and uploads
// the resolved tables per call.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_groups.h"
#include "program_histogram.hpp"

namespace omx {

// One resolved member, made on the host from h_meta_.  The two prefixes are exclusive running sums of the gating / short-term block
// counts over the WHOLE member table, modulo 2^32: a group starting at member f places block k of member m at flat index
// (before[m] - before[f]) + (k - 3), and only that index modulo 256 is ever needed (256 divides 2^32), so one table serves every
// group whatever ranges overlap.
struct PgMember {
    uint64_t offset;             // index into `segments` (stream * capacity + first_segment); bounded mode: not used
    uint32_t n;                  // segments of the member
    uint32_t gating_before;      // gating blocks of the members before it in the table (mod 2^32)
    uint32_t short_term_before;  // short-term blocks likewise
    uint32_t stream;
};
struct PgGroup {
    uint32_t first, count;  // members[first .. first + count)
    uint64_t frames, segments, gating_blocks, short_term_blocks;  // the record's counts: sums over the members
    uint64_t stage_at;      // stored mode: where the group's short-term blocks are staged in the scratch, kPgNoStage: formed anew in every walk
};
constexpr uint64_t kPgNoStage = ~0ull;
// Ten of the result pass's walks visit the short-term blocks (two reductions, eight select passes), and a block is 30 loads and 29
// additions.  A group with at least kPgStageMin of them writes each block once, in the first walk, to bank-owned scratch and reads it
// back in the other nine (the lane that wrote a block is the lane that reads it: no barrier, same bits).  Below that a lane forms at
// most 16 blocks per walk and the pass is a few microseconds of latency either way.  A call stages at most kPgStageMax blocks
// (256 MB of scratch); groups beyond that form their blocks anew, as the per-stream pass does.
constexpr uint64_t kPgStageMin = 4096;
constexpr uint64_t kPgStageMax = 1ull << 25;

struct PlResultArgs;
// a.records: [n_groups]
void launch_pg_stored(const PlResultArgs& a, const PgMember* members, const PgGroup* groups, double* stage, uint32_t n_groups, hipStream_t stream);

struct PgBoundedArgs {
    const omx_program_histogram* hist;  // [n_streams]
    const PhRunning* running;           // [n_streams]
    const PgMember* members;
    const PgGroup* groups;
    omx_program_loudness_record* records;  // [n_groups]
    float floor_db;
};
void launch_pg_bounded(const PgBoundedArgs& a, uint32_t n_groups, hipStream_t stream);

}  // namespace omx

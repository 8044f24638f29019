// Readers of the programme bank's peak timeline (include/omx/program_peak_timeline.h; program_peak_timeline.hpp describes the keys
// the timeline form of the peak pass keeps).  Everything here is integer work on those keys: a maximum with "the earlier frame wins
// among equals" is the larger key, so no result depends on the order it was formed in.
//
// Rows   : one workgroup per (stream, 16 rows), one lane per (row, channel slot, kind).  A lane walks the row's segments in ascending
//          order — at most `stride` 8-byte loads, the sixteen lanes of a row reading one segment's keys side by side — keeps the
//          first largest value, and writes its own two fields of the row; the lane of slot 0 adds frames and valid.
// Parts  : one workgroup per interval or group.  Lane t owns the key column t mod (2 channels) and every (256 / (2 channels))-th
//          segment, so a member's keys are read as contiguous runs of dwordx2; it walks the members in table order and their segments
//          in ascending order with a strict comparison, so it holds (value, first member, first frame) of what it saw.  The lanes of a
//          column meet in LDS, where the smaller member and then the smaller frame win among equal values, and thread 0 writes the
//          record with the dB fields, the maxima and the channel (the lowest on a tie, as pk_fold_kernel).
// Clear  : the keys the reset streams had stored, as contiguous 8-byte stores: one workgroup per run of the host's list.
// Plan   : pn_gain of program_gain_device.hpp, one lane per group.
// Only vector loads and vector stores are used; the kernels need no scratch.
#include "program_gain_device.hpp"
#include "program_loudness.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

__device__ __forceinline__ float key_value(unsigned long long k) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ uint32_t key_frame(unsigned long long k) { return 0xFFFFFFFFu - (uint32_t)k; }

__global__ __launch_bounds__(kPtThreads) void pt_rows_kernel(PtRowArgs a) {
    const uint32_t s = a.stream_base + blockIdx.y, lane = threadIdx.x & 15u;
    const uint32_t i = blockIdx.x * kPtRowsPerBlock + (threadIdx.x >> 4);
    if (i >= a.count) return;
    const uint32_t c = lane >> 1, kind = lane & 1u;
    const uint64_t frames = a.meta[s].frames, L = a.seg;
    const uint64_t n_seg = (frames + L - 1) / L;  // peak segments of the stream, the open one included
    const uint64_t j0 = a.first + (uint64_t)i * a.stride;  // (the host has checked that this fits 64 bits)
    uint64_t j1 = j0 + a.stride;
    if (j1 < j0 || j1 > n_seg) j1 = n_seg;
    float best = 0.0f;
    uint32_t offset = 0;
    if (c < a.channels) {
        const unsigned long long* col = a.keys + ((uint64_t)s * a.rows_capacity * a.channels + c) * kPtKinds + kind;
        for (uint64_t j = j0; j < j1; ++j) {  // (j < n_seg <= rows_capacity)
            const unsigned long long k = col[j * a.channels * kPtKinds];
            if (key_value(k) > best) {  // strictly greater, in time order: the first frame of the maximum
                best = key_value(k);
                offset = (uint32_t)(j - j0) * a.seg + key_frame(k);  // (stride * L fits 32 bits)
            }
        }
    }
    omx_program_peak_row* row = a.rows + (uint64_t)blockIdx.y * a.count + i;
    (kind == 0 ? row->true_peak : row->sample_peak)[c] = best;
    (kind == 0 ? row->true_peak_offset : row->sample_peak_offset)[c] = offset;
    if (lane == 0) {
        const bool valid = j0 < n_seg;
        row->frames = valid ? (uint32_t)(std::min<uint64_t>(frames, j1 * L) - j0 * L) : 0u;
        row->valid = valid ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kPtThreads) void pt_parts_kernel(PtPartArgs a) {
    __shared__ float s_value[kPtThreads];
    __shared__ uint32_t s_member[kPtThreads];
    __shared__ unsigned long long s_frame[kPtThreads];
    const uint32_t tid = threadIdx.x, W = a.channels * kPtKinds, G = kPtThreads / W;
    const uint32_t column = tid % W, g = tid / W;  // lanes with g >= G (256 is no multiple of W) stay idle
    const PtPart part = a.parts[blockIdx.x];
    float best = 0.0f;
    uint32_t member = 0;
    unsigned long long frame = 0;
    if (g < G) {
        for (uint32_t m = 0; m < part.count; ++m) {
            const PtMember mem = a.members[part.first + m];
            const unsigned long long* col = a.keys + ((uint64_t)mem.stream * a.rows_capacity + mem.first) * W + column;
            for (uint64_t j = g; j < mem.n; j += G) {  // (first + n <= the stream's stored segments <= rows_capacity)
                const unsigned long long k = col[j * W];
                if (key_value(k) > best) {
                    best = key_value(k);
                    member = m;
                    frame = (mem.first + j) * a.seg + key_frame(k);
                }
            }
        }
    }
    s_value[tid] = best;
    s_member[tid] = member;
    s_frame[tid] = frame;
    __syncthreads();
    if (tid < W) {  // the lanes of column tid, the same rule with the ties spelled out
        for (uint32_t h = 1; h < G; ++h) {
            const uint32_t at = h * W + tid;
            const float v = s_value[at];
            const bool earlier = s_member[at] < member || (s_member[at] == member && s_frame[at] < frame);
            if (v > best || (v == best && v > 0.0f && earlier)) {
                best = v;
                member = s_member[at];
                frame = s_frame[at];
            }
        }
    }
    __syncthreads();  // (every read of the lanes' slots lies before the columns' results overwrite slots 0 .. W)
    if (tid < W) {
        s_value[tid] = best;
        s_member[tid] = member;
        s_frame[tid] = frame;
    }
    __syncthreads();
    if (tid != 0) return;
    omx_program_part_peak r{};
    r.frames = part.frames;
    r.channels = part.frames != 0 ? a.channels : 0u;
    r.max_true_peak_db = a.floor_db;
    r.max_sample_peak_db = a.floor_db;
    float loudest = 0.0f;
    for (uint32_t c = 0; c < OMX_MAX_CHANNELS; ++c) {
        const bool used = c < a.channels;
        const uint32_t t = c * kPtKinds, m = t + 1;  // columns of channel c
        r.true_peak[c] = used ? s_value[t] : 0.0f;
        r.sample_peak[c] = used ? s_value[m] : 0.0f;
        r.true_peak_member[c] = used ? s_member[t] : 0u;
        r.sample_peak_member[c] = used ? s_member[m] : 0u;
        r.true_peak_frame[c] = used ? s_frame[t] : 0ull;
        r.sample_peak_frame[c] = used ? s_frame[m] : 0ull;
        r.true_peak_db[c] = ps_peak_db(r.true_peak[c], a.floor_db);
        r.sample_peak_db[c] = ps_peak_db(r.sample_peak[c], a.floor_db);
        if (c < r.channels) {
            r.max_true_peak_db = fmaxf(r.max_true_peak_db, r.true_peak_db[c]);
            r.max_sample_peak_db = fmaxf(r.max_sample_peak_db, r.sample_peak_db[c]);
            if (r.true_peak[c] > loudest) {  // lowest channel on a tie
                loudest = r.true_peak[c];
                r.max_true_peak_channel = c;
            }
        }
    }
    a.records[blockIdx.x] = r;
}

__global__ __launch_bounds__(kPtThreads) void pt_clear_kernel(unsigned long long* keys, const PtClearItem* items) {
    const PtClearItem item = items[blockIdx.x];
    unsigned long long* mine = keys + item.at;
    for (uint32_t e = threadIdx.x; e < item.n; e += kPtThreads) mine[e] = 0ull;
}

__global__ __launch_bounds__(64) void pt_plan_kernel(omx_program_gain_rule rule, const omx_program_loudness_record* group_records,
                                                      const omx_program_part_peak* peaks, omx_program_gain_record* gains, uint32_t n,
                                                      float floor_db) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    gains[k] = pn_gain(rule, group_records[k].integrated_lufs, group_records[k].gating_above_relative, peaks[k].max_true_peak_db, floor_db);
}

}  // namespace

void launch_pt_rows(const PtRowArgs& a, hipStream_t stream) {
    const dim3 grid((a.count + kPtRowsPerBlock - 1) / kPtRowsPerBlock, a.n_streams);
    hipLaunchKernelGGL(pt_rows_kernel, grid, dim3(kPtThreads), 0, stream, a);
}
void launch_pt_parts(const PtPartArgs& a, uint32_t n_parts, hipStream_t stream) {
    hipLaunchKernelGGL(pt_parts_kernel, dim3(n_parts), dim3(kPtThreads), 0, stream, a);
}
void launch_pt_clear(unsigned long long* keys, const PtClearItem* items, uint64_t n_items, hipStream_t stream) {
    constexpr uint64_t kSlab = 1ull << 30;  // (workgroups of one launch)
    for (uint64_t base = 0; base < n_items; base += kSlab)
        hipLaunchKernelGGL(pt_clear_kernel, dim3((uint32_t)std::min<uint64_t>(kSlab, n_items - base)), dim3(kPtThreads), 0, stream, keys, items + base);
}
void launch_pt_plan(const omx_program_gain_rule& rule, const omx_program_loudness_record* group_records, const omx_program_part_peak* peaks,
                    omx_program_gain_record* gains, uint32_t n_groups, float floor_db, hipStream_t stream) {
    hipLaunchKernelGGL(pt_plan_kernel, dim3((n_groups + 63) / 64), dim3(64), 0, stream, rule, group_records, peaks, gains, n_groups, floor_db);
}

}  // namespace omx

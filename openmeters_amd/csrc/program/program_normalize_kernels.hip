// Normalisation of the programme loudness bank (include/omx/program_normalize.h).
//
// Plan kernels: one thread per stream, or one wavefront per group (lanes stride the group's member range for the maximum of the
// member streams' true peaks), run pn_gain of program_gain_device.hpp, the function omx_program_gain_evaluate runs on the host.
//
// The pass, out = in * gain, is bandwidth bound: 4 B read and 4 B written per sample, one multiply, one compare, one maximum.
//   grid    : x = tiles of a row (kPnTileFloats floats), y = streams.  Calls are ragged: a tile wholly beyond frames[s] * channels
//             exits at once, before it reads anything but its stream's 16-byte call entry.
//   rows    : a row is frames_capacity * channels floats, so its base is not 16-byte aligned in general (3 channels x 1001 frames).
//             Tile 0 of a row peels up to three leading floats by dword so that the STORE address of the body is 16-byte aligned, and
//             takes the up to three floats behind the last whole vector; every tile then moves its kPnInFlight vectors per thread,
//             all loads issued before the first store.  When the load address of the body is 16-byte aligned too (always for an
//             in-place call) the loads are dwordx4; otherwise each vector is read as four dwords at 4-byte alignment and stored as one
//             aligned dwordx4 (the dword-load form).
//   reduce  : the count of |out| > 1 and the maximum of |out| per thread, six shuffle steps per wavefront, four wavefronts through
//             LDS, then at most ONE atomicAdd (u64) and ONE atomicMax (on the bit pattern of the non-negative float, which orders like
//             the value; fmaxf never lets a NaN in) per workgroup into the stream's apply record, which pn_begin_kernel cleared on the
//             same stream.  A sum of counts and a maximum do not depend on arrival order: the record is deterministic.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_gain_device.hpp"
#include "program_normalize.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void pn_plan_kernel(omx_program_gain_rule rule, const omx_program_loudness_record* records,
                                                      omx_program_gain_record* gains, uint32_t n, float floor_db) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    gains[s] = pn_gain(rule, records[s].integrated_lufs, records[s].gating_above_relative, records[s].max_true_peak_db, floor_db);
}

__global__ __launch_bounds__(64) void pn_plan_groups_kernel(omx_program_gain_rule rule, const omx_program_loudness_record* group_records,
                                                             const omx_program_loudness_record* stream_records, const PgMember* members,
                                                             const PgGroup* groups, omx_program_gain_record* gains, float floor_db) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const PgGroup g = groups[k];
    float peak = floor_db;  // (no stream's figure lies below the floor: an empty group keeps it)
    for (uint32_t i = lane; i < g.count; i += 64) peak = fmaxf(peak, stream_records[members[g.first + i].stream].max_true_peak_db);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) peak = fmaxf(peak, __shfl_xor(peak, d));
    if (lane == 0) gains[k] = pn_gain(rule, group_records[k].integrated_lufs, group_records[k].gating_above_relative, peak, floor_db);
}

__global__ __launch_bounds__(64) void pn_begin_kernel(PnApplyArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const PnStreamCall c = a.calls[s];
    omx_program_apply_record r;
    r.frames = c.n / a.channels;
    r.samples_over = 0;
    r.gain = c.gain_index == OMX_PROGRAM_UNITY_GAIN ? 1.0f : a.gains[c.gain_index].gain;
    r.out_sample_peak = 0.0f;
    r.out_sample_peak_db = a.floor_db;
    r.gain_index = c.gain_index;
    a.applied[s] = r;
}

__global__ __launch_bounds__(64) void pn_finish_kernel(PnApplyArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    a.applied[s].out_sample_peak_db = ps_peak_db(a.applied[s].out_sample_peak, a.floor_db);
}

template <bool WIDE, bool NT>
__device__ __forceinline__ void pn_body(const float* bi, float* bo, uint64_t v0, uint64_t nvec, float gain, PsTally& tally) {
    const bool full = v0 + kPnTileVecs <= nvec;
    v4f x[kPnInFlight];
#pragma unroll
    for (uint32_t k = 0; k < kPnInFlight; ++k) {
        const uint64_t v = v0 + k * kPnThreads + threadIdx.x;
        if (full || v < nvec) {
            const float* p = bi + 4 * v;
            if (WIDE) x[k] = *reinterpret_cast<const v4f*>(p);
            else x[k] = v4f{p[0], p[1], p[2], p[3]};
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kPnInFlight; ++k) {
        const uint64_t v = v0 + k * kPnThreads + threadIdx.x;
        if (full || v < nvec) {
            const v4f y = x[k] * gain;
            tally.take(y.x);
            tally.take(y.y);
            tally.take(y.z);
            tally.take(y.w);
            v4f* q = reinterpret_cast<v4f*>(bo + 4 * v);
            if (NT) __builtin_nontemporal_store(y, q);
            else *q = y;
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(kPnThreads) void pn_tile_kernel(PnApplyArgs a, uint32_t stream_base) {
    const uint32_t s = stream_base + blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const uint64_t n = a.calls[s].n;
    if (n == 0) return;
    const float* in = a.in + (uint64_t)s * a.row;
    float* out = a.out + (uint64_t)s * a.row;
    const uint64_t to_aligned = ps_to_aligned(out);
    const uint32_t peel = (uint32_t)(to_aligned < n ? to_aligned : n);
    const uint64_t nvec = (n - peel) >> 2, v0 = (uint64_t)t * kPnTileVecs;
    if (t != 0 && v0 >= nvec) return;  // (uniform over the workgroup, as the return above: no thread is left at the barrier below)
    const float gain = a.applied[s].gain;
    PsTally tally;
    if (t == 0) {  // the floats outside the aligned body: threads 0 .. 2 the head, threads 4 .. 6 the tail
        const uint32_t tail = (uint32_t)((n - peel) & 3u);
        uint64_t i = n;
        if (tid < peel) i = tid;
        else if (tid >= 4 && tid < 4 + tail) i = peel + 4 * nvec + (tid - 4);
        if (i < n) {
            const float y = in[i] * gain;
            tally.take(y);
            out[i] = y;
        }
    }
    if (v0 < nvec) {
        const float* bi = in + peel;
        if ((reinterpret_cast<uintptr_t>(bi) & 15u) == 0) pn_body<true, NT>(bi, out + peel, v0, nvec, gain, tally);
        else pn_body<false, NT>(bi, out + peel, v0, nvec, gain, tally);
    }
    tally.fold_workgroup<kPnThreads>();
    if (tid == 0) tally.commit(a.applied + s);
}

}  // namespace

void launch_pn_plan(const omx_program_gain_rule& rule, const omx_program_loudness_record* records, omx_program_gain_record* gains, uint32_t n,
                    float floor_db, hipStream_t stream) {
    hipLaunchKernelGGL(pn_plan_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, rule, records, gains, n, floor_db);
}
void launch_pn_plan_groups(const omx_program_gain_rule& rule, const omx_program_loudness_record* group_records,
                           const omx_program_loudness_record* stream_records, const PgMember* members, const PgGroup* groups,
                           omx_program_gain_record* gains, uint32_t n_groups, float floor_db, hipStream_t stream) {
    hipLaunchKernelGGL(pn_plan_groups_kernel, dim3(n_groups), dim3(64), 0, stream, rule, group_records, stream_records, members, groups, gains,
                       floor_db);
}
void launch_pn_begin(const PnApplyArgs& a, hipStream_t stream) {
    ps_launch_per_stream(pn_begin_kernel, a.n_streams, stream, a);
}
void launch_pn_finish(const PnApplyArgs& a, hipStream_t stream) {
    ps_launch_per_stream(pn_finish_kernel, a.n_streams, stream, a);
}
void launch_pn_tiles(const PnApplyArgs& a, uint64_t max_n, bool non_temporal, hipStream_t stream) {
    // tiles of the longest row (a row's body is at most max_n / 4 vectors; tile 0 exists for every row that brings a float)
    const uint64_t tiles = std::max<uint64_t>((max_n / 4 + kPnTileVecs - 1) / kPnTileVecs, 1);
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        const dim3 grid((uint32_t)tiles, count);
        if (non_temporal) hipLaunchKernelGGL(pn_tile_kernel<true>, grid, dim3(kPnThreads), 0, stream, a, base);
        else hipLaunchKernelGGL(pn_tile_kernel<false>, grid, dim3(kPnThreads), 0, stream, a, base);
    });
}

}  // namespace omx

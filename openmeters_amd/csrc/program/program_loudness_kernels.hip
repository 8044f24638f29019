// Programme loudness bank (include/omx/program_loudness.h): segment pass in two evaluation orders, segment commit, result pass
// (gates, gated means, loudness range by radix select, maxima) and the true-peak fold.
//
// Segment pass, one lane per (stream, channel) and work item: the K-weighting recurrence (loudness/processor.rs:153-162) in f64, the
// result rounded to f32 and squared in f64, weighted and summed per 100 ms segment.  PCM is channel-interleaved, so a lane walking its
// own channel would read 4 bytes at a stride of 4 x channels; instead the wavefront loads the tile of its streams (32 frames each)
// with contiguous dword accesses, one tile ahead in registers, and hands it over through a double-buffered LDS tile (one barrier per
// tile; rows padded by one slot group so that the per-lane reads fall on distinct banks).
//   reference order : one work item per stream = the whole call; the filter state and the open segment's sum are carried from call to
//                     call, nothing depends on where the calls were cut -> bit-identical segment energies for any partition.
//   time-parallel   : work items of `chunk` frames.  (A) zero-state end state of every full item as four dot products with host-made
//                     weights, (B) scan of the 4 x 4 zero-input transition over the items, (C) the items again from their true start
//                     states, summing into the (at most two) segments they overlap, (D) fold of those sums in item order.
// Built with -ffp-contract=off: the recurrence rounds like the reference's scalar code; fused multiply-adds are spelled out.
#include "program_result_device.hpp"

namespace omx {
namespace {

constexpr uint32_t TF = kPlTile;
constexpr int kTileLoads = 32;                    // dwords per lane and tile: 64 lanes x 32 = 64 slots x 32 frames
constexpr uint32_t kTileFloats = 64 * TF + 64;    // the largest tile: (64 >> shift) rows of TF * channels + (1 << shift) floats

__device__ __forceinline__ void flush_denormals(double (&f)[4]) {  // level.rs:14-18
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (fabs(f[k]) < 1.0e-30) f[k] = 0.0;
}

enum { PL_REFERENCE = 0, PL_ZERO_STATE = 1, PL_RECOMPUTE = 2 };

template <int MODE>
__global__ __launch_bounds__(64) void pl_segment_kernel(PlArgs a) {
    __shared__ float tile[2][kTileFloats];
    const uint32_t lane = threadIdx.x;
    const uint32_t chp = 1u << a.slot_shift, G = 64u >> a.slot_shift;
    const uint32_t group = blockIdx.x / a.n_chunks, chunk = blockIdx.x % a.n_chunks;
    const uint32_t sl = lane >> a.slot_shift, c = lane & (chp - 1u);
    const uint32_t s = group * G + sl;
    const bool live = s < a.n_streams && c < a.channels;
    const uint32_t slot = (s < a.n_streams ? s : 0u) * kPlSlots + (c < kPlSlots ? c : 0u);
    PlStreamCall call{};
    if (s < a.n_streams) call = a.calls[s];
    const uint64_t start = (uint64_t)chunk * a.chunk;
    // frames of this work item
    uint32_t nf = call.frames > start ? (uint32_t)min((uint64_t)a.chunk, (uint64_t)call.frames - start) : 0u;
    if constexpr (MODE == PL_ZERO_STATE) nf = (start + a.chunk < call.frames) ? a.chunk : 0u;  // full items that somebody starts behind
    uint32_t max_nf = nf;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) max_nf = max(max_nf, (uint32_t)__shfl_xor((int)max_nf, d));
    if (max_nf == 0) return;  // (uniform)

    // ---- the tile map of this lane: dword idx = lane + 64 r of the tile [G rows][TF frames][channels] (constant over the tiles)
    const uint32_t row_len = TF * a.channels, stride = row_len + chp;
    const float* src[kTileLoads];
    uint32_t lim[kTileLoads], dst[kTileLoads];
#pragma unroll
    for (int r = 0; r < kTileLoads; ++r) {
        const uint32_t idx = lane + 64u * (uint32_t)r;
        const uint32_t g = idx / row_len, i = idx - g * row_len, fi = i / a.channels;
        const uint32_t gs = group * G + g;
        const bool ok = g < G && gs < a.n_streams;
        const uint32_t nf_g = (uint32_t)__shfl((int)nf, (int)((g < G ? g : 0u) << a.slot_shift));
        lim[r] = (ok && nf_g > fi) ? nf_g - fi : 0u;  // the load of tile frame t0 is inside the item while t0 < lim
        src[r] = a.pcm + ((uint64_t)(ok ? gs : 0u) * a.frames_capacity + start) * a.channels + (ok ? i : 0u);
        dst[r] = (g < G ? g : 0u) * stride + i;
    }
    float pre[kTileLoads];
    auto issue = [&](uint32_t t0) {
#pragma unroll
        for (int r = 0; r < kTileLoads; ++r) pre[r] = t0 < lim[r] ? src[r][(uint64_t)t0 * a.channels] : 0.0f;
    };
    auto stage = [&](float* buf) {
#pragma unroll
        for (int r = 0; r < kTileLoads; ++r)
            if (lane + 64u * (uint32_t)r < G * row_len) buf[dst[r]] = pre[r];
    };

    // ---- lane state
    double w = 0.0;
#pragma unroll
    for (int i = 0; i < OMX_MAX_CHANNELS; ++i)
        if (c == (uint32_t)i) w = a.weights[i];
    double f[4] = {0.0, 0.0, 0.0, 0.0}, acc = 0.0, p0 = 0.0;
    bool crossed = false;
    uint32_t left = a.seg, emitted = 0;
    if constexpr (MODE != PL_ZERO_STATE) {
        if (live) {
            const double* st = MODE == PL_REFERENCE ? a.state + (uint64_t)slot * 4 : a.starts + ((uint64_t)slot * a.n_chunks + chunk) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = st[k];
            if constexpr (MODE == PL_REFERENCE) acc = a.part[slot];
        }
        left = a.seg - (uint32_t)(((uint64_t)call.phase + start) % a.seg);
    }
    const uint32_t lds_at = sl * stride + c;

    issue(0);
    stage(tile[0]);
    __syncthreads();
    const uint32_t n_tiles = (max_nf + TF - 1) / TF;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t t0 = t * TF;
        const bool more = t + 1 < n_tiles;  // (uniform)
        if (more) issue(t0 + TF);
        const float* buf = tile[t & 1u];
        if constexpr (MODE == PL_ZERO_STATE) {
            // frames beyond the item were staged as zeros; the weights are the same for every lane (scalar loads), eight frames at a
            // time: a whole tile of them (256 scalar registers) does not fit the scalar file
#pragma unroll 1
            for (uint32_t k0 = 0; k0 < TF; k0 += 8) {
                const double* wz = a.zs_weights + (uint64_t)(t0 + k0) * 4;
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const double xd = (double)buf[lds_at + (k0 + k) * a.channels];
#pragma unroll
                    for (int q = 0; q < 4; ++q) f[q] = fma(wz[k * 4 + q], xd, f[q]);
                }
            }
        } else {
            float x[TF];
#pragma unroll
            for (uint32_t k = 0; k < TF; ++k) x[k] = buf[lds_at + k * a.channels];
            const uint32_t n_here = (live && nf > t0) ? min(nf - t0, TF) : 0u;
            auto sample = [&](float xv) {  // k_weighted (:153-162), squared and weighted
                const double xd = (double)xv;
                const double y = a.b[0] * xd + f[0];
                f[0] = a.b[1] * xd + f[1] - a.a[1] * y;
                f[1] = a.b[2] * xd + f[2] - a.a[2] * y;
                f[2] = a.b[3] * xd + f[3] - a.a[3] * y;
                f[3] = a.b[4] * xd - a.a[4] * y;
                const double filtered = (double)(float)y;  // rounded to f32 before squaring (:161, :276-277)
                double value = filtered * filtered;
                value = isfinite(value) ? value : 0.0;     // WindowedMeans::push (dsp.rs:325)
                acc += w * value;
            };
            if (n_here == TF && left > TF) {  // the whole tile lies inside one segment: straight-line code (same operations, same order)
#pragma unroll
                for (uint32_t k = 0; k < TF; ++k) sample(x[k]);
                left -= TF;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < TF; ++k) {
                    if (k < n_here) {
                        sample(x[k]);
                        if (--left == 0) {  // the segment is complete
                            if constexpr (MODE == PL_REFERENCE) {
                                if (emitted < a.max_new) a.chan_sums[(uint64_t)slot * a.max_new + emitted] = acc;
                                ++emitted;
                                flush_denormals(f);  // (:281-285 for a host that delivers 100 ms blocks; on the segment grid, not the call grid)
                            } else {
                                p0 = acc;
                                crossed = true;
                            }
                            acc = 0.0;
                            left = a.seg;
                        }
                    }
                }
            }
        }
        if (more) stage(tile[(t + 1) & 1u]);
        __syncthreads();
    }

    if (!live) return;
    if constexpr (MODE == PL_REFERENCE) {
        a.part[slot] = acc;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.state[(uint64_t)slot * 4 + k] = f[k];
    } else if constexpr (MODE == PL_ZERO_STATE) {
        if (nf != 0) {
            double* z = a.starts + ((uint64_t)slot * a.n_chunks + chunk + 1) * 4;  // (chunk + 1 < n_chunks: the item is not the stream's last)
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = f[k];
        }
    } else {
        if (nf != 0) {
            double* p = a.partials + ((uint64_t)slot * a.n_chunks + chunk) * 2;
            p[0] = crossed ? p0 : acc;
            p[1] = crossed ? acc : 0.0;
            if (start + nf == call.frames) {  // the stream's last item leaves the carried state
                flush_denormals(f);
#pragma unroll
                for (int k = 0; k < 4; ++k) a.state[(uint64_t)slot * 4 + k] = f[k];
            }
        }
    }
}

// (B) start states of the work items: s[0] = carried state, s[j + 1] = T s[j] + z[j].  T = A^chunk has entries far larger than its
// action on a state (loudness.cpp: the companion form is far from normal; largest entry 4e2 at 48 kHz, 2.9e5 at 192 kHz, 2.1e6 at
// 384 kHz), so the host hands it over as high + low parts and the scan carries the state as a double-double pair: the products T s
// cancel to the state's own size, and a sum of them in plain f64 leaves 1e-16 x |T| x |s| in the start state — in a CPU model 6e-3 dB
// at 192 kHz and whole decibels at 384 kHz on a programme with a DC offset or rumble, where the state is large and the output small.  The zero-state
// terms z[j] (pass A) stay f64 sums: their error is not amplified.  Each start state is rounded to f64 once, as the sequential
// recurrence rounds its state at every sample.
struct DD {
    double h, l;
};
__device__ __forceinline__ DD dd_madd(DD acc, double th, double tl, DD u) {  // acc + (th + tl) * (u.h + u.l)
    const double p = th * u.h;
    const double pe = fma(th, u.h, -p) + (th * u.l + tl * u.h);
    const double s = acc.h + p, bb = s - acc.h;
    const double e = ((acc.h - (s - bb)) + (p - bb)) + (acc.l + pe);
    const double h = s + e;
    return {h, e - (h - s)};
}
__global__ __launch_bounds__(64) void pl_scan_kernel(PlArgs a) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t s = gid / kPlSlots, c = gid % kPlSlots;
    if (s >= a.n_streams || c >= a.channels) return;
    const uint32_t frames = a.calls[s].frames;
    if (frames == 0) return;
    const uint32_t items = (frames + a.chunk - 1) / a.chunk;
    DD st[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = {a.state[(uint64_t)gid * 4 + k], 0.0};
    double* out = a.starts + (uint64_t)gid * a.n_chunks * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = st[k].h;
    for (uint32_t j = 0; j + 1 < items; ++j) {
        DD nx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nx[i] = {out[(uint64_t)(j + 1) * 4 + i], 0.0};  // z[j] of pass A
#pragma unroll
            for (int k = 0; k < 4; ++k) nx[i] = dd_madd(nx[i], a.transition[i * 4 + k], a.transition[16 + i * 4 + k], st[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            st[k] = nx[k];
            out[(uint64_t)(j + 1) * 4 + k] = nx[k].h;
        }
    }
}

// (D) the items' sums, in item order, into the sums of the segments that complete in this call and the open segment's carry
__global__ __launch_bounds__(64) void pl_fold_kernel(PlArgs a) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t s = gid / kPlSlots, c = gid % kPlSlots;
    if (s >= a.n_streams || c >= a.channels) return;
    const PlStreamCall call = a.calls[s];
    if (call.frames == 0) return;
    const uint32_t items = (call.frames + a.chunk - 1) / a.chunk;
    double acc = a.part[gid];
    uint32_t left = a.seg - call.phase, emitted = 0;
    const double* p = a.partials + (uint64_t)gid * a.n_chunks * 2;
    for (uint32_t j = 0; j < items; ++j) {
        const uint32_t nf = min(a.chunk, call.frames - j * a.chunk);
        acc += p[(uint64_t)j * 2];
        if (nf >= left) {
            if (emitted < a.max_new) a.chan_sums[(uint64_t)gid * a.max_new + emitted] = acc;
            ++emitted;
            acc = p[(uint64_t)j * 2 + 1];
            left = a.seg - (nf - left);
        } else {
            left -= nf;
        }
    }
    a.part[gid] = acc;
}

// e[seg_base + i] = sum over the channels (in order) of the weighted sums / segment length
__global__ __launch_bounds__(256) void pl_commit_kernel(PlArgs a) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t s = (uint32_t)(gid / a.max_new), i = (uint32_t)(gid % a.max_new);
    if (s >= a.n_streams) return;
    const PlStreamCall call = a.calls[s];
    if (i >= call.n_new || call.seg_base + i >= a.capacity) return;
    double e = 0.0;
    for (uint32_t c = 0; c < a.channels; ++c) e += a.chan_sums[((uint64_t)s * kPlSlots + c) * a.max_new + i];
    a.segments[(uint64_t)s * a.capacity + call.seg_base + i] = e / (double)a.seg;
}

__global__ __launch_bounds__(64) void pl_reset_kernel(PlArgs a, float* tp_max, float floor_db) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t s = gid / kPlSlots, c = gid % kPlSlots;
    if (s >= a.n_streams || a.calls[s].reset == 0) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[(uint64_t)gid * 4 + k] = 0.0;
    a.part[gid] = 0.0;
    if (c == 0) tp_max[s] = floor_db;
}

__global__ __launch_bounds__(64) void pl_true_peak_fold_kernel(const omx_loudness_snapshot* snapshots, uint64_t n_blocks, const uint32_t* d_n_blocks,
                                                               uint32_t n_streams, float* tp_max) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    const uint64_t n = d_n_blocks ? min((uint64_t)d_n_blocks[s], n_blocks) : n_blocks;
    float m = tp_max[s];
    for (uint64_t k = 0; k < n; ++k) {
        const omx_loudness_snapshot& snap = snapshots[(uint64_t)s * n_blocks + k];
        const uint32_t ch = min(snap.channel_count, (uint32_t)OMX_MAX_CHANNELS);
        for (uint32_t c = 0; c < ch; ++c) m = fmaxf(m, snap.true_peak_db[c]);
    }
    tp_max[s] = m;
}

// ---- result pass: one workgroup per stream (or per interval of a stream: include/omx/program_timeline.h) over stored segment energies.
// The pass itself (block expressions, reductions, radix select, record writer) is program_result_device.hpp, shared with the group kernel.
constexpr uint32_t RT = kPlResultThreads;

__global__ __launch_bounds__(RT) void pl_result_kernel(PlResultArgs a) {
    const uint32_t s = blockIdx.x;
    const PlStreamMeta meta = a.meta[s];
    const PlSpanSource src{a.segments + (uint64_t)s * a.capacity, (uint32_t)min((uint64_t)meta.segments, a.capacity)};
    const PlRecordTail tail{meta.frames, meta.overflow, a.tp_max + s, a.peaks ? &a.peaks[s].max_true_peak_db : nullptr};
    pl_result_pass(src, tail, a.absolute_gate, a.floor_db, a.records + s);
}

// One workgroup per interval: the same pass on e[first .. first + count) of a stream
__global__ __launch_bounds__(RT) void pl_interval_kernel(PlResultArgs a, const PlIntervalDesc* descs) {
    const PlIntervalDesc in = descs[blockIdx.x];
    const PlSpanSource src{a.segments + in.offset, in.n};
    const PlRecordTail tail{in.frames, 0u, nullptr, nullptr};
    pl_result_pass(src, tail, a.absolute_gate, a.floor_db, a.records + blockIdx.x);
}

uint32_t segment_grid(const PlArgs& a) {
    const uint64_t G = 64u >> a.slot_shift, groups = (a.n_streams + G - 1) / G, blocks = groups * a.n_chunks;
    if (blocks > 0x7FFFFFFFull) unsupported("programme loudness: call too long for one launch");
    return (uint32_t)blocks;
}
uint32_t slot_grid(const PlArgs& a) { return (a.n_streams * kPlSlots + 63) / 64; }

}  // namespace

void launch_pl_reset(const PlArgs& a, float* tp_max, float floor_db, hipStream_t stream) {
    hipLaunchKernelGGL(pl_reset_kernel, dim3(slot_grid(a)), dim3(64), 0, stream, a, tp_max, floor_db);
}
void launch_pl_reference_order(const PlArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pl_segment_kernel<PL_REFERENCE>, dim3(segment_grid(a)), dim3(64), 0, stream, a);
}
void launch_pl_time_parallel(const PlArgs& a, hipStream_t stream) {
    const uint32_t grid = segment_grid(a);
    if (a.n_chunks > 1) hipLaunchKernelGGL(pl_segment_kernel<PL_ZERO_STATE>, dim3(grid), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(pl_scan_kernel, dim3(slot_grid(a)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(pl_segment_kernel<PL_RECOMPUTE>, dim3(grid), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(pl_fold_kernel, dim3(slot_grid(a)), dim3(64), 0, stream, a);
}
void launch_pl_commit(const PlArgs& a, hipStream_t stream) {
    if (a.max_new == 0) return;
    const uint64_t lanes = (uint64_t)a.n_streams * a.max_new;
    hipLaunchKernelGGL(pl_commit_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, a);
}
void launch_pl_results(const PlResultArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pl_result_kernel, dim3(a.n_streams), dim3(RT), 0, stream, a);
}
void launch_pl_intervals(const PlResultArgs& a, const PlIntervalDesc* descs, uint32_t n, hipStream_t stream) {  // a.records: [n]
    hipLaunchKernelGGL(pl_interval_kernel, dim3(n), dim3(RT), 0, stream, a, descs);
}
void launch_pl_true_peak_fold(const omx_loudness_snapshot* snapshots, uint64_t n_blocks, const uint32_t* d_n_blocks, uint32_t n_streams,
                              float* tp_max, hipStream_t stream) {
    hipLaunchKernelGGL(pl_true_peak_fold_kernel, dim3((n_streams + 63) / 64), dim3(64), 0, stream, snapshots, n_blocks, d_n_blocks, n_streams,
                       tp_max);
}

}  // namespace omx

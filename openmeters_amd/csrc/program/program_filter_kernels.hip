// Filter stage of the programme loudness bank (include/omx/program_filter.h): the pass in two evaluation orders, the scan of the
// time-parallel form, the fold of the record and the reset.
//
// The pass, one lane per (stream, channel) and work item: up to two biquad sections in f64 transposed direct form II, the result
// rounded to f32.  PCM is channel-interleaved, so a lane walking its own channel would touch 4 bytes at a stride of 4 x channels;
// instead the wavefront loads the tile of its streams (32 frames each) with contiguous dword accesses, one tile ahead in registers,
// and hands it over through a double-buffered LDS tile (rows padded by one slot group so that the per-lane accesses fall on distinct
// banks).  A lane puts its outputs back into its own column of the tile it read, and the wavefront stores the tile as whole rows, four
// dwords per lane: 16 bytes where the row's alignment allows, single dwords at a row's ragged end and under an odd base.
//   reference order : one work item per stream = the whole call; the state is carried from call to call, nothing depends on where
//                     the calls were cut -> bit-identical output for any partition.
//   time-parallel   : work items of `chunk` frames.  (A) zero-state end state of every full item as four dot products with the
//                     host-made weights of the lane's filter, (B) scan of the 4 x 4 zero-input transition over the items, the state
//                     a double-double pair, (C) the items again from their true start states, writing the output, (D) fold.
//                     An in-place call is safe: pass C reads and writes only its own item, and pass A has finished by the kernel
//                     boundary.  A lane on bypass takes no part in A and B.
// Every work item leaves what it saw of its lane's output (samples over full scale, samples that are not finite, the peak) in a table;
// the fold, one wavefront per stream, makes the record from it: integer sums and a maximum, so the record does not depend on the form.
// Built with -ffp-contract=off: the recurrence rounds like the definition's scalar code; the fused multiply-adds of pass A and of
// the scan are spelled out.
#include "program_filter.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

constexpr uint32_t TF = kFlTile;
constexpr int kTileLoads = 32;                    // dwords per lane and tile: 64 lanes x 32 = 64 slots x 32 frames
constexpr int kTileStores = kTileLoads / 4;       // groups of four dwords per lane and tile
constexpr uint32_t kTileFloats = 64 * TF + 64;    // the largest tile: (64 >> shift) rows of TF * channels + (1 << shift) floats

enum { FL_REFERENCE = 0, FL_ZERO_STATE = 1, FL_RECOMPUTE = 2 };

template <int MODE>
__global__ __launch_bounds__(64) void fl_pass_kernel(FlArgs a) {
    __shared__ float tile[2][kTileFloats];
    const uint32_t lane = threadIdx.x;
    const uint32_t chp = 1u << a.slot_shift, G = 64u >> a.slot_shift;
    const uint32_t group = blockIdx.x / a.n_chunks, chunk = blockIdx.x % a.n_chunks;
    const uint32_t sl = lane >> a.slot_shift, c = lane & (chp - 1u);
    const uint32_t s = group * G + sl;
    const bool live = s < a.n_streams && c < a.channels;
    const uint32_t slot = (s < a.n_streams ? s : 0u) * kFlSlots + (c < kFlSlots ? c : 0u);
    FlStreamCall call{};
    if (s < a.n_streams) call = a.calls[s];
    const uint64_t start = (uint64_t)chunk * a.chunk;
    // frames of this work item
    uint32_t nf = call.frames > start ? (uint32_t)min((uint64_t)a.chunk, (uint64_t)call.frames - start) : 0u;
    if constexpr (MODE == FL_ZERO_STATE) nf = (start + a.chunk < call.frames) ? a.chunk : 0u;  // full items that somebody starts behind
    uint32_t max_nf = nf;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) max_nf = max(max_nf, (uint32_t)__shfl_xor((int)max_nf, d));
    if (max_nf == 0) return;  // (uniform)

    // ---- the lane's filter
    const uint32_t filt = live ? a.lane_filter[slot] : OMX_FILTER_BYPASS;
    const bool bypass = filt == OMX_FILTER_BYPASS;
    uint32_t low_filt = filt;  // the lowest table index of the wavefront (bypass is the largest value)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) low_filt = min(low_filt, (uint32_t)__shfl_xor((int)low_filt, d));
    low_filt = (uint32_t)__builtin_amdgcn_readfirstlane((int)low_filt);
    if constexpr (MODE == FL_ZERO_STATE) {
        if (low_filt == OMX_FILTER_BYPASS) return;  // (uniform) nobody filters
    }

    // ---- the tile map of this lane: dword idx = lane + 64 r of the tile [G rows][TF frames][channels] (constant over the tiles)
    const uint32_t row_len = TF * a.channels, stride = row_len + chp;
    uint64_t src[kTileLoads];
    uint32_t lim[kTileLoads], dst[kTileLoads];
#pragma unroll
    for (int r = 0; r < kTileLoads; ++r) {
        const uint32_t idx = lane + 64u * (uint32_t)r;
        const uint32_t g = idx / row_len, i = idx - g * row_len, fi = i / a.channels;
        const uint32_t gs = group * G + g;
        const bool ok = g < G && gs < a.n_streams;
        const uint32_t nf_g = (uint32_t)__shfl((int)nf, (int)((g < G ? g : 0u) << a.slot_shift));
        lim[r] = (ok && nf_g > fi) ? nf_g - fi : 0u;  // the load of tile frame t0 is inside the item while t0 < lim
        src[r] = ((uint64_t)(ok ? gs : 0u) * a.frames_capacity + start) * a.channels + (ok ? i : 0u);
        dst[r] = (g < G ? g : 0u) * stride + i;
    }
    float pre[kTileLoads];
    auto issue = [&](uint32_t t0) {
#pragma unroll
        for (int r = 0; r < kTileLoads; ++r) pre[r] = t0 < lim[r] ? a.in[src[r] + (uint64_t)t0 * a.channels] : 0.0f;
    };
    auto stage = [&](float* buf) {
#pragma unroll
        for (int r = 0; r < kTileLoads; ++r)
            if (lane + 64u * (uint32_t)r < G * row_len) buf[dst[r]] = pre[r];
    };
    const uint32_t lds_at = sl * stride + c;

    if constexpr (MODE == FL_ZERO_STATE) {
        // ---- (A) frames beyond the item were staged as zeros.  With one filter in the wavefront the weights are the same for every
        // lane (scalar loads), eight frames at a time: a whole tile of them does not fit the scalar file.
        bool same = bypass || filt == low_filt;
        same = __all(same);
        double f[4] = {0.0, 0.0, 0.0, 0.0};
        issue(0);
        stage(tile[0]);
        __syncthreads();
        const uint32_t n_tiles = (max_nf + TF - 1) / TF;
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const uint32_t t0 = t * TF;
            const bool more = t + 1 < n_tiles;  // (uniform)
            if (more) issue(t0 + TF);
            const float* buf = tile[t & 1u];
            auto dots = [&](const double* weights) {
#pragma unroll 1
                for (uint32_t k0 = 0; k0 < TF; k0 += 8) {
                    const double* wz = weights + (uint64_t)(t0 + k0) * 4;
#pragma unroll
                    for (uint32_t k = 0; k < 8; ++k) {
                        const double xd = (double)buf[lds_at + (k0 + k) * a.channels];
#pragma unroll
                        for (int q = 0; q < 4; ++q) f[q] = fma(wz[k * 4 + q], xd, f[q]);
                    }
                }
            };
            if (same) dots(a.zs_weights + (uint64_t)low_filt * a.weights_stride);
            else dots(a.zs_weights + (uint64_t)(bypass ? low_filt : filt) * a.weights_stride);
            if (more) stage(tile[(t + 1) & 1u]);
            __syncthreads();
        }
        if (live && !bypass && nf != 0) {
            double* z = a.starts + ((uint64_t)slot * a.n_chunks + chunk + 1) * 4;  // (chunk + 1 < n_chunks: the item is not the stream's last)
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = f[k];
        }
        return;
    } else {
        // ---- the store map: group idx = lane + 64 r of four dwords each, of the same tile (a row is a multiple of four dwords long)
        uint64_t to[kTileStores];
        uint32_t from[kTileStores], row_nf[kTileStores], at[kTileStores];
#pragma unroll
        for (int r = 0; r < kTileStores; ++r) {
            const uint32_t idx = (lane + 64u * (uint32_t)r) * 4u;
            const uint32_t g = idx / row_len, i = idx - g * row_len;
            const uint32_t gs = group * G + g;
            const bool ok = g < G && gs < a.n_streams;
            const uint32_t nf_g = (uint32_t)__shfl((int)nf, (int)((g < G ? g : 0u) << a.slot_shift));
            row_nf[r] = ok ? nf_g : 0u;
            at[r] = i;
            to[r] = ((uint64_t)(ok ? gs : 0u) * a.frames_capacity + start) * a.channels + (ok ? i : 0u);
            from[r] = (g < G ? g : 0u) * stride + i;
        }
        const bool out_aligned = (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0;

        // ---- lane state
        double c0[5] = {1.0, 0.0, 0.0, 0.0, 0.0}, c1[5] = {1.0, 0.0, 0.0, 0.0, 0.0};
        bool two = false;
        if (!bypass) {
            const omx_program_filter& fl = a.filters[filt];
            two = fl.n_sections == 2;
            const omx_program_filter_section& s0 = fl.section[0];
            c0[0] = s0.b0, c0[1] = s0.b1, c0[2] = s0.b2, c0[3] = s0.a1, c0[4] = s0.a2;
            if (two) {
                const omx_program_filter_section& s1 = fl.section[1];
                c1[0] = s1.b0, c1[1] = s1.b1, c1[2] = s1.b2, c1[3] = s1.a1, c1[4] = s1.a2;
            }
        }
        const bool any_two = __any(two);  // (uniform)
        double f[4] = {0.0, 0.0, 0.0, 0.0};
        if (live && !bypass) {
            const double* st = MODE == FL_REFERENCE ? a.state + (uint64_t)slot * 4 : a.starts + ((uint64_t)slot * a.n_chunks + chunk) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = st[k];
        }
        uint32_t over = 0, nonfinite = 0;
        float peak = 0.0f;

        issue(0);
        stage(tile[0]);
        __syncthreads();
        const uint32_t n_tiles = (max_nf + TF - 1) / TF;
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const uint32_t t0 = t * TF;
            const bool more = t + 1 < n_tiles;  // (uniform)
            if (more) issue(t0 + TF);
            float* buf = tile[t & 1u];
            float x[TF];
#pragma unroll
            for (uint32_t k = 0; k < TF; ++k) x[k] = buf[lds_at + k * a.channels];
            const uint32_t n_here = (live && nf > t0) ? min(nf - t0, TF) : 0u;
            auto sample = [&](float& xv) {  // the definition; a lane on bypass keeps its bits
                const double v = (double)xv;
                double y = c0[0] * v + f[0];
                f[0] = (c0[1] * v - c0[3] * y) + f[1];
                f[1] = c0[2] * v - c0[4] * y;
                if (any_two) {
                    const double y2 = c1[0] * y + f[2];
                    const double n2 = (c1[1] * y - c1[3] * y2) + f[3];
                    const double n3 = c1[2] * y - c1[4] * y2;
                    f[2] = two ? n2 : f[2];
                    f[3] = two ? n3 : f[3];
                    y = two ? y2 : y;
                }
                const float yf = (float)y;
                xv = bypass ? xv : yf;
                const float m = fabsf(xv);
                over += m > 1.0f ? 1u : 0u;             // false for NaN, true for infinity
                nonfinite += m < INFINITY ? 0u : 1u;     // NaN and infinity
                peak = fmaxf(peak, m);                   // a NaN operand is ignored
            };
            if (n_here == TF) {  // straight-line code (same operations, same order)
#pragma unroll
                for (uint32_t k = 0; k < TF; ++k) sample(x[k]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < TF; ++k)
                    if (k < n_here) sample(x[k]);
            }
            // the outputs into the lane's own column (a slot behind the channels shares its addresses with the stream's channel 0)
            if (live) {
#pragma unroll
                for (uint32_t k = 0; k < TF; ++k) buf[lds_at + k * a.channels] = x[k];
            }
            if (more) stage(tile[(t + 1) & 1u]);
            __syncthreads();
            // ---- the tile leaves as whole rows
#pragma unroll
            for (int r = 0; r < kTileStores; ++r) {
                const uint32_t frames_left = row_nf[r] > t0 ? min(row_nf[r] - t0, TF) : 0u;
                const uint32_t floats_left = frames_left * a.channels;
                if (at[r] >= floats_left) continue;
                const uint32_t n = min(floats_left - at[r], 4u);
                const uint64_t o = to[r] + (uint64_t)t0 * a.channels;
                const float v0 = buf[from[r]], v1 = buf[from[r] + 1], v2 = buf[from[r] + 2], v3 = buf[from[r] + 3];
                if (n == 4 && out_aligned && (o & 3u) == 0) {
                    *reinterpret_cast<float4*>(a.out + o) = make_float4(v0, v1, v2, v3);
                } else {
                    a.out[o] = v0;
                    if (n > 1) a.out[o + 1] = v1;
                    if (n > 2) a.out[o + 2] = v2;
                    if (n > 3) a.out[o + 3] = v3;
                }
            }
            __syncthreads();
        }

        if (!live || nf == 0) return;
        a.partials[(uint64_t)slot * a.n_chunks + chunk] = FlPartial{over, nonfinite, peak, 0u};
        if (!bypass && start + nf == call.frames) {  // the stream's last item leaves the carried state
#pragma unroll
            for (int k = 0; k < 4; ++k) a.state[(uint64_t)slot * 4 + k] = f[k];
        }
    }
}

// (B) start states of the work items: s[0] = carried state, s[j + 1] = T s[j] + z[j].  The entries of T = A^chunk are larger than
// its action on a state (program_filter_plan.hpp has the figures), so the host hands it over as high + low parts and the scan carries
// the state as a double-double pair, as the loudness pass does (program_loudness_kernels.hip says why).  The zero-state terms z[j]
// (pass A) stay f64 sums.  Each start state is rounded to f64 once.
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
__global__ __launch_bounds__(64) void fl_scan_kernel(FlArgs a) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t s = gid / kFlSlots, c = gid % kFlSlots;
    if (s >= a.n_streams || c >= a.channels) return;
    const uint32_t filt = a.lane_filter[gid];
    if (filt == OMX_FILTER_BYPASS) return;
    const uint32_t frames = a.calls[s].frames;
    if (frames == 0) return;
    const uint32_t items = (frames + a.chunk - 1) / a.chunk;
    const double* T = a.transition + (uint64_t)filt * 32;
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
            for (int k = 0; k < 4; ++k) nx[i] = dd_madd(nx[i], T[i * 4 + k], T[16 + i * 4 + k], st[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            st[k] = nx[k];
            out[(uint64_t)(j + 1) * 4 + k] = nx[k].h;
        }
    }
}

// (D) one wavefront per stream: the items' tallies of every channel into the stream's record
__global__ __launch_bounds__(64) void fl_fold_kernel(FlArgs a) {
    const uint32_t s = blockIdx.x;
    const FlStreamCall call = a.calls[s];
    const uint32_t items = call.frames ? (call.frames + a.chunk - 1) / a.chunk : 0u;
    unsigned long long over = 0, nonfinite = 0;
    float peak = 0.0f;
    for (uint32_t c = 0; c < a.channels; ++c) {
        const FlPartial* p = a.partials + ((uint64_t)s * kFlSlots + c) * a.n_chunks;
        for (uint32_t j = threadIdx.x; j < items; j += 64) {
            const FlPartial v = p[j];
            over += v.over;
            nonfinite += v.nonfinite;
            peak = fmaxf(peak, v.peak);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        over += __shfl_xor(over, d);
        nonfinite += __shfl_xor(nonfinite, d);
        peak = fmaxf(peak, __shfl_xor(peak, d));
    }
    if (threadIdx.x != 0) return;
    omx_program_filter_record r{};
    r.frames = call.frames;
    r.frames_total = call.frames_total;
    r.samples_over = over;
    r.samples_nonfinite = nonfinite;
    r.out_sample_peak = peak;
    r.out_sample_peak_db = ps_peak_db(peak, a.floor_db);
    r.form = call.frames ? a.form : 0u;
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void fl_reset_kernel(FlArgs a) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t s = gid / kFlSlots, c = gid % kFlSlots;
    if (s >= a.n_streams || a.calls[s].frames == 0) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[(uint64_t)gid * 4 + k] = 0.0;
    if (c != 0) return;
    omx_program_filter_record r{};
    r.out_sample_peak_db = ps_peak_db(0.0f, a.floor_db);
    a.records[s] = r;
}

uint32_t pass_grid(const FlArgs& a) {
    const uint64_t G = 64u >> a.slot_shift, groups = (a.n_streams + G - 1) / G, blocks = groups * a.n_chunks;
    if (blocks > 0x7FFFFFFFull) unsupported("programme filter: call too long for one launch");
    return (uint32_t)blocks;
}
uint32_t slot_grid(const FlArgs& a) { return (a.n_streams * kFlSlots + 63) / 64; }

}  // namespace

void launch_fl_reset(const FlArgs& a, hipStream_t stream) { hipLaunchKernelGGL(fl_reset_kernel, dim3(slot_grid(a)), dim3(64), 0, stream, a); }
void launch_fl_reference_order(const FlArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(fl_pass_kernel<FL_REFERENCE>, dim3(pass_grid(a)), dim3(64), 0, stream, a);
}
void launch_fl_time_parallel(const FlArgs& a, hipStream_t stream) {
    const uint32_t grid = pass_grid(a);
    if (a.n_chunks > 1) hipLaunchKernelGGL(fl_pass_kernel<FL_ZERO_STATE>, dim3(grid), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(fl_scan_kernel, dim3(slot_grid(a)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(fl_pass_kernel<FL_RECOMPUTE>, dim3(grid), dim3(64), 0, stream, a);
}
void launch_fl_fold(const FlArgs& a, hipStream_t stream) { hipLaunchKernelGGL(fl_fold_kernel, dim3(a.n_streams), dim3(64), 0, stream, a); }

}  // namespace omx

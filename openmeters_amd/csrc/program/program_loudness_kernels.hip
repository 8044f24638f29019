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
#include "program_loudness.hpp"

namespace omx {
namespace {

constexpr uint32_t TF = kPlTile;
constexpr int kTileLoads = 32;                    // dwords per lane and tile: 64 lanes x 32 = 64 slots x 32 frames
constexpr uint32_t kTileFloats = 64 * TF + 64;    // the largest tile: (64 >> shift) rows of TF * channels + (1 << shift) floats

__device__ __forceinline__ float ms_to_lufs(double ms, float floor) {  // loudness/processor.rs:57-66
    return ms > 0.0 ? (float)fmax(fma(log10(ms), 10.0, -0.691), (double)floor) : floor;
}
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

// ---- result pass: one workgroup per stream (or per interval of a stream: include/omx/program_timeline.h) over stored segment energies
constexpr uint32_t RT = 256;

// What the pass works on: the whole of a stream (made from its PlStreamMeta) or a part of it (made from a PlIntervalDesc)
struct PlResultDesc {
    const double* e;       // the first segment energy
    uint32_t n;            // how many
    uint32_t overflow;
    uint64_t frames;
    const float* tp_max;   // max_true_peak_db = the larger of *tp_max and *tp_measured; null: the floor (a part has no peak of its own)
    const float* tp_measured;  // null with peaks off
};

__device__ __forceinline__ double gating_block(const double* e, uint32_t j) {  // j >= 3
    return (((e[j - 3] + e[j - 2]) + e[j - 1]) + e[j]) * 0.25;
}
__device__ __forceinline__ double short_term_block(const double* e, uint32_t j) {  // j >= 29
    double acc = e[j - 29];
#pragma unroll
    for (uint32_t k = 1; k < 30; ++k) acc += e[j - 29 + k];
    return acc / 30.0;
}
// workgroup reductions in a fixed order (lane-strided partials, then a binary tree)
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = RT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_max(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = RT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + d]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void pl_result_block(const PlResultDesc& d, double absolute_gate, float floor_db, omx_program_loudness_record* out) {
    __shared__ double red[RT];
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long prefix[2];
    __shared__ uint32_t rank[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = d.n;
    const double* e = d.e;
    const uint32_t ng = n >= 4 ? n - 3 : 0, ns = n >= 30 ? n - 29 : 0;
    const double gate = absolute_gate;

    // ---- gating blocks: maximum, mean above the absolute gate, mean above both gates
    double sum = 0.0, cnt = 0.0, mx = 0.0;
    for (uint32_t j = 3 + tid; j < n; j += RT) {
        const double g = gating_block(e, j);
        mx = fmax(mx, g);
        if (g > gate) {
            sum += g;
            cnt += 1.0;
        }
    }
    const double g_max = block_max(mx, red);
    const double g_abs_sum = block_sum(sum, red), g_abs_cnt = block_sum(cnt, red);  // (counts < 2^53: exact)
    const double g_rel = g_abs_cnt > 0.0 ? 0.1 * (g_abs_sum / g_abs_cnt) : 0.0;
    sum = 0.0;
    cnt = 0.0;
    for (uint32_t j = 3 + tid; j < n; j += RT) {
        const double g = gating_block(e, j);
        if (g > gate && g > g_rel) {
            sum += g;
            cnt += 1.0;
        }
    }
    const double g_rel_sum = block_sum(sum, red), g_rel_cnt = block_sum(cnt, red);
    const double integrated = g_rel_cnt > 0.0 ? g_rel_sum / g_rel_cnt : 0.0;

    // ---- short-term blocks: maximum, relative gate, survivors
    sum = 0.0;
    cnt = 0.0;
    mx = 0.0;
    for (uint32_t j = 29 + tid; j < n; j += RT) {
        const double v = short_term_block(e, j);
        mx = fmax(mx, v);
        if (v > gate) {
            sum += v;
            cnt += 1.0;
        }
    }
    const double s_max = block_max(mx, red);
    const double s_abs_sum = block_sum(sum, red), s_abs_cnt = block_sum(cnt, red);
    const double s_rel = s_abs_cnt > 0.0 ? 0.01 * (s_abs_sum / s_abs_cnt) : 0.0;
    cnt = 0.0;
    for (uint32_t j = 29 + tid; j < n; j += RT) {
        const double v = short_term_block(e, j);
        if (v > gate && v > s_rel) cnt += 1.0;
    }
    const double s_rel_cnt = block_sum(cnt, red);

    // ---- loudness range: the two nearest-rank elements of the survivors by radix select on the f64 bit patterns (energies are
    // non-negative, so the patterns order like the values), eight bits per pass, both ranks in the same passes
    double lo_e = 0.0, hi_e = 0.0;
    if (s_rel_cnt > 0.0) {
        if (tid == 0) {
            prefix[0] = prefix[1] = 0ull;
            rank[0] = (uint32_t)floor((s_rel_cnt - 1.0) * 0.10 + 0.5);
            rank[1] = (uint32_t)floor((s_rel_cnt - 1.0) * 0.95 + 0.5);
        }
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            const unsigned long long done = pass == 0 ? 0ull : ~0ull << (shift + 8);
            hist[0][tid] = 0;
            hist[1][tid] = 0;
            __syncthreads();
            const unsigned long long pre0 = prefix[0], pre1 = prefix[1];
            for (uint32_t j = 29 + tid; j < n; j += RT) {
                const double v = short_term_block(e, j);
                if (v > gate && v > s_rel) {
                    const unsigned long long key = (unsigned long long)__double_as_longlong(v);
                    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
                    if ((key & done) == pre0) atomicAdd(&hist[0][digit], 1u);
                    if ((key & done) == pre1) atomicAdd(&hist[1][digit], 1u);
                }
            }
            __syncthreads();
            if (tid < 2) {
                uint32_t r = rank[tid], below = 0;
                for (uint32_t d = 0; d < 256; ++d) {
                    const uint32_t h = hist[tid][d];
                    if (r < below + h) {
                        prefix[tid] |= (unsigned long long)d << shift;
                        rank[tid] = r - below;
                        break;
                    }
                    below += h;
                }
            }
            __syncthreads();
        }
        lo_e = __longlong_as_double((long long)prefix[0]);
        hi_e = __longlong_as_double((long long)prefix[1]);
    }

    if (tid == 0) {
        omx_program_loudness_record r{};
        const float floor = floor_db;
        r.integrated_energy = integrated;
        r.relative_threshold_energy = g_rel;
        r.lra_low_energy = lo_e;
        r.lra_high_energy = hi_e;
        r.momentary_energy = ng ? gating_block(e, n - 1) : 0.0;
        r.short_term_energy = ns ? short_term_block(e, n - 1) : 0.0;
        r.max_momentary_energy = g_max;
        r.max_short_term_energy = s_max;
        r.frames = d.frames;
        r.segments = n;
        r.gating_blocks = ng;
        r.gating_above_absolute = (uint64_t)g_abs_cnt;
        r.gating_above_relative = (uint64_t)g_rel_cnt;
        r.short_term_blocks = ns;
        r.short_term_above_absolute = (uint64_t)s_abs_cnt;
        r.short_term_above_relative = (uint64_t)s_rel_cnt;
        r.integrated_lufs = ms_to_lufs(integrated, floor);
        r.relative_threshold_lufs = ms_to_lufs(g_rel, floor);
        r.loudness_range_lu = s_rel_cnt > 0.0 ? (float)(fma(log10(hi_e), 10.0, -0.691) - fma(log10(lo_e), 10.0, -0.691)) : 0.0f;
        r.momentary_lufs = ms_to_lufs(r.momentary_energy, floor);
        r.short_term_lufs = ms_to_lufs(r.short_term_energy, floor);
        r.max_momentary_lufs = ms_to_lufs(g_max, floor);
        r.max_short_term_lufs = ms_to_lufs(s_max, floor);
        r.max_true_peak_db = !d.tp_max ? floor : (d.tp_measured ? fmaxf(*d.tp_max, *d.tp_measured) : *d.tp_max);
        r.overflow = d.overflow;
        *out = r;
    }
}

__global__ __launch_bounds__(RT) void pl_result_kernel(PlResultArgs a) {
    const uint32_t s = blockIdx.x;
    const PlStreamMeta meta = a.meta[s];
    PlResultDesc d;
    d.e = a.segments + (uint64_t)s * a.capacity;
    d.n = (uint32_t)min((uint64_t)meta.segments, a.capacity);
    d.overflow = meta.overflow;
    d.frames = meta.frames;
    d.tp_max = a.tp_max + s;
    d.tp_measured = a.peaks ? &a.peaks[s].max_true_peak_db : nullptr;
    pl_result_block(d, a.absolute_gate, a.floor_db, a.records + s);
}

// One workgroup per interval: the same pass on e[first .. first + count) of a stream
__global__ __launch_bounds__(RT) void pl_interval_kernel(PlResultArgs a, const PlIntervalDesc* descs) {
    const PlIntervalDesc in = descs[blockIdx.x];
    PlResultDesc d;
    d.e = a.segments + in.offset;
    d.n = in.n;
    d.overflow = 0;
    d.frames = in.frames;
    d.tp_max = nullptr;
    d.tp_measured = nullptr;
    pl_result_block(d, a.absolute_gate, a.floor_db, a.records + blockIdx.x);
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

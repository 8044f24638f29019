// Device side of the programme bank's result pass over stored segment energies, shared by the per-stream and interval kernels
// (program_loudness_kernels.hip) and the group kernel (program_groups_kernels.hip): the block expressions, the workgroup reductions,
// the gated means, the loudness range by radix select and the record writer.  The pass is written once, over a SOURCE that says which
// gating and short-term blocks a lane visits and in which order:
//   PlSpanSource  : one (e, n).  Lane t visits block j = 3 + t (29 + t), then every 256th.
//   PlGroupSource : a list of such spans (include/omx/program_groups.h), program_groups_kernels.hip.
// Everything a lane does with a block, and everything after the lanes' partial sums, is the same code for every source.
// Include from .hip files only.
#pragma once
#include "program_loudness.hpp"

namespace omx {

constexpr uint32_t kPlResultThreads = 256;

__device__ __forceinline__ float ms_to_lufs(double ms, float floor) {  // loudness/processor.rs:57-66
    return ms > 0.0 ? (float)fmax(fma(log10(ms), 10.0, -0.691), (double)floor) : floor;
}
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
    for (uint32_t d = kPlResultThreads / 2; d > 0; d >>= 1) {
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
    for (uint32_t d = kPlResultThreads / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + d]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One span of stored energies: the whole of a stream or an interval of it
struct PlSpanSource {
    const double* e;  // the first segment energy
    uint32_t n;       // how many
    template <class F>
    __device__ __forceinline__ void for_gating(F&& f) const {
        for (uint32_t j = 3 + threadIdx.x; j < n; j += kPlResultThreads) f(gating_block(e, j));
    }
    template <class F>
    __device__ __forceinline__ void for_short_term(F&& f) const {
        for (uint32_t j = 29 + threadIdx.x; j < n; j += kPlResultThreads) f(short_term_block(e, j));
    }
    // the latest blocks and the counts of the record (one lane asks)
    __device__ __forceinline__ uint64_t segments() const { return n; }
    __device__ __forceinline__ uint64_t gating_blocks() const { return n >= 4 ? n - 3 : 0; }
    __device__ __forceinline__ uint64_t short_term_blocks() const { return n >= 30 ? n - 29 : 0; }
    __device__ __forceinline__ double momentary() const { return n >= 4 ? gating_block(e, n - 1) : 0.0; }
    __device__ __forceinline__ double short_term() const { return n >= 30 ? short_term_block(e, n - 1) : 0.0; }
};

// What the record holds besides the figures of the pass
struct PlRecordTail {
    uint64_t frames;
    uint32_t overflow;
    const float* tp_max;       // max_true_peak_db = the larger of *tp_max and *tp_measured; null: the floor (a part has no peak of its own)
    const float* tp_measured;  // null with peaks off
};

template <class Source>
__device__ __forceinline__ void pl_result_pass(const Source& src, const PlRecordTail& tail, double absolute_gate, float floor_db,
                                               omx_program_loudness_record* out) {
    constexpr uint32_t RT = kPlResultThreads;
    __shared__ double red[RT];
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long prefix[2];
    __shared__ uint32_t rank[2];
    const uint32_t tid = threadIdx.x;
    const double gate = absolute_gate;

    // ---- gating blocks: maximum, mean above the absolute gate, mean above both gates
    double sum = 0.0, cnt = 0.0, mx = 0.0;
    src.for_gating([&](double g) {
        mx = fmax(mx, g);
        if (g > gate) {
            sum += g;
            cnt += 1.0;
        }
    });
    const double g_max = block_max(mx, red);
    const double g_abs_sum = block_sum(sum, red), g_abs_cnt = block_sum(cnt, red);  // (counts < 2^53: exact)
    const double g_rel = g_abs_cnt > 0.0 ? 0.1 * (g_abs_sum / g_abs_cnt) : 0.0;
    sum = 0.0;
    cnt = 0.0;
    src.for_gating([&](double g) {
        if (g > gate && g > g_rel) {
            sum += g;
            cnt += 1.0;
        }
    });
    const double g_rel_sum = block_sum(sum, red), g_rel_cnt = block_sum(cnt, red);
    const double integrated = g_rel_cnt > 0.0 ? g_rel_sum / g_rel_cnt : 0.0;

    // ---- short-term blocks: maximum, relative gate, survivors
    sum = 0.0;
    cnt = 0.0;
    mx = 0.0;
    src.for_short_term([&](double v) {
        mx = fmax(mx, v);
        if (v > gate) {
            sum += v;
            cnt += 1.0;
        }
    });
    const double s_max = block_max(mx, red);
    const double s_abs_sum = block_sum(sum, red), s_abs_cnt = block_sum(cnt, red);
    const double s_rel = s_abs_cnt > 0.0 ? 0.01 * (s_abs_sum / s_abs_cnt) : 0.0;
    cnt = 0.0;
    src.for_short_term([&](double v) {
        if (v > gate && v > s_rel) cnt += 1.0;
    });
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
            src.for_short_term([&](double v) {
                if (v > gate && v > s_rel) {
                    const unsigned long long key = (unsigned long long)__double_as_longlong(v);
                    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
                    if ((key & done) == pre0) atomicAdd(&hist[0][digit], 1u);
                    if ((key & done) == pre1) atomicAdd(&hist[1][digit], 1u);
                }
            });
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
        r.momentary_energy = src.momentary();
        r.short_term_energy = src.short_term();
        r.max_momentary_energy = g_max;
        r.max_short_term_energy = s_max;
        r.frames = tail.frames;
        r.segments = src.segments();
        r.gating_blocks = src.gating_blocks();
        r.gating_above_absolute = (uint64_t)g_abs_cnt;
        r.gating_above_relative = (uint64_t)g_rel_cnt;
        r.short_term_blocks = src.short_term_blocks();
        r.short_term_above_absolute = (uint64_t)s_abs_cnt;
        r.short_term_above_relative = (uint64_t)s_rel_cnt;
        r.integrated_lufs = ms_to_lufs(integrated, floor);
        r.relative_threshold_lufs = ms_to_lufs(g_rel, floor);
        r.loudness_range_lu = s_rel_cnt > 0.0 ? (float)(fma(log10(hi_e), 10.0, -0.691) - fma(log10(lo_e), 10.0, -0.691)) : 0.0f;
        r.momentary_lufs = ms_to_lufs(r.momentary_energy, floor);
        r.short_term_lufs = ms_to_lufs(r.short_term_energy, floor);
        r.max_momentary_lufs = ms_to_lufs(g_max, floor);
        r.max_short_term_lufs = ms_to_lufs(s_max, floor);
        r.max_true_peak_db = !tail.tp_max ? floor : (tail.tp_measured ? fmaxf(*tail.tp_max, *tail.tp_measured) : *tail.tp_max);
        r.overflow = tail.overflow;
        *out = r;
    }
}

}  // namespace omx

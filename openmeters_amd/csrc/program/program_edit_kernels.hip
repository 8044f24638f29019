// Edit pass of the programme loudness bank (include/omx/program_edit.h states the definition, program_edit.hpp the passes,
// program_edit_plan.hpp the spans).
//
// The pass is bandwidth bound: 4 B written per output sample and 4 B read per clip that covers it.
//   main   : grid (tile of ed_tile_frames(C) frames of the output window, output stream), 256 threads, templated on the channel count C.
//            A tile wholly beyond out_frames[o] leaves after reading its stream's 48-byte call entry.
//     spans  the stream's spans are sorted and tile [0, 2^40): a binary search (a handful of uniform loads that hit L2) finds the one
//            that holds the tile's first frame, and the tile walks on from there.  The usual tile lies inside one span; a tile over
//            many short splices walks many, each with its own head and tail: correct, not fast.
//     run    the part of a span inside the tile is one contiguous run of d_out.  The floats in front of its first 16-byte boundary
//            (up to 3) and behind the last one go by dword (threads 0 .. 2 and 4 .. 6), the body in aligned 16-byte stores, as
//            pn_tile_kernel does.  A source of a run is a contiguous run of d_in at ANY 4-byte offset against the output (odd channel
//            counts, odd trims): where every source of the run is 16-byte aligned at the body's start the loads are dwordx4, otherwise
//            each vector is read as four dwords (the dword-load form).  All loads of a thread are issued before its first store, and
//            no load sits under a per-thread branch: a thread without a vector (or without an edge float) loads the run's last
//            vector (its first float) again and keeps nothing.
//     paths  uniform over the workgroup, by the span: zero fill (no load); plain (one or two sources with constant weights; a weight
//            of exactly 1.0f selects the loaded bits instead of the product: the header's copy rule); faded (the weight of a frame
//            comes from ed_weight, the function omx_program_edit_gain runs on the host, once per frame a vector touches and not once
//            per sample: a vector of four floats touches at most 4, 3 or 2 frames at 1, 2 or more channels, and which of them a float
//            belongs to follows from a division by the compile-time C; the weights are picked by selects, never by an index a
//            register holds, which would send them to scratch).
//     reduce PsTally (program_stage_device.hpp): count and maximum per thread over everything it stored, six shuffle steps, four
//            wavefronts through LDS, at most one atomicAdd (u64) and one atomicMax (bit pattern) per workgroup.
//   The record's counts (silent, faded, mixed frames, clips) follow from the spans and the window: the host puts them into the call
//   entry and the begin kernel writes them.  Only vector loads, vector stores and vector atomics are used; DESIGN.md lists registers,
//   LDS and scratch per instantiation.
#include "program_edit.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void ed_begin_kernel(EdArgs a) {
    const uint32_t o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.n_out) return;
    EdStreamCall c{};
    if (a.calls) c = a.calls[o];
    omx_program_edit_record r;
    r.out_first = c.out_first;
    r.frames = c.out_frames;
    r.silent_frames = c.silent_frames;
    r.faded_frames = c.faded_frames;
    r.mixed_frames = c.mixed_frames;
    r.samples_over = 0;
    r.out_sample_peak = 0.0f;
    r.out_sample_peak_db = a.floor_db;
    r.clips = c.clips;
    r._pad = 0;
    a.records[o] = r;
}

__global__ __launch_bounds__(64) void ed_finish_kernel(EdArgs a) {
    const uint32_t o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.n_out) return;
    a.records[o].out_sample_peak_db = ps_peak_db(a.records[o].out_sample_peak, a.floor_db);
}

// frames a 16-byte vector can touch at C channels, whatever its offset inside a frame
template <int C>
constexpr uint32_t ed_vector_frames() { return C == 1 ? 4 : (C == 2 ? 3 : 2); }

// The weights of the frames a vector touches (or of its four floats), as named registers: an array picked by a value a register
// holds goes to scratch (or, promoted, to LDS).
struct EdFrameWeights {
    float w0, w1, w2, w3;
    // the weight of the float `at` floats behind the first float of frame 0 (at < 4 * C).  By thresholds: a chain of selects on
    // idx == 1, idx == 2 .. is turned back into an indexed table by the compiler.
    template <int C>
    __device__ __forceinline__ float pick(uint32_t at) const {
        float v = w0;
        v = at >= C ? w1 : v;
        if (C <= 2) v = at >= 2 * C ? w2 : v;
        if (C == 1) v = at >= 3 * C ? w3 : v;
        return v;
    }
    // the weights of a vector's four floats, the first of them channel r of frame 0
    template <int C>
    __device__ __forceinline__ EdFrameWeights spread(uint32_t r) const {
        if (C == 2) {  // (by the one bit of r: the thresholds 2 and 4 are a shift to the compiler, and an index again)
            const bool odd = r != 0;
            return EdFrameWeights{w0, odd ? w1 : w0, w1, odd ? w2 : w1};
        }
        return EdFrameWeights{pick<C>(r), pick<C>(r + 1), pick<C>(r + 2), pick<C>(r + 3)};
    }
};
template <uint32_t NF>
__device__ __forceinline__ EdFrameWeights ed_frame_weights(const EdClip& c, const float* tabs, uint64_t frame, bool fade_in, bool fade_out) {
    EdFrameWeights w{0.0f, 0.0f, 0.0f, 0.0f};
    w.w0 = ed_weight(c, tabs, frame, fade_in, fade_out);
    w.w1 = ed_weight(c, tabs, frame + 1, fade_in, fade_out);
    if (NF > 2) w.w2 = ed_weight(c, tabs, frame + 2, fade_in, fade_out);
    if (NF > 3) w.w3 = ed_weight(c, tabs, frame + 3, fade_in, fade_out);
    return w;
}

// one clip's share of an output sample: the loaded bits where the header says copy, else the rounded product
__device__ __forceinline__ float ed_scaled(float x, float w, bool copy) { return copy ? x : w * x; }

// One run: n floats at d (n >= 1), the first of them channel 0 of absolute output frame `frame`; sa / sb: the floats of the sources
// that land on d[0].  NS sources (0: zero fill), FADED: per-frame weights, WIDE: every source is 16-byte aligned where d's body starts.
template <int C, int NS, bool FADED, bool WIDE>
__device__ __forceinline__ void ed_run(float* d, uint32_t n, uint64_t frame, const float* sa, const float* sb, const EdClip& ca, const EdClip& cb,
                                       uint32_t flags, const float* tabs, PsTally& tally) {
    constexpr uint32_t K = ed_in_flight(C), NF = ed_vector_frames<C>();
    const uint32_t tid = threadIdx.x;
    const uint32_t peel = min(n, ps_to_aligned(d));
    const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
    // which fades apply (uniform), and which clips are copied where no fade applies
    const bool in_a = flags & kEdFadeInA, out_a = flags & kEdFadeOutA, in_b = flags & kEdFadeInB, out_b = flags & kEdFadeOutB;
    const bool copy_a = NS >= 1 && !in_a && !out_a && ca.gain == 1.0f, copy_b = NS >= 2 && !in_b && !out_b && cb.gain == 1.0f;

    // ---- the floats outside the aligned body: threads 0 .. 2 the head, threads 4 .. 6 the tail
    uint32_t e = n;
    if (tid < peel) e = tid;
    else if (tid >= 4 && tid < 4 + tail) e = peel + 4 * nvec + (tid - 4);
    const uint32_t ec = e < n ? e : 0u;
    float xe_a = 0.0f, xe_b = 0.0f;
    if (NS >= 1) xe_a = sa[ec];
    if (NS >= 2) xe_b = sb[ec];

    // ---- the body's loads
    v4f xa[K], xb[K];
    if (NS >= 1 && nvec != 0) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t v = min(k * kEdThreads + tid, nvec - 1);
            const float* pa = sa + peel + 4 * v;
            if (WIDE) xa[k] = *reinterpret_cast<const v4f*>(pa);
            else xa[k] = v4f{pa[0], pa[1], pa[2], pa[3]};
            if (NS >= 2) {
                const float* pb = sb + peel + 4 * v;
                if (WIDE) xb[k] = *reinterpret_cast<const v4f*>(pb);
                else xb[k] = v4f{pb[0], pb[1], pb[2], pb[3]};
            }
        }
    }

    // ---- edge float
    {
        float y = 0.0f;
        if (NS >= 1) {
            float wa = ca.gain, wb = cb.gain;
            if (FADED) {
                const uint64_t f = frame + ec / C;
                wa = ed_weight(ca, tabs, f, in_a, out_a);
                if (NS >= 2) wb = ed_weight(cb, tabs, f, in_b, out_b);
            }
            y = ed_scaled(xe_a, wa, copy_a);
            if (NS >= 2) y = y + ed_scaled(xe_b, wb, copy_b);
        }
        if (e < n) {
            if (NS >= 1) tally.take(y);
            d[e] = y;
        }
    }

    // ---- body
    if (nvec != 0) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t v = k * kEdThreads + tid;
            v4f y = v4f{0.0f, 0.0f, 0.0f, 0.0f};
            if (NS >= 1) {
                EdFrameWeights wa{ca.gain, ca.gain, ca.gain, ca.gain}, wb{cb.gain, cb.gain, cb.gain, cb.gain};  // per float of the vector
                if (FADED) {
                    const uint32_t q = peel + 4 * min(v, nvec - 1);  // the vector's first float in the run
                    const uint32_t f0 = q / C, r = q - f0 * C;
                    const EdFrameWeights fa = ed_frame_weights<NF>(ca, tabs, frame + f0, in_a, out_a);
                    wa = fa.spread<C>(r);
                    if (NS >= 2) {
                        const EdFrameWeights fb = ed_frame_weights<NF>(cb, tabs, frame + f0, in_b, out_b);
                        wb = fb.spread<C>(r);
                    }
                }
                y.x = ed_scaled(xa[k].x, wa.w0, copy_a);
                y.y = ed_scaled(xa[k].y, wa.w1, copy_a);
                y.z = ed_scaled(xa[k].z, wa.w2, copy_a);
                y.w = ed_scaled(xa[k].w, wa.w3, copy_a);
                if (NS >= 2) {
                    y.x = y.x + ed_scaled(xb[k].x, wb.w0, copy_b);
                    y.y = y.y + ed_scaled(xb[k].y, wb.w1, copy_b);
                    y.z = y.z + ed_scaled(xb[k].z, wb.w2, copy_b);
                    y.w = y.w + ed_scaled(xb[k].w, wb.w3, copy_b);
                }
            }
            if (v < nvec) {
                if (NS >= 1) {
                    tally.take(y.x);
                    tally.take(y.y);
                    tally.take(y.z);
                    tally.take(y.w);
                }
                *reinterpret_cast<v4f*>(d + peel + 4 * v) = y;
            }
        }
    }
}

template <int C, int NS, bool FADED>
__device__ __forceinline__ void ed_run_aligned(float* d, uint32_t n, uint64_t frame, const float* sa, const float* sb, const EdClip& ca,
                                               const EdClip& cb, uint32_t flags, const float* tabs, PsTally& tally) {
    const uint32_t peel = min(n, ps_to_aligned(d));
    const uintptr_t bits = reinterpret_cast<uintptr_t>(sa + peel) | (NS >= 2 ? reinterpret_cast<uintptr_t>(sb + peel) : 0);
    if ((bits & 15u) == 0) ed_run<C, NS, FADED, true>(d, n, frame, sa, sb, ca, cb, flags, tabs, tally);
    else ed_run<C, NS, FADED, false>(d, n, frame, sa, sb, ca, cb, flags, tabs, tally);
}

template <int C>
__global__ __launch_bounds__(kEdThreads) void ed_main_kernel(EdArgs a, uint32_t o_base) {
    constexpr uint32_t kTile = ed_tile_frames(C);
    const uint32_t o = o_base + blockIdx.y;
    const EdStreamCall call = a.calls[o];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;  // the tile's first frame inside the window
    if (t0 >= call.out_frames) return;  // (uniform over the workgroup: no thread is left at the barrier of the tally)
    const uint32_t nf = (uint32_t)min((uint64_t)kTile, (uint64_t)call.out_frames - t0);
    const uint64_t first = call.out_first + t0, last = first + nf;  // absolute output frames
    float* row = a.out + (uint64_t)o * a.out_capacity * C;
    const EdSpan* sp = a.spans + call.span_begin;
    uint32_t lo = 0, hi = call.span_count;  // sp[lo].first <= first (span 0 starts at frame 0), sp[hi].first > first
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sp[mid].first <= first) lo = mid;
        else hi = mid;
    }
    PsTally tally;
    for (uint32_t i = lo; i < call.span_count; ++i) {
        const EdSpan s = sp[i];
        if (s.first >= last) break;
        const uint64_t ra = max(first, s.first), rb = min(last, s.end);
        if (ra >= rb) continue;
        const uint32_t n = (uint32_t)(rb - ra) * C;
        float* d = row + (ra - call.out_first) * C;
        if (s.n_clips == 0) {
            const EdClip none{};
            ed_run<C, 0, false, true>(d, n, ra, nullptr, nullptr, none, none, 0u, a.tabs, tally);
            continue;
        }
        const EdClip ca = a.clips[s.a];
        const float* sa = a.in + (ca.src_base + (ra - ca.dst_first)) * C;
        if (s.n_clips == 1) {
            if (s.flags) ed_run_aligned<C, 1, true>(d, n, ra, sa, nullptr, ca, ca, s.flags, a.tabs, tally);
            else ed_run_aligned<C, 1, false>(d, n, ra, sa, nullptr, ca, ca, 0u, a.tabs, tally);
            continue;
        }
        const EdClip cb = a.clips[s.b];
        const float* sb = a.in + (cb.src_base + (ra - cb.dst_first)) * C;
        if (s.flags) ed_run_aligned<C, 2, true>(d, n, ra, sa, sb, ca, cb, s.flags, a.tabs, tally);
        else ed_run_aligned<C, 2, false>(d, n, ra, sa, sb, ca, cb, 0u, a.tabs, tally);
    }
    tally.fold_workgroup<kEdThreads>();
    if (threadIdx.x == 0) tally.commit(a.records + o);
}

template <int C>
void ed_launch_main(const EdArgs& a, hipStream_t stream) {
    constexpr uint32_t kTile = ed_tile_frames(C);
    const uint64_t tiles = std::max<uint64_t>(((uint64_t)a.max_frames + kTile - 1) / kTile, 1);
    for_stream_slabs(a.n_out, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(ed_main_kernel<C>, dim3((uint32_t)tiles, count), dim3(kEdThreads), 0, stream, a, base);
    });
}

}  // namespace

void launch_ed_begin(const EdArgs& a, hipStream_t stream) {
    ps_launch_per_stream(ed_begin_kernel, a.n_out, stream, a);
}
void launch_ed_finish(const EdArgs& a, hipStream_t stream) {
    ps_launch_per_stream(ed_finish_kernel, a.n_out, stream, a);
}
void launch_ed_main(const EdArgs& a, hipStream_t stream) {
    switch (a.channels) {
        case 1: ed_launch_main<1>(a, stream); break;
        case 2: ed_launch_main<2>(a, stream); break;
        case 3: ed_launch_main<3>(a, stream); break;
        case 4: ed_launch_main<4>(a, stream); break;
        case 5: ed_launch_main<5>(a, stream); break;
        case 6: ed_launch_main<6>(a, stream); break;
        case 7: ed_launch_main<7>(a, stream); break;
        default: ed_launch_main<8>(a, stream); break;
    }
}

}  // namespace omx

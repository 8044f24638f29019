// The convolve stage of the programme loudness bank (include/omx/program_convolve.h states the definition, program_convolve.hpp the
// passes).
//
// Indices.  `rel` counts input frames from the first frame of the call: frame n of the stream is rel = n - n_old.  Frames in front of
// the call (rel < 0) come from the ring the carry pass of the earlier calls wrote (the newest max_taps - 1 frames, frame n at slot
// n mod (max_taps - 1)), frames in front of the stream (n < 0) are +0, and so are frames at and beyond the last frame taken, which only
// a flush reads.  Output frame e_old + f of the stream is frame f of the call and reads x[n - k] with n at rel = rel_e + f.
//
//   main   : grid (tile of TILE output frames, stream).  A tile wholly beyond the stream's emission leaves after reading its call
//            entry.  A workgroup is four wavefronts; a thread computes R = 8 consecutive output frames of ONE channel, and the 64
//            threads of a wavefront take 512 consecutive frames of the same channel, so a wavefront's taps are uniform (the tap
//            pointer is made from values the compiler knows to be uniform).  TILE is 512 frames (2048 at one channel, 1024 at two,
//            so that every wavefront has work); at five to eight channels a wavefront takes two channels.
//            The taps are taken in blocks of KB = 256 ascending k with the 8 f64 accumulators of a thread kept in registers: the
//            order of the definition is kept and LDS does not grow with T.  Per block the input span, (block width + tile) frames of
//            every channel, goes to LDS once: aligned 16-byte loads when the span lies inside the call, frame by frame when it
//            reaches the ring, the zeros in front of the stream or behind a flush.
//            LDS is planar per channel.  A thread reads its samples as aligned runs of 8 floats (two ds_read_b128) and lane g's run
//            starts 32 bytes behind lane g - 1's; laid out flat, the sixteen lanes of a ds_read_b128 group would cover 128 dwords, every
//            bank twice.  So a row keeps the even 16-byte pieces in its first half and the odd ones in its second: the lanes' reads
//            of either half are 16 bytes apart and cover every bank once.
//            Sliding window: tap k of frame r reads sample (r - k) of the thread's run, so over 8 taps the 8 frames read 15
//            consecutive samples: the run before (8 new floats, converted to f64 once) and the run of the 8 taps before.  Two
//            ds_read_b128, 8 conversions and 8 uniform tap loads feed 64 f64 multiply-adds.  The products are exact in f64, so the
//            fma gives what the header's "product, then sum" gives; the accumulators start at -0.0, which the first term replaces on
//            bits.  A FIR's last taps (T mod 8) run the same code under a uniform guard per tap: no zero tap is ever added.
//            A bypassed channel picks x[m] out of the block that holds tap D and keeps its bits.
//            The results go through LDS (the staging's space, frame-interleaved, one pad dword per thread's run against bank
//            conflicts) and leave in 16-byte stores of consecutive floats.  Counts are summed and the peak is taken on bit
//            patterns, per wave, then per workgroup, with at most one atomic of each kind per workgroup: order-free, so the record
//            is deterministic.
//   carry  : behind the main pass on the same stream: the newest min(F, max_taps - 1) frames of the call into the ring.  The slots it
//            does not write keep the older frames, so a call of fewer frames, or of none, leaves the newest max_taps - 1 in place.
//   Only vector stores and vector atomics are used.
#include "program_convolve.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr uint32_t kCvR = kCvFramesPerThread, kCvKB = kCvTapBlock;
static_assert(kCvR == 8 && kCvKB % kCvR == 0, "the window code below is written for runs of 8");

__device__ __forceinline__ omx_program_convolve_record cv_idle_record(const CvArgs& a) {
    omx_program_convolve_record r{};
    r.out_sample_peak_db = a.floor_db;
    r.state = OMX_CONVOLVE_IDLE;
    r.delay_frames = a.delay;
    r.max_taps = a.max_taps;
    return r;
}

__global__ __launch_bounds__(64) void cv_begin_kernel(CvArgs a, uint32_t whole_call) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const CvStreamCall c = a.calls[s];
    omx_program_convolve_record r = a.records[s];
    if (c.flags & kCarryFlagClear) r = cv_idle_record(a);
    if (whole_call) ps_begin_record<OMX_CONVOLVE_IDLE, OMX_CONVOLVE_RUNNING, OMX_CONVOLVE_FLUSHED>(r, c.n_old, c.e_old, c.frames, c.emit, c.flags);
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void cv_finish_kernel(CvArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    a.records[s].out_sample_peak_db = ps_peak_db(a.records[s].out_sample_peak, a.floor_db);
}

// Where sample j of a channel's row lies: the even 16-byte pieces in the first half, the odd ones in the second
template <uint32_t HALF>
__device__ __forceinline__ uint32_t cv_row_at(uint32_t j) {
    const uint32_t piece = j >> 2;
    return (piece & 1u) * HALF + (piece >> 1) * 4 + (j & 3u);
}

// run `run` (samples 8 run .. 8 run + 7) of a row, as f64
template <uint32_t HALF>
__device__ __forceinline__ void cv_load_run(const float* row, uint32_t run, double (&w)[8]) {
    const v4f lo = *reinterpret_cast<const v4f*>(row + run * 4), hi = *reinterpret_cast<const v4f*>(row + HALF + run * 4);
    w[0] = (double)lo.x, w[1] = (double)lo.y, w[2] = (double)lo.z, w[3] = (double)lo.w;
    w[4] = (double)hi.x, w[5] = (double)hi.y, w[6] = (double)hi.z, w[7] = (double)hi.w;
}

// Eight taps h[0 .. 7] (the first `n` of them when GUARDED) on the eight frames of a thread: frame r under tap q reads sample r - q
// of the window, `cur` for r - q >= 0 and `prev` (the run in front of it) below.  Ascending q for every frame.
template <bool GUARDED>
__device__ __forceinline__ void cv_eight_taps(double (&acc)[8], const double* __restrict__ h, uint32_t n, const double (&cur)[8],
                                              const double (&prev)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (GUARDED && (uint32_t)q >= n) break;
        const double hq = h[q];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = __builtin_fma(hq, r - q >= 0 ? cur[(r - q) & 7] : prev[(8 + r - q) & 7], acc[r]);
    }
}

template <int C>
__global__ __launch_bounds__(kCvThreads) void cv_main_kernel(CvArgs a, uint32_t s_base) {
    constexpr uint32_t G = cv_groups(C), TILE = G * kCvR, ROW = kCvKB + TILE, HALF = ROW / 2;
    constexpr uint32_t ITEMS = C * (G / 64), NI = (ITEMS + 3) / 4;  // (channel, 64 runs) pieces of the tile, and how many a wavefront takes
    static_assert(HALF % 4 == 0 && TILE * C + G <= C * ROW, "the rows' halves are 16-byte aligned; the results fit the staging");
    __shared__ __attribute__((aligned(16))) float s_x[C * ROW];
    const uint32_t s = s_base + blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const CvStreamCall call = a.calls[s];
    const uint64_t first = (uint64_t)blockIdx.x * TILE;  // the tile's first frame, counted from the call's first emitted frame
    if (first >= call.emit) return;  // (uniform over the workgroup: no thread is left at a barrier below)
    const uint32_t n_out = (uint32_t)min((uint64_t)TILE, (uint64_t)call.emit - first);
    const uint32_t n_runs8 = (n_out + 7u) & ~7u;  // the frames of the runs that hold an output

    uint32_t item_c[NI], item_g[NI], item_taps[NI], item_first[NI];
    bool item_live[NI];
    double acc[NI][8];
#pragma unroll
    for (uint32_t j = 0; j < NI; ++j) {
        const uint32_t item = wave + 4 * j;
        item_live[j] = item < ITEMS;
        item_c[j] = item_live[j] ? item / (G / 64) : 0u;
        item_g[j] = (item % (G / 64)) * 64 + lane;
        const CvChannel ch = a.chan[(uint64_t)s * OMX_MAX_CHANNELS + item_c[j]];
        item_taps[j] = __builtin_amdgcn_readfirstlane(ch.n_taps);
        item_first[j] = __builtin_amdgcn_readfirstlane(ch.tap_first);
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[j][r] = -0.0;
    }

    const int64_t rel_first = call.rel_e + (int64_t)first;  // the newest frame the tile's first output reads
    for (uint32_t kb0 = 0; kb0 < call.reach; kb0 += kCvKB) {
        const uint32_t kbw = min(kCvKB, (call.reach - kb0 + 7u) & ~7u);  // the block's width, whole runs
        // row sample j is x at rel_base + j: tap kb0 + q of tile frame f reads sample kbw + f - q
        const int64_t rel_base = rel_first - (int64_t)kb0 - (int64_t)kbw;
        const uint32_t span = kbw + n_runs8, n = span * C;
        if (kb0 != 0) __syncthreads();  // (the block before has been read)
        const auto stage = [&](uint32_t idx, float value) {
            const uint32_t fr = idx / C, c = idx - fr * C;
            s_x[c * ROW + cv_row_at<HALF>(fr)] = value;
        };
        if (rel_base >= 0 && rel_base + (int64_t)span <= (int64_t)call.frames) {
            // the span is one contiguous run of d_in: aligned 16-byte loads, four in flight per thread; the floats outside the
            // aligned body as dwords
            const float* src = a.in + ((uint64_t)s * a.frames_capacity + (uint64_t)rel_base) * C;
            const uint32_t peel = min(n, ps_to_aligned(src));
            const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
            if (tid < peel) stage(tid, src[tid]);
            else if (tid >= 4 && tid < 4 + tail) stage(peel + 4 * nvec + (tid - 4), src[peel + 4 * nvec + (tid - 4)]);
            for (uint32_t v0 = 0; v0 < nvec; v0 += 4 * kCvThreads) {
                v4f v[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint32_t i = v0 + u * kCvThreads + tid;
                    v[u] = i < nvec ? *reinterpret_cast<const v4f*>(src + peel + 4 * i) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
                }
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint32_t i = v0 + u * kCvThreads + tid, idx = peel + 4 * i;
                    if (i < nvec) {
                        stage(idx, v[u].x);
                        stage(idx + 1, v[u].y);
                        stage(idx + 2, v[u].z);
                        stage(idx + 3, v[u].w);
                    }
                }
            }
        } else {
            // (further back than the ring reaches lies only the staging's alignment pad: no tap reads it)
            for (uint32_t idx = tid; idx < n; idx += kCvThreads) stage(idx, ps_ring_x_at(a, call, s, rel_base + (int64_t)(idx / C), idx % C));
        }
        __syncthreads();

#pragma unroll
        for (uint32_t j = 0; j < NI; ++j) {
            if (!item_live[j]) continue;
            const float* row = s_x + item_c[j] * ROW;
            const uint32_t g = item_g[j], T = item_taps[j];
            if (g * kCvR >= n_runs8) continue;  // (the run holds no output: its samples were not staged)
            if (T == 0) {  // bypass: x[m], which is tap D of the window, on bits
                if (a.delay >= kb0 && a.delay - kb0 < kCvKB) {
                    const uint32_t at = kbw + g * kCvR - (a.delay - kb0);
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        acc[j][r] = __longlong_as_double((long long)__float_as_uint(row[cv_row_at<HALF>(at + r)]));
                }
            } else if (kb0 < T) {
                const uint32_t nq = min(T - kb0, kbw);
                const double* __restrict__ h = a.taps + item_first[j] + kb0;
                uint32_t run = (kbw >> 3) + g;  // the thread's run under tap kb0
                double w0[8], w1[8];
                cv_load_run<HALF>(row, run, w0);
                for (uint32_t q0 = 0; q0 < nq; q0 += 16) {  // (two steps per trip: the windows swap roles without a copy)
                    cv_load_run<HALF>(row, --run, w1);
                    if (q0 + 8 <= nq) cv_eight_taps<false>(acc[j], h + q0, 8, w0, w1);
                    else cv_eight_taps<true>(acc[j], h + q0, nq - q0, w0, w1);
                    if (q0 + 8 >= nq) break;
                    cv_load_run<HALF>(row, --run, w0);
                    if (q0 + 16 <= nq) cv_eight_taps<false>(acc[j], h + q0 + 8, 8, w1, w0);
                    else cv_eight_taps<true>(acc[j], h + q0 + 8, nq - q0 - 8, w1, w0);
                }
            }
        }
    }

    // the results through LDS: frame-interleaved as they lie in d_out, one pad dword per run of 8 frames
    __syncthreads();
    PsTally tally;
    uint32_t nonfinite = 0;
#pragma unroll
    for (uint32_t j = 0; j < NI; ++j) {
        if (!item_live[j]) continue;
        const uint32_t g = item_g[j];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float y = item_taps[j] == 0 ? __uint_as_float((uint32_t)__double_as_longlong(acc[j][r])) : (float)acc[j][r];
            if (g * kCvR + r < n_out) {
                tally.take(y);
                nonfinite += (__float_as_uint(y) & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
                s_x[(g * kCvR + r) * C + item_c[j] + g] = y;
            }
        }
    }
    __syncthreads();
    {
        const uint32_t n = n_out * C;
        float* dst = a.out + ((uint64_t)s * a.out_capacity + first) * C;
        const auto staged = [&](uint32_t idx) { return s_x[idx + idx / (kCvR * C)]; };
        const uint32_t peel = min(n, ps_to_aligned(dst));
        const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
        if (tid < peel) dst[tid] = staged(tid);
        else if (tid >= 4 && tid < 4 + tail) dst[peel + 4 * nvec + (tid - 4)] = staged(peel + 4 * nvec + (tid - 4));
        for (uint32_t i = tid; i < nvec; i += kCvThreads) {
            const uint32_t idx = peel + 4 * i;
            *reinterpret_cast<v4f*>(dst + idx) = v4f{staged(idx), staged(idx + 1), staged(idx + 2), staged(idx + 3)};
        }
    }

    // the folds: one loop of shuffles for the three values, one barrier
    __shared__ uint32_t s_nonfinite[kCvThreads / 64];
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        tally.fold_step(step);
        ps_fold_step(nonfinite, PsSum{}, step);
    }
    ps_fold_post(nonfinite, s_nonfinite);
    tally.fold_waves<kCvThreads>();  // (holds the barrier)
    if (tid == 0) {
        ps_fold_gather<kCvThreads>(nonfinite, PsSum{}, s_nonfinite);
        tally.commit(a.records + s);
        if (nonfinite != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.records[s].samples_nonfinite), (unsigned long long)nonfinite);
    }
}

// ---- carry: frame n of the stream at slot n mod (max_taps - 1) of its ring
__global__ __launch_bounds__(256) void cv_carry_kernel(CvArgs a, uint32_t s_base) {
    const uint32_t s = s_base + blockIdx.y;
    const CvStreamCall call = a.calls[s];
    const uint32_t C = a.channels;
    ps_carry_row(a.ring + (uint64_t)s * a.history * C, a.history, C, call.ring, call.frames, blockIdx.x * 256 + threadIdx.x,
                 [&](uint64_t rel, uint32_t c) { return a.in[((uint64_t)s * a.frames_capacity + rel) * C + c]; });
}

template <int C>
void cv_launch_main(const CvArgs& a, hipStream_t stream) {
    const uint64_t tiles = ((uint64_t)a.max_emit + cv_tile(C) - 1) / cv_tile(C);
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(cv_main_kernel<C>, dim3((uint32_t)tiles, count), dim3(kCvThreads), 0, stream, a, base);
    });
}

}  // namespace

void launch_cv_begin(const CvArgs& a, bool whole_call, hipStream_t stream) {
    ps_launch_per_stream(cv_begin_kernel, a.n_streams, stream, a, whole_call ? 1u : 0u);
}
void launch_cv_finish(const CvArgs& a, hipStream_t stream) {
    ps_launch_per_stream(cv_finish_kernel, a.n_streams, stream, a);
}
void launch_cv_main(const CvArgs& a, hipStream_t stream) {
    switch (a.channels) {
        case 1: cv_launch_main<1>(a, stream); break;
        case 2: cv_launch_main<2>(a, stream); break;
        case 3: cv_launch_main<3>(a, stream); break;
        case 4: cv_launch_main<4>(a, stream); break;
        case 5: cv_launch_main<5>(a, stream); break;
        case 6: cv_launch_main<6>(a, stream); break;
        case 7: cv_launch_main<7>(a, stream); break;
        default: cv_launch_main<8>(a, stream); break;
    }
}
void launch_cv_carry(const CvArgs& a, hipStream_t stream) {
    if (a.history == 0) return;  // (a table of one-tap FIRs reads no earlier frame)
    const uint64_t tiles = ((uint64_t)a.history * a.channels + 255) / 256;
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(cv_carry_kernel, dim3((uint32_t)tiles, count), dim3(256), 0, stream, a, base);
    });
}

}  // namespace omx

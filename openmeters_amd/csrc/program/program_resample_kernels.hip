// Sample-rate conversion of the programme loudness bank (include/omx/program_resample.h states the definition, program_resample.hpp the
// passes).
//
// Indices.  `rel` counts input frames from the first frame of the call: frame n of the stream is rel = n - n_old.  Frames in front of
// the call (rel < 0) come from the ring the carry pass of the earlier calls wrote (the newest T - 1 frames, frame n at slot
// n mod (T - 1)), frames in front of the stream (n < 0) are +0, and so are frames at and beyond the last frame taken, which only a
// flush reads.  Output frame e_old + f of the stream is frame f of the call; the host hands over (e_old * M) / L - n_old and
// (e_old * M) % L, so that no thread divides a 64-bit position: thread 0 of a workgroup divides once for the tile's first frame, the
// others go on from its quotient and remainder in 32 bits (remainder + 255 * M < 2^19).
//
//   main   : grid (tile of `tile` output frames, stream).  A tile wholly beyond the stream's emission leaves after reading its call
//            entry.  The input frames the tile reaches, i0(first) - H + 1 .. i0(last) + H, go to LDS (a tile inside the call: aligned 16-byte
//            loads of one contiguous run; else float by float, the part in front of the call from the ring), interleaved as they lie
//            in memory or, with 8 channels, as two planes of four.  A thread then computes one output frame for all
//            channels: per four taps one 16-byte load of its phase's taps (through L1 / L2.  The device's table is [T / 4][L][4]: the
//            64 lanes of a wave have 64 different phases, and at one k they read 16-byte pieces of one stretch of L * 16 bytes, 20
//            cache lines at L = 160; as [L][T] rows every lane would touch a line of its own) and four frames from LDS, each in
//            vectors (8 channels: two ds_read_b128 from two planes, 4: one, 2: ds_read_b64, odd counts: dwords); four accumulators per channel
//            (k mod 4), multiply THEN add: the library is built with -ffp-contract=off.  The frame leaves in 16-byte stores where the
//            channel count and d_out's address allow.  Counts are summed and the peak is taken on bit patterns, per wave, then per
//            workgroup, with at most one atomic of each kind per workgroup: order-free, so the record is deterministic.
//   carry  : behind the main pass on the same stream: the newest min(F, T - 1) frames of the call into the ring.  The slots it does
//            not write keep the older frames, so a call of F < T - 1 frames, or of none, leaves the newest T - 1 frames in place.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_resample.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ omx_program_resample_record rs_idle_record(const RsArgs& a) {
    omx_program_resample_record r{};
    r.out_sample_peak_db = a.floor_db;
    r.state = OMX_RESAMPLE_IDLE;
    r.L = a.L;
    r.M = a.M;
    r.taps = a.taps;
    r.latency_frames = a.half;
    return r;
}

__global__ __launch_bounds__(64) void rs_begin_kernel(RsArgs a, uint32_t whole_call) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const RsStreamCall c = a.calls[s];
    omx_program_resample_record r = a.records[s];
    if (c.flags & kCarryFlagClear) r = rs_idle_record(a);
    if (whole_call) ps_begin_record<OMX_RESAMPLE_IDLE, OMX_RESAMPLE_RUNNING, OMX_RESAMPLE_FLUSHED>(r, c.n_old, c.e_old, c.frames, c.emit, c.flags);
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void rs_finish_kernel(RsArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    a.records[s].out_sample_peak_db = ps_peak_db(a.records[s].out_sample_peak, a.floor_db);
}

// Where sample (frame fr, channel c) of the staging lies.  Up to 7 channels: interleaved, as in memory.  8 channels: two planes of four
// channels, [2][span][4]: neighbouring lanes then read 16 bytes 16 bytes apart (a ds_read_b128 without a bank conflict; interleaved
// they would lie 32 bytes apart, two lanes of every sixteen on the same banks).
template <int C>
__device__ __forceinline__ uint32_t rs_staged_at(uint32_t fr, uint32_t c, uint32_t span) {
    if constexpr (C == 8) return (c >> 2) * span * 4 + fr * 4 + (c & 3u);
    else return fr * C + c;
}

// one frame out of LDS in the vectors the channel count allows (the staging starts 16-byte aligned)
template <int C>
__device__ __forceinline__ void rs_load_frame(const float* s_x, uint32_t fr, uint32_t span, float (&x)[C]) {
    if constexpr (C == 8) {
        const v4f lo = *reinterpret_cast<const v4f*>(s_x + fr * 4), hi = *reinterpret_cast<const v4f*>(s_x + (span + fr) * 4);
        x[0] = lo.x, x[1] = lo.y, x[2] = lo.z, x[3] = lo.w, x[4] = hi.x, x[5] = hi.y, x[6] = hi.z, x[7] = hi.w;
    } else if constexpr (C == 4) {
        const v4f v = *reinterpret_cast<const v4f*>(s_x + fr * 4);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else if constexpr (C % 2 == 0) {
#pragma unroll
        for (int i = 0; i < C; i += 2) {
            const v2f v = *reinterpret_cast<const v2f*>(s_x + fr * C + i);
            x[i] = v.x, x[i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) x[i] = s_x[fr * C + i];
    }
}

template <int C>
__global__ __launch_bounds__(kRsThreads) void rs_main_kernel(RsArgs a, uint32_t s_base) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];  // [span][C]; 8 channels: [2][span][4]
    __shared__ uint32_t s_head[3];                               // the tile's quotient (low, high) and remainder
    const uint32_t s = s_base + blockIdx.y, tid = threadIdx.x;
    const RsStreamCall call = a.calls[s];
    const uint64_t first = (uint64_t)blockIdx.x * a.tile;  // the tile's first frame, counted from the call's first emitted frame
    if (first >= call.emit) return;  // (uniform over the workgroup: no thread is left at a barrier below)
    const uint32_t n_out = (uint32_t)min((uint64_t)a.tile, (uint64_t)call.emit - first);
    const uint32_t L = a.L, M = a.M, T = a.taps;
    if (tid == 0) {
        const uint64_t b = first * M + call.phase_e, q = b / L;
        s_head[0] = (uint32_t)q;
        s_head[1] = (uint32_t)(q >> 32);
        s_head[2] = (uint32_t)(b - q * L);
    }
    __syncthreads();
    const uint64_t q0 = (uint64_t)s_head[0] | ((uint64_t)s_head[1] << 32);
    const uint32_t r0 = s_head[2];
    // LDS frame 0 is the first frame the tile's first output reads; the last output reads up to frame last_off + T - 1
    const int64_t rel_base = call.rel_e + (int64_t)q0 - (int64_t)a.half + 1;
    const uint32_t last_off = (r0 + (n_out - 1) * M) / L;
    const uint32_t span = last_off + T;  // <= (tile - 1) * M / L + 1 + T: what the launch sized the staging for
    const uint32_t n = span * C;
    const auto stage = [&](uint32_t idx, float value) {
        const uint32_t fr = idx / C, c = idx - fr * C;
        s_x[rs_staged_at<C>(fr, c, span)] = value;
    };
    if (rel_base >= 0 && rel_base + (int64_t)span <= (int64_t)call.frames) {
        // Every tile but the call's first and last few: the reach is one contiguous run of d_in.  Aligned 16-byte loads, four in flight
        // per thread before the first is used (one dependent load after the other, each waiting out its trip to memory, cost more than
        // the taps); the floats outside the aligned body as dwords.
        const float* src = a.in + ((uint64_t)s * a.frames_capacity + (uint64_t)rel_base) * C;
        const uint32_t peel = min(n, ps_to_aligned(src));
        const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
        if (tid < peel) stage(tid, src[tid]);
        else if (tid >= 4 && tid < 4 + tail) stage(peel + 4 * nvec + (tid - 4), src[peel + 4 * nvec + (tid - 4)]);
        for (uint32_t v0 = 0; v0 < nvec; v0 += 4 * kRsThreads) {
            v4f v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t i = v0 + u * kRsThreads + tid;
                v[u] = i < nvec ? *reinterpret_cast<const v4f*>(src + peel + 4 * i) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t i = v0 + u * kRsThreads + tid, idx = peel + 4 * i;
                if (i < nvec) {
                    stage(idx, v[u].x);
                    stage(idx + 1, v[u].y);
                    stage(idx + 2, v[u].z);
                    stage(idx + 3, v[u].w);
                }
            }
        }
    } else {
        // (no emitted frame reaches further back than the ring's T - 1 frames: the header's STREAMING)
        for (uint32_t idx = tid; idx < n; idx += kRsThreads) stage(idx, ps_ring_x_at(a, call, s, rel_base + (int64_t)(idx / C), idx % C));
    }
    __syncthreads();

    PsTally tally;
    if (tid < n_out) {
        const uint32_t v = r0 + tid * M, off = v / L, p = v - off * L;
        const float* h = a.table + p * 4;  // [T / 4][L][4]: taps k .. k + 3 of phase p
        float acc[4][C];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[j][c] = 0.0f;
        for (uint32_t k = 0; k < T; k += 4) {
            const v4f hv = *reinterpret_cast<const v4f*>(h + (uint64_t)k * L);
            const float hj[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xf[C];
                rs_load_frame<C>(s_x, off + k + j, span, xf);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float prod = hj[j] * xf[c];
                    acc[j][c] = acc[j][c] + prod;
                }
            }
        }
        float y[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            y[c] = (acc[0][c] + acc[1][c]) + (acc[2][c] + acc[3][c]);
            tally.take(y[c]);
        }
        float* out = a.out + ((uint64_t)s * a.out_capacity + first + tid) * C;
        const uintptr_t base = reinterpret_cast<uintptr_t>(a.out);
        if (C % 4 == 0 && (base & 15u) == 0) {
#pragma unroll
            for (int i = 0; i + 3 < C; i += 4) *reinterpret_cast<v4f*>(out + i) = v4f{y[i], y[i + 1], y[i + 2], y[i + 3]};
        } else if (C % 2 == 0 && (base & 7u) == 0) {
#pragma unroll
            for (int i = 0; i + 1 < C; i += 2) *reinterpret_cast<v2f*>(out + i) = v2f{y[i], y[i + 1]};
        } else {
#pragma unroll
            for (int i = 0; i < C; ++i) out[i] = y[i];
        }
    }
    tally.fold_workgroup<kRsThreads>();
    if (tid == 0) tally.commit(a.records + s);
}

// ---- carry: frame n of the stream at slot n mod (T - 1) of its ring
__global__ __launch_bounds__(256) void rs_carry_kernel(RsArgs a, uint32_t s_base) {
    const uint32_t s = s_base + blockIdx.y;
    const RsStreamCall call = a.calls[s];
    const uint32_t C = a.channels;
    ps_carry_row(a.ring + (uint64_t)s * a.history * C, a.history, C, call.ring, call.frames, blockIdx.x * 256 + threadIdx.x,
                 [&](uint64_t rel, uint32_t c) { return a.in[((uint64_t)s * a.frames_capacity + rel) * C + c]; });
}

template <int C>
void rs_launch_main(const RsArgs& a, uint32_t tiles, size_t lds, hipStream_t stream) {
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(rs_main_kernel<C>, dim3(tiles, count), dim3(kRsThreads), lds, stream, a, base);
    });
}

}  // namespace

void launch_rs_begin(const RsArgs& a, bool whole_call, hipStream_t stream) {
    ps_launch_per_stream(rs_begin_kernel, a.n_streams, stream, a, whole_call ? 1u : 0u);
}
void launch_rs_finish(const RsArgs& a, hipStream_t stream) {
    ps_launch_per_stream(rs_finish_kernel, a.n_streams, stream, a);
}
void launch_rs_main(const RsArgs& a, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)(((uint64_t)a.max_emit + a.tile - 1) / a.tile);
    const size_t lds = ((size_t)((uint64_t)(a.tile - 1) * a.M / a.L) + 1 + a.taps) * a.channels * sizeof(float);
    switch (a.channels) {
        case 1: rs_launch_main<1>(a, tiles, lds, stream); break;
        case 2: rs_launch_main<2>(a, tiles, lds, stream); break;
        case 3: rs_launch_main<3>(a, tiles, lds, stream); break;
        case 4: rs_launch_main<4>(a, tiles, lds, stream); break;
        case 5: rs_launch_main<5>(a, tiles, lds, stream); break;
        case 6: rs_launch_main<6>(a, tiles, lds, stream); break;
        case 7: rs_launch_main<7>(a, tiles, lds, stream); break;
        default: rs_launch_main<8>(a, tiles, lds, stream); break;
    }
}
void launch_rs_carry(const RsArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.history * a.channels + 255) / 256;
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(rs_carry_kernel, dim3(tiles, count), dim3(256), 0, stream, a, base);
    });
}

}  // namespace omx

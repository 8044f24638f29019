// Channel remix of the programme loudness bank (include/omx/program_remix.h states the definition, program_remix.hpp the passes).
//
// The pass is bandwidth bound: (channels_in + channels_out) * 4 bytes per frame and a handful of multiply-adds.  A frame is
// 4 * channels bytes, another size on each side, and a row's base is only 4-byte aligned (3 channels x 1001 frames), so a frame does
// not stay inside one 16-byte vector of either buffer.  Both buffers therefore go through LDS:
//
//   main   : grid (tile of 256 * FPT frames, stream; FPT frames per thread, rm_frames_per_thread of the channel pair).  A tile wholly beyond frames[s] leaves after reading its stream's 16-byte call
//            entry.
//     in     the tile's input is one contiguous run of d_in.  The floats in front of the first 16-byte boundary (up to 3) and behind
//            the last one go by dword, the body by aligned 16-byte loads, all of a thread's loads issued before the first is used.
//            Float j of the run lands at s_x[(j / CI) * SI + j % CI], SI = CI | 1: a frame stride of an odd number of dwords.  A thread
//            reads ONE channel of ITS frame at a time (below), so the 32 lanes of a ds_read_b32 group read 32 addresses SI dwords
//            apart, which an odd SI spreads over all 32 banks; interleaved as in memory (SI = CI) an even channel count collides,
//            8 channels eight ways.  (The resampler, whose threads read whole frames, splits 8 channels into two planes of four for
//            ds_read_b128; a thread here never wants a whole frame, because of the next point.)
//     mix    the matrix is uniform over the workgroup.  The host compacted it into per-output term lists (RmMatrix); the workgroup
//            copies the header and the terms in use to LDS, and every thread walks the same list for each output with the term's
//            channel and coefficient in scalar registers: a skipped coefficient costs nothing and no sample is indexed by a value a
//            register holds (which would send the frame to scratch).  The first term of a list is a product, every later one a
//            product THEN a sum (the library is built with -ffp-contract=off), an empty list gives +0.0f: the header's DEFINITION.
//            A thread mixes FPT frames, 256 frames apart, under one walk.
//     out    out[f][o] goes to s_y[f * SO + o]; SO = channels_out, but channels_out + 1 for 4 and 8 channels (the dword stores of a
//            group would collide 4 and 8 ways; with 2 or 6 they collide 2 ways, which a ds_write_b32 absorbs).  The tile's output is
//            one contiguous run of d_out and leaves like the input came: head and tail by dword, the body in aligned 16-byte stores.
//     reduce PsTally (program_stage_device.hpp): count and maximum per thread, six shuffle steps, four wavefronts through LDS, at
//            most one atomicAdd (u64) and one atomicMax (bit pattern) per workgroup.
//   Templated on channels_in (and the frames per thread that go with it), not on channels_out: the input staging divides every
//   float's index by the channel count, which has to be a constant to be cheap, while channels_out only bounds a uniform loop and
//   strides the output staging (a shift for 4 and 8).  Fourteen instantiations; DESIGN.md lists their registers, LDS and scratch.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_remix.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void rm_begin_kernel(RmArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const RmStreamCall c = a.calls[s];
    omx_program_remix_record r;
    r.frames = c.frames;
    r.samples_over = 0;
    r.out_sample_peak = 0.0f;
    r.out_sample_peak_db = a.floor_db;
    r.matrix_index = c.matrix;
    r.terms = c.terms;
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void rm_finish_kernel(RmArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    a.records[s].out_sample_peak_db = ps_peak_db(a.records[s].out_sample_peak, a.floor_db);
}

__device__ __forceinline__ uint32_t rm_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

template <int CI, int FPT>
__global__ __launch_bounds__(kRmThreads) void rm_main_kernel(RmArgs a, uint32_t s_base) {
    constexpr uint32_t kTile = kRmThreads * FPT;                   // frames of a tile
    extern __shared__ __attribute__((aligned(16))) float s_mem[];  // s_x [kTile][SI], s_y [kTile][SO] (+ shift)
    __shared__ uint32_t s_tm[kRmHeaderDwords + 2 * kRmMaxTerms];   // the matrix in use, as RmMatrix lays it out
    constexpr uint32_t SI = rm_in_stride(CI);
    const uint32_t s = s_base + blockIdx.y, tid = threadIdx.x;
    const RmStreamCall call = a.calls[s];
    const uint64_t first = (uint64_t)blockIdx.x * kTile;
    if (first >= call.frames) return;  // (uniform over the workgroup: no thread is left at a barrier below)
    const uint32_t nf = (uint32_t)min((uint64_t)kTile, (uint64_t)call.frames - first);
    const uint32_t CO = a.channels_out;
    const bool padded = CO == 4 || CO == 8;
    const uint32_t SO = rm_out_stride(CO), co_shift = CO == 8 ? 3 : 2;
    float* s_x = s_mem;
    float* s_y = s_mem + kTile * SI;
    // The tile's run of d_out, and where float j of it is staged.  Unpadded, the staging is shifted by up to three floats so that the
    // run's first aligned 16-byte vector is an aligned 16 bytes of LDS as well: the body then leaves LDS in ds_read_b128.
    float* dst = a.out + ((uint64_t)s * a.frames_capacity + first) * CO;
    const uint32_t n_out = nf * CO, peel_out = min(n_out, ps_to_aligned(dst));
    const uint32_t y_shift = padded ? 0u : (4u - peel_out) & 3u;
    const auto y_at = [&](uint32_t j) { return padded ? (j >> co_shift) * SO + (j & (CO - 1)) : y_shift + j; };

    {   // ---- in: the matrix, and the tile's run of d_in
        const uint32_t* tm = reinterpret_cast<const uint32_t*>(a.matrices + call.matrix);
        if (tid < kRmHeaderDwords + 2 * call.terms) s_tm[tid] = tm[tid];  // (at most 140 dwords)
        const float* src = a.in + ((uint64_t)s * a.frames_capacity + first) * CI;
        const uint32_t n = nf * CI;
        const auto stage = [&](uint32_t j, float value) {
            const uint32_t fr = j / CI;
            s_x[fr * SI + (j - fr * CI)] = value;
        };
        const uint32_t peel = min(n, ps_to_aligned(src));
        const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
        if (tid < peel) stage(tid, src[tid]);  // threads 0 .. 2 the head, threads 4 .. 6 the tail
        else if (tid >= 4 && tid < 4 + tail) stage(peel + 4 * nvec + (tid - 4), src[peel + 4 * nvec + (tid - 4)]);
        constexpr uint32_t kInFlight = (kTile * CI / 4 + kRmThreads - 1) / kRmThreads;  // every vector of a full tile in one round
        v4f v[kInFlight];
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; ++u) {
            const uint32_t i = u * kRmThreads + tid;
            if (i < nvec) v[u] = *reinterpret_cast<const v4f*>(src + peel + 4 * i);
        }
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; ++u) {
            const uint32_t i = u * kRmThreads + tid, j = peel + 4 * i;
            if (i < nvec) {
                stage(j, v[u].x);
                stage(j + 1, v[u].y);
                stage(j + 2, v[u].z);
                stage(j + 3, v[u].w);
            }
        }
    }
    __syncthreads();

    // ---- mix: frames tid, tid + 256, .. of the tile (a thread without a frame walks along on frame 0 and keeps nothing)
    PsTally tally;
    uint32_t at_x[FPT], at_y[FPT];
    bool live[FPT];
#pragma unroll
    for (uint32_t k = 0; k < FPT; ++k) {
        const uint32_t f = k * kRmThreads + tid;
        live[k] = f < nf;
        at_x[k] = (live[k] ? f : 0u) * SI;
        at_y[k] = y_at((live[k] ? f : 0u) * CO);
    }
    for (uint32_t o = 0; o < CO; ++o) {
        const uint32_t t0 = rm_uniform(s_tm[o]), t1 = rm_uniform(s_tm[o + 1]);
        float acc[FPT];
#pragma unroll
        for (uint32_t k = 0; k < FPT; ++k) acc[k] = 0.0f;
        if (t0 < t1) {
            const uint32_t in0 = rm_uniform(s_tm[kRmHeaderDwords + 2 * t0]);
            const float coef0 = __uint_as_float(rm_uniform(s_tm[kRmHeaderDwords + 2 * t0 + 1]));
#pragma unroll
            for (uint32_t k = 0; k < FPT; ++k) acc[k] = coef0 * s_x[at_x[k] + in0];
            for (uint32_t t = t0 + 1; t < t1; ++t) {
                const uint32_t in = rm_uniform(s_tm[kRmHeaderDwords + 2 * t]);
                const float coef = __uint_as_float(rm_uniform(s_tm[kRmHeaderDwords + 2 * t + 1]));
#pragma unroll
                for (uint32_t k = 0; k < FPT; ++k) {
                    const float prod = coef * s_x[at_x[k] + in];
                    acc[k] = acc[k] + prod;
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < FPT; ++k) {
            if (live[k]) {
                tally.take(acc[k]);
                s_y[at_y[k] + o] = acc[k];
            }
        }
    }
    __syncthreads();

    {   // ---- out: the tile's run of d_out
        const uint32_t n = n_out, peel = peel_out;
        const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
        if (tid < peel) dst[tid] = s_y[y_at(tid)];
        else if (tid >= 4 && tid < 4 + tail) dst[peel + 4 * nvec + (tid - 4)] = s_y[y_at(peel + 4 * nvec + (tid - 4))];
        for (uint32_t i = tid; i < nvec; i += kRmThreads) {
            const uint32_t j = peel + 4 * i;
            v4f v;
            if (padded) v = v4f{s_y[y_at(j)], s_y[y_at(j + 1)], s_y[y_at(j + 2)], s_y[y_at(j + 3)]};
            else v = *reinterpret_cast<const v4f*>(s_y + y_shift + j);
            *reinterpret_cast<v4f*>(dst + j) = v;
        }
    }

    tally.fold_workgroup<kRmThreads>();
    if (tid == 0) tally.commit(a.records + s);
}

template <int CI, int FPT>
void rm_launch_tiles(const RmArgs& a, hipStream_t stream) {
    constexpr uint32_t kTile = kRmThreads * FPT;
    const uint64_t tiles = std::max<uint64_t>(((uint64_t)a.max_frames + kTile - 1) / kTile, 1);
    const size_t lds = ((size_t)kTile * (rm_in_stride(CI) + rm_out_stride(a.channels_out)) + 4) * sizeof(float);  // (+ 4: the output's shift)
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL((rm_main_kernel<CI, FPT>), dim3((uint32_t)tiles, count), dim3(kRmThreads), lds, stream, a, base);
    });
}

// the tile of the pair (rm_frames_per_thread): 8, 4 or 2 frames per thread with up to 2 input channels, 4 or 2 with up to 4, else 2
template <int CI>
void rm_launch_main(const RmArgs& a, hipStream_t stream) {
    const uint32_t fpt = rm_frames_per_thread(CI, a.channels_out);
    if constexpr (CI <= 2) {
        if (fpt == 8) return rm_launch_tiles<CI, 8>(a, stream);
    }
    if constexpr (CI <= 4) {
        if (fpt == 4) return rm_launch_tiles<CI, 4>(a, stream);
    }
    rm_launch_tiles<CI, 2>(a, stream);
}

}  // namespace

void launch_rm_begin(const RmArgs& a, hipStream_t stream) {
    ps_launch_per_stream(rm_begin_kernel, a.n_streams, stream, a);
}
void launch_rm_finish(const RmArgs& a, hipStream_t stream) {
    ps_launch_per_stream(rm_finish_kernel, a.n_streams, stream, a);
}
void launch_rm_main(const RmArgs& a, hipStream_t stream) {
    switch (a.channels_in) {
        case 1: rm_launch_main<1>(a, stream); break;
        case 2: rm_launch_main<2>(a, stream); break;
        case 3: rm_launch_main<3>(a, stream); break;
        case 4: rm_launch_main<4>(a, stream); break;
        case 5: rm_launch_main<5>(a, stream); break;
        case 6: rm_launch_main<6>(a, stream); break;
        case 7: rm_launch_main<7>(a, stream); break;
        default: rm_launch_main<8>(a, stream); break;
    }
}

}  // namespace omx

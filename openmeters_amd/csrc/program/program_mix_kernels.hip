// Mix pass of the programme loudness bank (include/omx/program_mix.h states the definition, program_mix.hpp the passes,
// program_mix_plan.hpp the spans).
//
// The pass moves 4 B written per bus sample and 4 B read per send that covers it; per 4 B read it runs one f32 -> f64 convert and one
// f64 multiply-add, and per 4 B written one f64 -> f32 convert.
//   main   : grid (tile of mx_tile_frames(C) frames of the bus window, bus), 256 threads, templated on the channel count C.
//            A tile wholly beyond out_frames[o] leaves after reading its bus's 48-byte call entry.
//     spans  the bus's spans are sorted and tile [0, 2^40): a binary search finds the one that holds the tile's first frame, and the
//            tile walks on from there, as ed_main_kernel does.
//     run    the part of a span inside the tile is one contiguous run of d_out, stored the way the edit pass stores it: the floats in
//            front of its first 16-byte boundary (up to 3) and behind the last one go by dword (threads 0 .. 2 and 4 .. 6), the body
//            in aligned 16-byte stores.  A source of a run is a contiguous run of d_in at ANY 4-byte offset against the output.
//            The source says four dword loads per vector at 4-byte alignment; the compiler makes ONE global_load_dwordx4 of them,
//            which gfx950 takes at any 4-byte offset, so there is one load form, not two (a branch on the source's alignment
//            compiled to the same instruction on both sides and was taken out).  A run without a whole aligned vector is its
//            edge floats alone (a uniform choice between two instantiations of the run).
//     tables the call entry, the spans, the index list and the send entries are read through the constant address space
//            (mx_table_load): scalar loads.  Through a plain pointer they became VECTOR loads behind the first store to d_out (the
//            compiler cannot rule out that the store aliases them), each with a wait for every load in flight.
//     layers in batches of kMxLayersPerBatch (4).  The first batch reads its four list entries together, then its four send
//            entries together (two scalar round trips).  Every batch issues all its data loads back to back (its layers x the
//            thread's two vectors and its edge float: twelve vector loads), then the scalar loads of the NEXT batch's entries,
//            and only then adds; an empty asm statement over the loaded registers keeps the compiler from sinking the loads of
//            layers 1 .. 3 behind the adds of the layer before.  No wait sits between the data loads of a batch.  A batch
//            with fewer layers than 4 loads its last layer again and adds nothing of it (the choice is uniform: no load sits
//            under a per-thread branch, and a thread without a vector or an edge float loads the run's last vector or first
//            float again and keeps nothing).  The f64 accumulators (two vectors of four, one
//            edge) are named registers that live across the batches; every array below is indexed by unrolled loop counters only.
//            An accumulator starts at -0.0, the identity of IEEE addition for every operand, so the first layer needs no other
//            code than the rest: -0.0 + g x is g x on bits (a NaN's bits are not defined).  The products are exact in f64, so the
//            explicit fma below gives what the header's "product, then sum" gives.
//     zero   a span with no layer stores +0.0f without a load.
//     reduce PsTally (program_stage_device.hpp) for samples_over and the peak; samples_nonfinite is counted beside it, folded in the
//            same six shuffle steps and around the same barrier, and committed with one more atomicAdd per workgroup at the most.
//   The record's counts (silent and mixed frames, sends, max_layers) follow from the spans and the window: the host puts them into
//   the call entry and the begin kernel writes them.  Scalar loads for the tables, vector loads for PCM, vector stores and vector
//   atomics only; DESIGN.md lists registers, LDS and scratch per instantiation.
#include "program_mix.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void mx_begin_kernel(MxArgs a) {
    const uint32_t o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.n_out) return;
    MxBusCall c{};
    if (a.calls) c = a.calls[o];
    omx_program_mix_record r;
    r.out_first = c.out_first;
    r.frames = c.out_frames;
    r.silent_frames = c.silent_frames;
    r.mixed_frames = c.mixed_frames;
    r.samples_over = 0;
    r.samples_nonfinite = 0;
    r.out_sample_peak = 0.0f;
    r.out_sample_peak_db = a.floor_db;
    r.sends = c.sends;
    r.max_layers = c.max_layers;
    a.records[o] = r;
}

__global__ __launch_bounds__(64) void mx_finish_kernel(MxArgs a) {
    const uint32_t o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.n_out) return;
    a.records[o].out_sample_peak_db = ps_peak_db(a.records[o].out_sample_peak, a.floor_db);
}

// what a thread has stored: the family's tally, and the samples that are NaN or infinite
struct MxTally {
    PsTally ps;
    uint32_t nonfinite = 0;
    __device__ __forceinline__ void take(float y) {
        ps.take(y);
        nonfinite += (__float_as_uint(y) & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
    }
};

// A load from the call's tables (entries, spans, index list, sends) at a uniform address.  The host uploads the tables in front of
// the launch and no kernel writes them, so they may be read through the constant address space: the compiler then issues scalar
// loads, which a kernel that has already stored to d_out would otherwise not get (a plain pointer may alias the stores).
template <class T>
__device__ __forceinline__ T mx_table_load(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(4))) T*)(reinterpret_cast<uintptr_t>(p));
#else
    return *p;
#endif
}

__device__ __forceinline__ double mx_mac(float g, float x, double acc) { return __builtin_fma((double)g, (double)x, acc); }

// One run under n_layers >= 1 sends: n floats at d (n >= 1), the first of them channel 0 of absolute bus frame `frame`.  BODY: the
// run holds at least one aligned 16-byte vector (uniform; a run without one is its edge floats alone and loads no vector).
template <int C, bool BODY>
__device__ __forceinline__ void mx_run_layers(float* d, uint32_t n, uint64_t frame, const uint32_t* list, uint32_t n_layers, const MxArgs& a,
                                       MxTally& tally) {
    constexpr uint32_t K = mx_in_flight(C), B = kMxLayersPerBatch;
    const uint32_t tid = threadIdx.x;
    const uint32_t peel = min(n, ps_to_aligned(d));
    const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
    // the float outside the aligned body this thread stores, if any: threads 0 .. 2 the head, threads 4 .. 6 the tail
    uint32_t e = n;
    if (tid < peel) e = tid;
    else if (tid >= 4 && tid < 4 + tail) e = peel + 4 * nvec + (tid - 4);
    const uint32_t ec = e < n ? e : 0u;
    // the thread's vectors of the body; one beyond the body is the body's last again (nvec != 0 wherever it is read)
    uint32_t at[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) at[k] = peel + 4 * min(k * kMxThreads + tid, nvec - 1);

    double acc_e = -0.0;
    double acc[K][4];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = -0.0;

    // The table entries of a batch: its list entries together, then its send entries together, all by scalar loads (the addresses
    // are uniform and no kernel writes the tables).  The first batch's are read here; inside the loop the NEXT batch's are read
    // behind the current batch's data loads, so that from the second batch on no data load waits for a table entry.
    MxSend s[B];
    {
        uint32_t idx[B];
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) idx[j] = mx_table_load(list + min(j, n_layers - 1));
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) s[j] = mx_table_load(a.sends + idx[j]);
    }
    for (uint32_t l0 = 0; l0 < n_layers; l0 += B) {
        float g[B], xe[B];
        v4f x[B][K];
        // ---- every data load of the batch, back to back.  A vector is read as four dwords at 4-byte alignment: the compiler makes
        // one dwordx4 of them, which the hardware takes at any 4-byte offset.
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            g[j] = s[j].gain;
            const float* src = a.in + (s[j].src_base + (frame - s[j].dst_first)) * C;
            xe[j] = src[ec];
            if (BODY) {
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) {
                    const float* p = src + at[k];
                    x[j][k] = v4f{p[0], p[1], p[2], p[3]};
                }
            }
        }
        // ---- the next batch's table entries (the last layer's again where there is no next batch: always a valid index)
        MxSend sn[B];
        {
            uint32_t idx[B];
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) idx[j] = mx_table_load(list + min(l0 + B + j, n_layers - 1));
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) sn[j] = mx_table_load(a.sends + idx[j]);
        }
        // Every load above is issued before the first add below: without this fence the compiler sinks the loads of layers 1 .. 3
        // under the uniform `l0 + j < n_layers` of their adds, behind the adds of the layer before.
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            asm volatile("" : "+v"(xe[j]));
#pragma unroll
            for (uint32_t k = 0; BODY && k < K; ++k) asm volatile("" : "+v"(x[j][k]));
        }
        // ---- the batch's adds, in table order
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            if (l0 + j < n_layers) {  // uniform
                acc_e = mx_mac(g[j], xe[j], acc_e);
#pragma unroll
                for (uint32_t k = 0; BODY && k < K; ++k) {
                    acc[k][0] = mx_mac(g[j], x[j][k].x, acc[k][0]);
                    acc[k][1] = mx_mac(g[j], x[j][k].y, acc[k][1]);
                    acc[k][2] = mx_mac(g[j], x[j][k].z, acc[k][2]);
                    acc[k][3] = mx_mac(g[j], x[j][k].w, acc[k][3]);
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) s[j] = sn[j];
    }

    if (e < n) {
        const float y = (float)acc_e;
        tally.take(y);
        d[e] = y;
    }
    if (BODY) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) {
            if (k * kMxThreads + tid < nvec) {
                const v4f y = v4f{(float)acc[k][0], (float)acc[k][1], (float)acc[k][2], (float)acc[k][3]};
                tally.take(y.x);
                tally.take(y.y);
                tally.take(y.z);
                tally.take(y.w);
                *reinterpret_cast<v4f*>(d + at[k]) = y;
            }
        }
    }
}

template <int C>
__device__ __forceinline__ void mx_run(float* d, uint32_t n, uint64_t frame, const uint32_t* list, uint32_t n_layers, const MxArgs& a,
                                       MxTally& tally) {
    if (n - min(n, ps_to_aligned(d)) >= 4) mx_run_layers<C, true>(d, n, frame, list, n_layers, a, tally);
    else mx_run_layers<C, false>(d, n, frame, list, n_layers, a, tally);
}

// One run under no send: +0.0f, no load
template <int C>
__device__ __forceinline__ void mx_zero(float* d, uint32_t n) {
    constexpr uint32_t K = mx_in_flight(C);
    const uint32_t tid = threadIdx.x;
    const uint32_t peel = min(n, ps_to_aligned(d));
    const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
    if (tid < peel) d[tid] = 0.0f;
    else if (tid >= 4 && tid < 4 + tail) d[peel + 4 * nvec + (tid - 4)] = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t v = k * kMxThreads + tid;
        if (v < nvec) *reinterpret_cast<v4f*>(d + peel + 4 * v) = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

template <int C>
__global__ __launch_bounds__(kMxThreads) void mx_main_kernel(MxArgs a, uint32_t o_base) {
    constexpr uint32_t kTile = mx_tile_frames(C);
    const uint32_t o = o_base + blockIdx.y;
    const MxBusCall call = mx_table_load(a.calls + o);
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;  // the tile's first frame inside the window
    if (t0 >= call.out_frames) return;  // (uniform over the workgroup: no thread is left at the barrier of the tally)
    const uint32_t nf = (uint32_t)min((uint64_t)kTile, (uint64_t)call.out_frames - t0);
    const uint64_t first = call.out_first + t0, last = first + nf;  // absolute bus frames
    float* row = a.out + (uint64_t)o * a.out_capacity * C;
    const MxSpan* sp = a.spans + call.span_begin;
    uint32_t lo = 0, hi = call.span_count;  // sp[lo].first <= first (span 0 starts at frame 0), sp[hi].first > first
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mx_table_load(&sp[mid].first) <= first) lo = mid;
        else hi = mid;
    }
    MxTally tally;
    for (uint32_t i = lo; i < call.span_count; ++i) {
        const MxSpan s = mx_table_load(sp + i);
        if (s.first >= last) break;
        const uint64_t ra = max(first, s.first), rb = min(last, s.end);
        if (ra >= rb) continue;
        const uint32_t n = (uint32_t)(rb - ra) * C;
        float* d = row + (ra - call.out_first) * C;
        if (s.n_layers == 0) mx_zero<C>(d, n);
        else mx_run<C>(d, n, ra, a.list + s.list_begin, s.n_layers, a, tally);
    }
    // the folds: one loop of shuffles for the three values, one barrier
    __shared__ uint32_t s_nonfinite[kMxThreads / 64];
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        tally.ps.fold_step(step);
        ps_fold_step(tally.nonfinite, PsSum{}, step);
    }
    ps_fold_post(tally.nonfinite, s_nonfinite);
    tally.ps.fold_waves<kMxThreads>();  // (holds the barrier)
    if (threadIdx.x == 0) {
        ps_fold_gather<kMxThreads>(tally.nonfinite, PsSum{}, s_nonfinite);
        tally.ps.commit(a.records + o);
        if (tally.nonfinite != 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(&a.records[o].samples_nonfinite), (unsigned long long)tally.nonfinite);
    }
}

template <int C>
void mx_launch_main(const MxArgs& a, hipStream_t stream) {
    constexpr uint32_t kTile = mx_tile_frames(C);
    const uint64_t tiles = std::max<uint64_t>(((uint64_t)a.max_frames + kTile - 1) / kTile, 1);
    for_stream_slabs(a.n_out, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(mx_main_kernel<C>, dim3((uint32_t)tiles, count), dim3(kMxThreads), 0, stream, a, base);
    });
}

}  // namespace

void launch_mx_begin(const MxArgs& a, hipStream_t stream) {
    ps_launch_per_stream(mx_begin_kernel, a.n_out, stream, a);
}
void launch_mx_finish(const MxArgs& a, hipStream_t stream) {
    ps_launch_per_stream(mx_finish_kernel, a.n_out, stream, a);
}
void launch_mx_main(const MxArgs& a, hipStream_t stream) {
    switch (a.channels) {
        case 1: mx_launch_main<1>(a, stream); break;
        case 2: mx_launch_main<2>(a, stream); break;
        case 3: mx_launch_main<3>(a, stream); break;
        case 4: mx_launch_main<4>(a, stream); break;
        case 5: mx_launch_main<5>(a, stream); break;
        case 6: mx_launch_main<6>(a, stream); break;
        case 7: mx_launch_main<7>(a, stream); break;
        default: mx_launch_main<8>(a, stream); break;
    }
}

}  // namespace omx

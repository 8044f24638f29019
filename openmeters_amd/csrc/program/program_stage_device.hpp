// What the kernels of the programme bank's stages share: the dB figure of a power, the distance to the next 16-byte boundary, the
// folds of a per-thread value over a wavefront and a workgroup, the tally of a pass's output (samples over full scale, sample peak)
// with its commit to the stream's record, the ring read, the carry and the record begin of the stages that carry state between calls,
// the launch of a per-stream kernel and the launch loop over slabs of streams.  Include from .hip files only.
#pragma once
#include "../common.hpp"
#include "program_carried.hpp"

namespace omx {

__device__ __forceinline__ float power_to_db(float power, float floor) {  // level.rs:28-34
    return power > 0.0f ? fmaxf(logf(power) * 4.3429448f, floor) : floor;
}
// what a finish kernel does to a record: the dB field of a linear peak (or envelope)
__device__ __forceinline__ float ps_peak_db(float peak, float floor) { return power_to_db(peak * peak, floor); }

__device__ __forceinline__ uint32_t ps_to_aligned(const float* p) {  // floats up to the next 16-byte boundary
    return ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
}

// ---- folds.  Sums of uint32_t, maxima and minima do not depend on the order they are formed in.
struct PsSum {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct PsMax {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return b > a ? b : a; }
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }  // a NaN operand is ignored
};
struct PsMin {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }  // a NaN operand is ignored
};

// One step of a wavefront's fold.  The fold is the six steps d = 32, 16 .. 1, after which every lane holds the wavefront's value; a
// kernel that folds several values takes them through ONE loop, a step of each per trip, so that the shuffles of a trip are in
// flight together (one value after the other waits out twice the shuffles: 3.5 % on the 2 -> 1 remix of 1024 x 16 384 frames).
template <class T, class Op>
__device__ __forceinline__ void ps_fold_step(T& v, Op op, int d) {
    v = op(v, __shfl_xor(v, d));
}
// The wavefronts' values to the workgroup's, around ONE __syncthreads() of the caller however many values it folds: every thread
// posts (lane 0 of a wavefront writes its slot of `part`, one per wavefront), the barrier, thread 0 gathers the other wavefronts'.
template <class T>
__device__ __forceinline__ void ps_fold_post(T v, T* part) {
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
}
template <uint32_t THREADS, class T, class Op>
__device__ __forceinline__ void ps_fold_gather(T& v, Op op, const T* part) {
    for (uint32_t w = 1; w < THREADS / 64; ++w) v = op(v, part[w]);
}

// ---- the tally of a pass's output samples
struct PsTally {
    uint32_t over = 0;  // samples with |y| > 1
    float peak = 0.0f;  // the largest |y|

    __device__ __forceinline__ void take(float y) {
        const float m = fabsf(y);
        over += m > 1.0f ? 1u : 0u;  // false for NaN, true for infinity
        peak = fmaxf(peak, m);       // a NaN operand is ignored
    }
    __device__ __forceinline__ void fold_step(int d) {
        ps_fold_step(over, PsSum{}, d);
        ps_fold_step(peak, PsMax{}, d);
    }
    __device__ __forceinline__ void fold_wave() {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) fold_step(d);
    }
    // Behind the wavefronts' folds, called by every thread of a workgroup of THREADS (it holds a barrier): thread 0 ends with the
    // workgroup's tally.
    template <uint32_t THREADS>
    __device__ __forceinline__ void fold_waves() {
        __shared__ uint32_t s_over[THREADS / 64];
        __shared__ float s_peak[THREADS / 64];
        ps_fold_post(over, s_over);
        ps_fold_post(peak, s_peak);
        __syncthreads();
        if (threadIdx.x == 0) {
            ps_fold_gather<THREADS>(over, PsSum{}, s_over);
            ps_fold_gather<THREADS>(peak, PsMax{}, s_peak);
        }
    }
    template <uint32_t THREADS>
    __device__ __forceinline__ void fold_workgroup() {
        fold_wave();
        fold_waves<THREADS>();
    }
    // Thread 0, behind fold_workgroup: at most ONE atomicAdd (u64) and ONE atomicMax per workgroup into the stream's record, which
    // the stage's begin kernel cleared on the same stream.  The maximum goes by the bit pattern of the non-negative float, which
    // orders like the value; fmaxf never lets a NaN in.
    template <class Record>
    __device__ __forceinline__ void commit(Record* r) const {
        if (over != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->samples_over), (unsigned long long)over);
        if (peak > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&r->out_sample_peak), __float_as_uint(peak));
    }
};

// ---- what the stages that carry state between calls share (program_carried.hpp holds the host's half).  `rel` counts a stream's
// frames from the first frame of the call; a ring of `length` entries holds entry n of the stream at slot n mod length, and a call's
// table hands over `ring`, the slot of the call's first entry.

// Sample (frame rel, channel c) of stream s for a stage whose ring holds the `history` frames in front of the call: +0 in front of the
// stream, at and beyond the last frame taken (which only a flush reads) and further back than the ring reaches (which nothing the stage
// emits reads), the call's PCM at rel >= 0, the ring below.  Args: in, frames_capacity, channels, history, ring; Call: n_old, frames, ring.
template <class Args, class Call>
__device__ __forceinline__ float ps_ring_x_at(const Args& a, const Call& call, uint32_t s, int64_t rel, uint32_t c) {
    if ((int64_t)call.n_old + rel < 0 || rel >= (int64_t)call.frames) return 0.0f;
    if (rel >= 0) return a.in[((uint64_t)s * a.frames_capacity + (uint64_t)rel) * a.channels + c];
    if (rel < -(int64_t)a.history) return 0.0f;
    int64_t slot = (int64_t)call.ring + rel;
    if (slot < 0) slot += a.history;
    return a.ring[((uint64_t)s * a.history + (uint64_t)slot) * a.channels + c];
}

// A row into its ring, for thread e of the carry pass: element e of the newest min(frames, length) entries of the call's row (entries of
// `width` elements; fetch(rel, c) is element c of entry rel) goes to slot (ring + rel) mod length of `row`, the stream's ring.  The slots
// it does not write keep the older entries, so a call of fewer entries than the ring holds, or of none, leaves the newest `length` in place.
template <class T, class Fetch>
__device__ __forceinline__ void ps_carry_row(T* row, uint32_t length, uint32_t width, uint32_t ring, uint32_t frames, uint32_t e, Fetch&& fetch) {
    const uint32_t nx = min(frames, length);
    if (e < nx * width) {  // (never with length 0)
        const uint32_t fr = e / width, c = e - fr * width;
        const uint64_t rel = (uint64_t)(frames - nx) + fr;
        const uint64_t slot = ((uint64_t)ring + rel) % length;
        row[slot * width + c] = fetch(rel, c);
    }
}

// What a begin kernel writes of a whole call into the stream's record: the counters behind the call and the state
template <uint32_t IDLE, uint32_t RUNNING, uint32_t FLUSHED, class Record>
__device__ __forceinline__ void ps_begin_record(Record& r, uint64_t n_old, uint64_t e_old, uint32_t frames, uint32_t emit, uint32_t flags) {
    r.frames_in = n_old + frames;
    r.frames_out = e_old + emit;
    r.frames_written = emit;
    r.state = (flags & kCarryFlagFlush) ? FLUSHED : (r.frames_in != 0 ? RUNNING : IDLE);
}

// ---- launch of a kernel with one thread per stream (the begin and finish kernels): workgroups of 64
template <class... Params, class... Args>
void ps_launch_per_stream(void (*kernel)(Params...), uint32_t n_streams, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((n_streams + 63) / 64), dim3(64), 0, stream, args...);
}

// ---- launches of a (tiles, streams) grid.  A launch holds at most 65535 streams in y and fewer than 2^32 threads (workgroups of up
// to 256): launch(base, count) once per slab of streams.
template <class Launch>
void for_stream_slabs(uint32_t n_streams, uint64_t tiles, Launch&& launch) {
    const uint64_t slab = std::max<uint64_t>(std::min<uint64_t>(65535, ((1ull << 24) - 1) / tiles), 1);
    for (uint64_t base = 0; base < n_streams; base += slab) launch((uint32_t)base, (uint32_t)std::min<uint64_t>(slab, n_streams - base));
}

}  // namespace omx

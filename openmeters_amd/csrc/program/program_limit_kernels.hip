// Limiter of the programme loudness bank (include/omx/program_limit.h states the definition, program_limit.hpp the passes).
//
// Indices.  `rel` counts frames from the first frame of the call: frame n of the stream is rel = n - n_old.  Frames in front of the
// call (rel < 0) come from the rings the carry pass of the earlier calls wrote (x: the newest LA frames, q: the newest W + A - 2
// values), frames in front of the stream (n < 0) are x = 0 and q = 2^24, and so is q at and beyond the last frame taken, which only a
// flush reads.  A call emits frames f = 0 .. emit-1, frame f being x[rel = f - held], with the envelope S[rel = f - held + LA].
//
//   level  : grid (stream, tile of kLmLevelTile frames).  The tile and the 23 frames before it go to LDS per channel (coalesced dword
//            loads of the interleaved PCM: one contiguous run when the history lies inside the call), every thread takes four frames
//            a quarter of a tile apart (consecutive lanes read consecutive LDS words), two of them side by side as the lanes of the
//            packed multiplies and adds, and runs the interpolator chains of every channel in the order of program_peaks.h
//            (multiply, THEN add: the library is built with -ffp-contract=off), folds the channels with fmaxf and writes one u32 q
//            per frame.
//   hold   : grid (stream, tile of kLmHoldTile values).  q with a halo of L - 1 in LDS, the window minimum by doubling (windows 1, 2,
//            4 .. P <= L, then two overlapping windows of P), all in LDS.  L = min(W, kLmHoldMaxWindow); a longer W is the minimum of
//            W / L shifted windows and one at the far end, taken by the smooth pass as it loads.
//   smooth : grid (stream, tile of kLmSmoothTile frames).  w with a halo of A - 1 in LDS as u64, an exact prefix sum (a run per thread,
//            the run totals scanned), S = P[n] - P[n - A], Gf = (float)((double)S / (double)(A << 24)).
//   apply  : as pn_tile_kernel: the store address of the body is 16-byte aligned (tile 0 peels the floats outside it), loads are
//            dwords (the held frames come from the ring, the rest from d_in), one k = g * Gf per frame; counts are summed and maxima /
//            minima taken on bit patterns with at most one atomic of each kind per workgroup: order-free, so the record is deterministic.
//   carry  : the newest LA frames of PCM and the newest W + A - 2 values of q into the rings, behind the apply pass that read them.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_limit.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lm_x_at(const LmArgs& a, const LmStreamCall& call, uint32_t s, int64_t rel, uint32_t c) {
    if ((int64_t)call.n_old + rel < 0 || rel >= (int64_t)call.frames) return 0.0f;
    if (rel >= 0) return a.in[((uint64_t)s * a.frames_capacity + (uint64_t)rel) * a.channels + c];
    int64_t slot = (int64_t)call.ring_x + rel;  // rel >= -latency
    if (slot < 0) slot += a.latency;
    return a.ring_x[((uint64_t)s * a.latency + (uint64_t)slot) * a.channels + c];
}

__device__ __forceinline__ uint32_t lm_q_at(const LmArgs& a, const LmStreamCall& call, uint32_t s, int64_t rel) {
    if ((int64_t)call.n_old + rel < 0 || rel >= (int64_t)call.frames) return kLmUnity;
    if (rel >= 0) return a.q[(uint64_t)s * a.q_row + (uint64_t)rel];
    int64_t slot = (int64_t)call.ring_q + rel;  // rel >= -q_history
    if (slot < 0) slot += a.q_history;
    return a.ring_q[(uint64_t)s * a.q_history + (uint64_t)slot];
}

__device__ __forceinline__ omx_program_limit_record lm_idle_record(const LmArgs& a) {
    omx_program_limit_record r{};
    r.gain = 1.0f;
    r.ceiling = a.ceiling;
    r.min_envelope = 1.0f;
    r.out_sample_peak_db = a.floor_db;
    r.gain_index = OMX_PROGRAM_UNITY_GAIN;
    r.state = OMX_LIMIT_IDLE;
    r.latency_frames = a.latency;
    return r;
}

__global__ __launch_bounds__(64) void lm_begin_kernel(LmArgs a, uint32_t whole_call) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const LmStreamCall c = a.calls[s];
    omx_program_limit_record r = a.records[s];
    if (c.flags & kCarryFlagClear) r = lm_idle_record(a);
    if (c.flags & kLmFlagLatch) {
        r.gain = c.gain_index == OMX_PROGRAM_UNITY_GAIN ? 1.0f : a.gains[c.gain_index].gain;
        r.gain_index = c.gain_index;
    }
    if (whole_call) ps_begin_record<OMX_LIMIT_IDLE, OMX_LIMIT_RUNNING, OMX_LIMIT_FLUSHED>(r, c.n_old, c.n_old - c.held, c.frames, c.emit, c.flags);
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void lm_finish_kernel(LmArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    a.records[s].out_sample_peak_db = ps_peak_db(a.records[s].out_sample_peak, a.floor_db);
    a.records[s].max_reduction_db = -ps_peak_db(a.records[s].min_envelope, a.floor_db);
}

// ---- level
typedef float v2f __attribute__((ext_vector_type(2)));  // two independent f32 lanes of a v_pk_*_f32 instruction

// the levels of two frames of one channel, w0[-i] / w1[-i] = the samples i frames before them
template <int DL>
__device__ __forceinline__ v2f lm_pair_level(const LmArgs& a, const float* w0, const float* w1) {
    v2f x = v2f{w0[0], w1[0]};
    v2f vc = v2f{fabsf(x.x), fabsf(x.y)};
    if constexpr (DL == 12) {
        v2f o0 = x * v2f{a.fir4[0][0], a.fir4[0][0]}, o1 = x * v2f{a.fir4[0][1], a.fir4[0][1]}, o2 = x * v2f{a.fir4[0][2], a.fir4[0][2]};
#pragma unroll
        for (int i = 1; i < 12; ++i) {
            x = v2f{w0[-i], w1[-i]};
            const v2f p0 = x * v2f{a.fir4[i][0], a.fir4[i][0]}, p1 = x * v2f{a.fir4[i][1], a.fir4[i][1]}, p2 = x * v2f{a.fir4[i][2], a.fir4[i][2]};
            o0 = o0 + p0;
            o1 = o1 + p1;
            o2 = o2 + p2;
        }
        vc.x = fmaxf(fmaxf(fmaxf(vc.x, fabsf(o0.x)), fabsf(o1.x)), fabsf(o2.x));
        vc.y = fmaxf(fmaxf(fmaxf(vc.y, fabsf(o0.y)), fabsf(o1.y)), fabsf(o2.y));
    } else if constexpr (DL == 24) {
        v2f o = x * v2f{a.fir2[0], a.fir2[0]};
#pragma unroll
        for (int i = 1; i < 24; ++i) {
            x = v2f{w0[-i], w1[-i]};
            const v2f p = x * v2f{a.fir2[i], a.fir2[i]};
            o = o + p;
        }
        vc.x = fmaxf(vc.x, fabsf(o.x));
        vc.y = fmaxf(vc.y, fabsf(o.y));
    }
    return vc;
}

template <int DL>
__global__ __launch_bounds__(kLmLevelThreads) void lm_level_kernel(LmArgs a, uint32_t n_tiles) {
    constexpr uint32_t H = kLmHistory, T = kLmLevelTile, stride = T + H + 1;
    extern __shared__ float xs[];  // [channels][stride]: LDS frame H + f = frame f of the tile
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const LmStreamCall call = a.calls[s];
    const uint64_t t0 = (uint64_t)tile * T;
    if (t0 >= call.frames) return;  // (uniform)
    const uint32_t C = a.channels, total = (T + H) * C;
    {
        // dword e of the staged run is (frame e / C, channel e % C): both advance without a division
        const uint32_t q = kLmLevelThreads / C, r = kLmLevelThreads - q * C;
        uint32_t fr = tid / C, c = tid - fr * C;
        // a tile with its history inside the call: one contiguous run of the interleaved PCM (frames beyond frames[s] of the last
        // tile are inside the row; their levels are never written)
        const bool inside = t0 >= H && t0 + T <= a.frames_capacity;
        const float* run = a.in + ((uint64_t)s * a.frames_capacity + (inside ? t0 - H : 0)) * C;
#pragma unroll 4
        for (uint32_t e = tid; e < total; e += kLmLevelThreads) {
            xs[c * stride + fr] = inside ? run[e] : lm_x_at(a, call, s, (int64_t)t0 - (int64_t)H + (int64_t)fr, c);
            fr += q;
            c += r;
            if (c >= C) {
                c -= C;
                ++fr;
            }
        }
    }
    __syncthreads();
    const float g = fabsf(a.records[s].gain);
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {  // frames tid, tid + 256 of each half of the tile share the packed arithmetic
        const uint32_t f0 = half * (T / 2) + tid, f1 = f0 + kLmLevelThreads;
        if (t0 + f0 >= call.frames) break;
        v2f v = v2f{__builtin_nanf(""), __builtin_nanf("")};  // fmaxf ignores it: a level whose every operand is NaN stays NaN
        for (uint32_t c = 0; c < C; ++c) {
            const float* w = xs + c * stride + H;
            const v2f vc = lm_pair_level<DL>(a, w + f0, w + f1);
            v.x = fmaxf(v.x, vc.x);
            v.y = fmaxf(v.y, vc.y);
        }
        const float u[2] = {v.x * g, v.y * g};
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            const uint64_t rel = t0 + (k ? f1 : f0);
            if (rel >= call.frames) continue;
            uint32_t q = kLmUnity;
            if (u[k] > a.ceiling) q = (uint32_t)((double)a.ceiling / (double)u[k] * 16777216.0);  // (false for NaN; an infinite u gives 0)
            a.q[(uint64_t)s * a.q_row + rel] = q;
        }
    }
}

// ---- hold.  Entry i of a stream's row is the minimum of the L values of q that end at rel = first + i,
// first = (latency - held) - (attack - 1) - (window - hold_len): the oldest one the smooth pass reads.
__device__ __forceinline__ int64_t lm_first_held(const LmArgs& a, const LmStreamCall& call) {
    return (int64_t)a.latency - (int64_t)call.held - (int64_t)(a.attack - 1) - (int64_t)(a.window - a.hold_len);
}

__global__ __launch_bounds__(256) void lm_hold_kernel(LmArgs a, uint32_t n_tiles) {
    constexpr uint32_t kPer = (kLmHoldTile + kLmHoldMaxWindow) / 256;
    __shared__ uint32_t b[kLmHoldTile + kLmHoldMaxWindow];
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const LmStreamCall call = a.calls[s];
    if (call.emit == 0) return;  // (uniform)
    const uint64_t count = (uint64_t)call.emit + (a.attack - 1) + (a.window - a.hold_len), i0 = (uint64_t)tile * kLmHoldTile;
    if (i0 >= count) return;
    const uint32_t L = a.hold_len, M = kLmHoldTile + L - 1;
    const int64_t base = lm_first_held(a, call) + (int64_t)i0 - (int64_t)(L - 1);  // rel of b[0]
    for (uint32_t k = tid; k < M; k += 256) b[k] = lm_q_at(a, call, s, base + (int64_t)k);
    __syncthreads();
    uint32_t win = 1;
    for (; 2 * win <= L; win *= 2) {  // b[k] = the minimum of the `win` values that end at k (for k >= win - 1; what lies before is not used)
        uint32_t m[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t k = tid + j * 256;
            m[j] = k < M ? min(b[k], b[k >= win ? k - win : k]) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t k = tid + j * 256;
            if (k < M) b[k] = m[j];
        }
        __syncthreads();
    }
    // win <= L < 2 win: two windows of `win` cover the L values that end at k
    for (uint32_t t = tid; t < kLmHoldTile; t += 256)
        if (i0 + t < count) a.held_min[(uint64_t)s * a.m_row + i0 + t] = min(b[L - 1 + t], b[win - 1 + t]);
}

// ---- smooth
__global__ __launch_bounds__(256) void lm_smooth_kernel(LmArgs a, uint32_t n_tiles, uint32_t per) {
    extern __shared__ unsigned long long lm_lds[];  // [256 * per] values and their prefix sums, then [2][256] run totals
    unsigned long long* P = lm_lds;
    unsigned long long* tot = lm_lds + 256u * per;
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const LmStreamCall call = a.calls[s];
    const uint64_t f0 = (uint64_t)tile * kLmSmoothTile;
    if (f0 >= call.emit) return;  // (uniform)
    const uint32_t A = a.attack, L = a.hold_len, far = a.window - L, K = a.window / L;
    const uint32_t n_here = (uint32_t)min((uint64_t)kLmSmoothTile, (uint64_t)call.emit - f0), M = n_here + A - 1;
    // P[k] = w at rel = (latency - held) + f0 - (A - 1) + k: entry f0 + k + far of the stream's row of window-L minima
    const uint32_t* hm = a.held_min + (uint64_t)s * a.m_row + f0 + far;
    for (uint32_t k = tid; k < M; k += 256) {
        uint32_t w = hm[(int64_t)k - (int64_t)far];
        for (uint32_t j = 0; j < K; ++j) w = min(w, hm[(int64_t)k - (int64_t)j * L]);
        P[k] = w;
    }
    __syncthreads();
    unsigned long long sum = 0;
    const uint32_t k0 = tid * per;
    for (uint32_t j = 0; j < per; ++j)
        if (k0 + j < M) sum += P[k0 + j];
    tot[tid] = sum;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of the run totals
        const unsigned long long v = tot[cur * 256 + tid] + (tid >= d ? tot[cur * 256 + tid - d] : 0ull);
        tot[(cur ^ 1) * 256 + tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    unsigned long long run = tot[cur * 256 + tid] - sum;  // what lies in front of this thread's run
    for (uint32_t j = 0; j < per; ++j)
        if (k0 + j < M) {
            run += P[k0 + j];
            P[k0 + j] = run;
        }
    __syncthreads();
    const double scale = (double)((unsigned long long)A << 24);
    for (uint32_t t = tid; t < n_here; t += 256) {
        const unsigned long long S = P[t + A - 1] - (t != 0 ? P[t - 1] : 0ull);
        a.envelope[(uint64_t)s * a.e_row + f0 + t] = (float)((double)S / scale);
    }
}

// ---- apply
struct LmTally {
    PsTally out;           // of the emitted samples
    uint32_t limited = 0;  // frames with Gf < 1
    float low = 1.0f;      // the smallest Gf
};

// float i of the stream's output row: frame f = i / channels of the call's emitted frames
__device__ __forceinline__ float lm_scaled(const LmArgs& a, const LmStreamCall& call, uint32_t s, float gain, const float* env, uint64_t f,
                                           uint32_t c, LmTally& t) {
    const float gf = env[f];
    const float y = lm_x_at(a, call, s, (int64_t)f - (int64_t)call.held, c) * (gain * gf);
    t.out.take(y);
    if (c == 0) {
        t.limited += gf < 1.0f ? 1u : 0u;
        t.low = fminf(t.low, gf);
    }
    return y;
}

__global__ __launch_bounds__(kLmApplyThreads) void lm_apply_kernel(LmArgs a, uint32_t n_tiles) {
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const LmStreamCall call = a.calls[s];
    const uint32_t C = a.channels;
    const uint64_t n = (uint64_t)call.emit * C;
    if (n == 0) return;
    float* out = a.out + (uint64_t)s * a.out_capacity * C;
    const uint64_t to_aligned = ps_to_aligned(out);
    const uint32_t peel = (uint32_t)(to_aligned < n ? to_aligned : n);
    const uint64_t nvec = (n - peel) >> 2, v0 = (uint64_t)tile * kLmApplyTileVecs;
    if (tile != 0 && v0 >= nvec) return;  // (uniform over the workgroup, as the return above: no thread is left at the barrier below)
    const float gain = a.records[s].gain;
    const float* env = a.envelope + (uint64_t)s * a.e_row;
    LmTally t;
    if (tile == 0) {  // the floats outside the aligned body: threads 0 .. 2 the head, threads 4 .. 6 the tail
        const uint32_t tail = (uint32_t)((n - peel) & 3u);
        uint64_t i = n;
        if (tid < peel) i = tid;
        else if (tid >= 4 && tid < 4 + tail) i = peel + 4 * nvec + (tid - 4);
        if (i < n) out[i] = lm_scaled(a, call, s, gain, env, i / C, (uint32_t)(i % C), t);
    }
#pragma unroll
    for (uint32_t k = 0; k < kLmApplyInFlight; ++k) {
        const uint64_t v = v0 + k * kLmApplyThreads + tid;
        if (v < nvec) {
            const uint64_t i = peel + 4 * v;
            uint64_t f = i / C;
            uint32_t c = (uint32_t)(i - f * C);
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                y[j] = lm_scaled(a, call, s, gain, env, f, c, t);
                if (++c == C) {
                    c = 0;
                    ++f;
                }
            }
            *reinterpret_cast<v4f*>(out + i) = v4f{y[0], y[1], y[2], y[3]};
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        t.out.fold_step(d);
        ps_fold_step(t.limited, PsSum{}, d);
        ps_fold_step(t.low, PsMin{}, d);
    }
    // the two fields of its own go through the barrier of the sample tally's fold: posted in front of it, gathered behind it
    __shared__ uint32_t s_limited[kLmApplyThreads / 64];
    __shared__ float s_low[kLmApplyThreads / 64];
    ps_fold_post(t.limited, s_limited);
    ps_fold_post(t.low, s_low);
    t.out.fold_waves<kLmApplyThreads>();
    if (tid == 0) {
        ps_fold_gather<kLmApplyThreads>(t.limited, PsSum{}, s_limited);
        ps_fold_gather<kLmApplyThreads>(t.low, PsMin{}, s_low);
        omx_program_limit_record* r = a.records + s;
        t.out.commit(r);
        if (t.limited != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->frames_limited), (unsigned long long)t.limited);
        // (the bit pattern of a non-negative float orders like the value; fminf never lets a NaN in, and Gf is never one)
        if (t.low < 1.0f) atomicMin(reinterpret_cast<unsigned int*>(&r->min_envelope), __float_as_uint(t.low));
    }
}

// ---- carry: frame n of the stream at slot n mod length of its ring
__global__ __launch_bounds__(256) void lm_carry_kernel(LmArgs a, uint32_t n_tiles) {
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const LmStreamCall call = a.calls[s];
    const uint32_t C = a.channels, e = tile * 256 + threadIdx.x;
    ps_carry_row(a.ring_x + (uint64_t)s * a.latency * C, a.latency, C, call.ring_x, call.frames, e,
                 [&](uint64_t rel, uint32_t c) { return a.in[((uint64_t)s * a.frames_capacity + rel) * C + c]; });
    ps_carry_row(a.ring_q + (uint64_t)s * a.q_history, a.q_history, 1u, call.ring_q, call.frames, e,
                 [&](uint64_t rel, uint32_t) { return a.q[(uint64_t)s * a.q_row + rel]; });
}

uint32_t lm_grid(const LmArgs& a, uint64_t tiles) {
    const uint64_t blocks = (uint64_t)a.n_streams * tiles;
    if (blocks > 0x7FFFFFFFull) unsupported("programme limiter: call too long for one launch");
    return (uint32_t)blocks;
}

}  // namespace

void launch_lm_begin(const LmArgs& a, bool whole_call, hipStream_t stream) {
    ps_launch_per_stream(lm_begin_kernel, a.n_streams, stream, a, whole_call ? 1u : 0u);
}
void launch_lm_finish(const LmArgs& a, hipStream_t stream) {
    ps_launch_per_stream(lm_finish_kernel, a.n_streams, stream, a);
}
void launch_lm_level(const LmArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.max_frames + kLmLevelTile - 1) / kLmLevelTile;
    const dim3 grid(lm_grid(a, tiles)), block(kLmLevelThreads);
    const size_t lds = (size_t)a.channels * (kLmLevelTile + kLmHistory + 1) * sizeof(float);
    if (a.delay_len == 12) hipLaunchKernelGGL(lm_level_kernel<12>, grid, block, lds, stream, a, tiles);
    else if (a.delay_len == 24) hipLaunchKernelGGL(lm_level_kernel<24>, grid, block, lds, stream, a, tiles);
    else hipLaunchKernelGGL(lm_level_kernel<0>, grid, block, lds, stream, a, tiles);
}
void launch_lm_hold(const LmArgs& a, hipStream_t stream) {
    const uint64_t count = (uint64_t)a.max_emit + (a.attack - 1) + (a.window - a.hold_len);
    const uint32_t tiles = (uint32_t)((count + kLmHoldTile - 1) / kLmHoldTile);
    hipLaunchKernelGGL(lm_hold_kernel, dim3(lm_grid(a, tiles)), dim3(256), 0, stream, a, tiles);
}
void launch_lm_smooth(const LmArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.max_emit + kLmSmoothTile - 1) / kLmSmoothTile;
    // values per thread: odd, so that the runs of neighbouring threads start in different LDS banks
    const uint32_t per = ((kLmSmoothTile + a.attack - 1 + 255) / 256) | 1u;
    const size_t lds = ((size_t)256 * per + 512) * sizeof(unsigned long long);
    hipLaunchKernelGGL(lm_smooth_kernel, dim3(lm_grid(a, tiles)), dim3(256), lds, stream, a, tiles, per);
}
void launch_lm_apply(const LmArgs& a, hipStream_t stream) {
    // tiles of the longest row (a row's body is at most n / 4 vectors; tile 0 exists for every row that emits a float)
    const uint64_t max_n = (uint64_t)a.max_emit * a.channels;
    const uint64_t tiles = std::max<uint64_t>((max_n / 4 + kLmApplyTileVecs - 1) / kLmApplyTileVecs, 1);
    hipLaunchKernelGGL(lm_apply_kernel, dim3(lm_grid(a, tiles)), dim3(kLmApplyThreads), 0, stream, a, (uint32_t)tiles);
}
void launch_lm_carry(const LmArgs& a, hipStream_t stream) {
    const uint32_t longest = std::max(a.latency * a.channels, a.q_history);
    const uint32_t tiles = (longest + 255) / 256;
    hipLaunchKernelGGL(lm_carry_kernel, dim3(lm_grid(a, tiles)), dim3(256), 0, stream, a, tiles);
}

}  // namespace omx

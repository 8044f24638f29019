// Dynamics stage of the programme loudness bank (include/omx/program_dynamics.h states the definition, program_dynamics.hpp the passes).
//
// Indices.  `rel` counts frames from the first frame of the call: frame n of the stream is rel = n - n_old.  Frames in front of the
// call (rel < 0) come from the rings the carry pass of the earlier calls wrote (x and r: the newest LA = A - 1 frames, Gt: the newest
// W - 1 values), frames in front of the stream (n < 0) are x = 0, Gt = T[0] and r = T[0] * 2^16, and so is Gt at and beyond the last
// frame taken, which only a flush reads.  A call emits frames f = 0 .. emit-1, frame f being x[rel = f - held], with the gain
// E = floor(sum(r[rel .. rel + A - 1]) / A); it computes r for rel = 0 .. scan-1, scan = frames (+ LA with the flush).
//
//   level   : grid (stream, tile of kDyLevelTile frames).  The stream's curve and LOG go to LDS once per workgroup (a wavefront's
//             lookups are divergent: LDS serves them at a word per lane, scalar loads would take them one lane at a time), every
//             thread takes the frames tid + 256 j, folds the detector channels with fmaxf, takes the integer log2 from the bits and
//             the curve's value by an integer lerp and writes one int32 Gt.  No transcendental.
//   hold    : grid (stream, tile of kDyHoldTile values).  Gt with a halo of L - 1 in LDS, the window minimum by doubling, as the
//             limiter's on signed values.  L = min(W, kDyHoldMaxWindow); a longer W is the minimum of W / L shifted windows and one
//             at the far end, taken by the release pass as it loads.
//   release : grid (stream, tile of kDyReleaseTile values).  The min-plus scan r[n] = min(w[n] * 2^16, r[n-1] + d) as if the tile
//             began the stream: a run of 8 per thread in registers, the runs' aggregates (len, m) scanned over the workgroup with
//             combine((l1, m1), (l2, m2)) = (l1 + l2, min(m1 + l2 d, m2)), every length known from the index.  The ramp term
//             saturates at 40 * 2^32, above which no r lies, so that 64 bits hold every intermediate.  One aggregate per tile.
//   chain   : grid (stream).  The same scan over a stream's tile aggregates, a run of tiles per thread: the carry in front of every
//             tile, and the stream's carry into the next call.  The only place where a stream is serial, and it is one value per tile.
//   apply   : grid (stream, tile of kDySmoothTile frames).  r = min(local, carry + (position + 1) d) with a halo of A - 1 in LDS, an
//             exact prefix sum, E = floor(S / A), the factor by the EXP table and one exact power of two, out = (float)((double)x * k)
//             with 16-byte stores on aligned addresses (every tile peels the floats outside its aligned body), the trace, and the
//             record's sums and extrema with at most one atomic of each kind per workgroup: order-free, so the record is deterministic.
//   carry   : the newest LA frames of PCM and of r and the newest W - 1 values of Gt into the rings, behind the passes that read them.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_dynamics.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef long long v2ll __attribute__((ext_vector_type(2)));
constexpr uint32_t kDyFoldSlots = 6;  // 8-byte slots a wavefront posts to the apply pass's fold (five used)

__device__ __forceinline__ int32_t dy_first_gain(const DyArgs& a, const DyStreamCall& call) { return a.curves[(uint64_t)call.curve * kDyCurveRow]; }

__device__ __forceinline__ uint32_t dy_x_bits(const DyArgs& a, const DyStreamCall& call, uint32_t s, int64_t rel, uint32_t c) {
    if ((int64_t)call.n_old + rel < 0 || rel >= (int64_t)call.frames) return 0u;
    if (rel >= 0) return __float_as_uint(a.in[((uint64_t)s * a.frames_capacity + (uint64_t)rel) * a.channels + c]);
    int64_t slot = (int64_t)call.ring_x + rel;  // rel >= -LA
    if (slot < 0) slot += call.attack - 1;
    return __float_as_uint(a.ring_x[((uint64_t)s * a.max_latency + (uint64_t)slot) * a.channels + c]);
}

__device__ __forceinline__ int32_t dy_gt_at(const DyArgs& a, const DyStreamCall& call, uint32_t s, int64_t rel, int32_t first_gain) {
    if ((int64_t)call.n_old + rel < 0 || rel >= (int64_t)call.frames) return first_gain;
    if (rel >= 0) return a.gt[(uint64_t)s * a.g_row + (uint64_t)rel];
    int64_t slot = (int64_t)call.ring_g + rel;  // rel >= -(W - 1)
    if (slot < 0) slot += call.window - 1;
    return a.ring_g[(uint64_t)s * a.max_history + (uint64_t)slot];
}

// min(m + len * d, 40 * 2^32) for m in [-40 * 2^32, 40 * 2^32]: the ramp of the release over len frames, saturated
__device__ __forceinline__ long long dy_ramp(long long m, unsigned long long len, long long d) {
    const unsigned long long hi = __umul64hi(len, (unsigned long long)d), lo = len * (unsigned long long)d;
    const unsigned long long inc = (hi != 0 || lo > 2ull * (unsigned long long)kDyCap) ? 2ull * (unsigned long long)kDyCap : lo;
    const long long r = m + (long long)inc;
    return r > kDyCap ? kDyCap : r;
}

// the same inside one release tile: len <= kDyReleaseTile and d < 2^38, so the product stays below 2^50 and nothing can overflow
__device__ __forceinline__ long long dy_ramp_in_tile(long long m, uint32_t len, long long d) {
    const long long r = m + (long long)len * d;
    return r > kDyCap ? kDyCap : r;
}

// r at rel >= 0 of the call: the tile-local value under the ramp from the tile's carry
__device__ __forceinline__ long long dy_r_here(const DyArgs& a, const DyStreamCall& call, uint32_t s, uint64_t rel) {
    const uint64_t tile = rel / kDyReleaseTile;
    const long long local = a.r_local[(uint64_t)s * a.r_row + rel], carry = a.tile_carry[(uint64_t)s * a.t_row + tile];
    return min(local, dy_ramp_in_tile(carry, (uint32_t)(rel - tile * kDyReleaseTile) + 1u, call.step));
}

__device__ __forceinline__ long long dy_r_at(const DyArgs& a, const DyStreamCall& call, uint32_t s, int64_t rel, int32_t first_gain) {
    if ((int64_t)call.n_old + rel < 0) return (long long)first_gain * 65536;
    if (rel >= 0) return dy_r_here(a, call, s, (uint64_t)rel);
    int64_t slot = (int64_t)call.ring_x + rel;  // rel >= -LA
    if (slot < 0) slot += call.attack - 1;
    return a.ring_r[(uint64_t)s * a.max_latency + (uint64_t)slot];
}

__device__ __forceinline__ omx_program_dynamics_record dy_idle_record(const DyArgs& a, const DyStreamCall& c) {
    omx_program_dynamics_record r{};
    r.out_sample_peak_db = a.floor_db;
    r.state = OMX_DYNAMICS_IDLE;
    r.latency_frames = c.attack - 1;
    r.curve_index = c.curve_index;
    return r;
}

__global__ __launch_bounds__(64) void dy_begin_kernel(DyArgs a, uint32_t whole_call) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const DyStreamCall c = a.calls[s];
    omx_program_dynamics_record r = a.records[s];
    if (c.flags & kCarryFlagClear) {
        r = dy_idle_record(a, c);
        a.carry[s] = (long long)dy_first_gain(a, c) * 65536;
    }
    if (whole_call) ps_begin_record<OMX_DYNAMICS_IDLE, OMX_DYNAMICS_RUNNING, OMX_DYNAMICS_FLUSHED>(r, c.n_old, c.n_old - c.held, c.frames, c.emit, c.flags);
    a.records[s] = r;
}

__global__ __launch_bounds__(64) void dy_finish_kernel(DyArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    omx_program_dynamics_record* r = a.records + s;
    r->out_sample_peak_db = ps_peak_db(r->out_sample_peak, a.floor_db);
    r->min_gain_db = (float)((double)r->min_gain * (kDyOctave / 4294967296.0));
    r->max_gain_db = (float)((double)r->max_gain * (kDyOctave / 4294967296.0));
}

// ---- level
__device__ __forceinline__ int32_t dy_level(float v, const int32_t* lg) {
    if (!(v >= 0x1p-40f)) return kDyLMin;  // (zeros, denormals; v is never NaN: fmaxf keeps it out)
    if (v >= 256.0f) return kDyLMax;
    const uint32_t bits = __float_as_uint(v), m = bits & 0x7FFFFFu, i = m >> 15;
    const int32_t e = (int32_t)(bits >> 23) - 127, f = (int32_t)(m & 0x7FFFu);
    return e * 65536 + lg[i] + (((lg[i + 1] - lg[i]) * f + 16384) >> 15);
}

__device__ __forceinline__ int32_t dy_curve_lerp(const int32_t* T, int32_t L) {
    const uint32_t u = (uint32_t)(L - kDyLMin), k = u >> 12, f = u & 4095u;
    const int32_t t0 = T[k];
    if (f == 0) return t0;  // (k = 768 only here: T[769] is never read)
    return t0 + (int32_t)((((long long)T[k + 1] - (long long)t0) * (long long)f + 2048) >> 12);
}

__global__ __launch_bounds__(kDyThreads) void dy_level_kernel(DyArgs a, uint32_t n_tiles) {
    __shared__ int32_t s_curve[kDyCurveRow];
    __shared__ int32_t s_log[OMX_DYNAMICS_TABLE_ENTRIES + 3];
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const DyStreamCall call = a.calls[s];
    const uint64_t t0 = (uint64_t)tile * kDyLevelTile;
    if (t0 >= call.frames) return;  // (uniform)
    const int32_t* T = a.curves + (uint64_t)call.curve * kDyCurveRow;
    for (uint32_t k = tid; k < OMX_DYNAMICS_CURVE_POINTS; k += kDyThreads) s_curve[k] = T[k];
    for (uint32_t k = tid; k < OMX_DYNAMICS_TABLE_ENTRIES; k += kDyThreads) s_log[k] = a.log_table[k];
    __syncthreads();
    const uint32_t C = a.channels, mask = call.mask;
    const float* key = a.key + ((uint64_t)s * a.frames_capacity + t0) * C;
    int32_t* gt = a.gt + (uint64_t)s * a.g_row + t0;
    const uint32_t n_here = (uint32_t)min((uint64_t)kDyLevelTile, (uint64_t)call.frames - t0);
#pragma unroll 4
    for (uint32_t f = tid; f < n_here; f += kDyThreads) {
        float v = 0.0f;  // fmaxf ignores a NaN: a frame of NaN stays 0
        for (uint32_t c = 0; c < C; ++c)
            if ((mask >> c) & 1u) v = fmaxf(v, fabsf(key[(uint64_t)f * C + c]));
        gt[f] = dy_curve_lerp(s_curve, dy_level(v, s_log));
    }
}

// ---- hold.  Entry i of a stream's row is the minimum of the L values of Gt that end at rel = i - (W - L): entry rel + (W - L) ends
// at rel, and the oldest entry is the far window of w[0].
__global__ __launch_bounds__(kDyThreads) void dy_hold_kernel(DyArgs a, uint32_t n_tiles) {
    constexpr uint32_t kPer = (kDyHoldTile + kDyHoldMaxWindow) / kDyThreads;
    __shared__ int32_t b[kDyHoldTile + kDyHoldMaxWindow];
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const DyStreamCall call = a.calls[s];
    if (call.scan == 0) return;  // (uniform)
    const uint32_t W = call.window, L = min(W, kDyHoldMaxWindow), far = W - L, M = kDyHoldTile + L - 1;
    const uint64_t count = (uint64_t)call.scan + far, i0 = (uint64_t)tile * kDyHoldTile;
    if (i0 >= count) return;
    const int32_t first_gain = dy_first_gain(a, call);
    const int64_t base = (int64_t)i0 - (int64_t)far - (int64_t)(L - 1);  // rel of b[0]
    for (uint32_t k = tid; k < M; k += kDyThreads) b[k] = dy_gt_at(a, call, s, base + (int64_t)k, first_gain);
    __syncthreads();
    uint32_t win = 1;
    for (; 2 * win <= L; win *= 2) {  // b[k] = the minimum of the `win` values that end at k (for k >= win - 1; what lies before is not used)
        int32_t m[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t k = tid + j * kDyThreads;
            m[j] = k < M ? min(b[k], b[k >= win ? k - win : k]) : 0;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t k = tid + j * kDyThreads;
            if (k < M) b[k] = m[j];
        }
        __syncthreads();
    }
    // win <= L < 2 win: two windows of `win` cover the L values that end at k
    for (uint32_t t = tid; t < kDyHoldTile; t += kDyThreads)
        if (i0 + t < count) a.held_min[(uint64_t)s * a.m_row + i0 + t] = min(b[L - 1 + t], b[win - 1 + t]);
}

// ---- release, inside tiles.  Elements [lo, hi) of a tile of n values, clipped
__device__ __forceinline__ uint32_t dy_clip(uint32_t x, uint32_t n) { return x < n ? x : n; }

__global__ __launch_bounds__(kDyThreads) void dy_release_kernel(DyArgs a, uint32_t n_tiles) {
    __shared__ long long sm[2][kDyThreads];
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const DyStreamCall call = a.calls[s];
    const uint64_t i0 = (uint64_t)tile * kDyReleaseTile;
    if (i0 >= call.scan) return;  // (uniform)
    const uint32_t n_here = (uint32_t)min((uint64_t)kDyReleaseTile, (uint64_t)call.scan - i0);
    const uint32_t W = call.window, L = min(W, kDyHoldMaxWindow), far = W - L, K = W / L;
    const long long d = call.step;
    const int32_t* hm = a.held_min + (uint64_t)s * a.m_row + i0;  // entry k + far: the window-L minimum that ends at value k of the tile
    const uint32_t k0 = tid * kDyReleasePer;
    long long v[kDyReleasePer], run = kDyCap;  // (40 * 2^32 is the scan's identity: no r lies above it)
#pragma unroll
    for (uint32_t j = 0; j < kDyReleasePer; ++j) {
        v[j] = kDyCap;
        if (k0 + j < n_here) {
            int32_t w = hm[k0 + j];  // the far window
            for (uint32_t q = 0; q < K; ++q) w = min(w, hm[k0 + j + far - q * L]);
            run = min((long long)w * 65536, run + d);  // (run <= 40 * 2^32 and d <= 40 * 2^32: no overflow; the other operand caps it)
            v[j] = run;
        }
    }
    // inclusive scan of the runs' aggregates; after the step `dd` entry t covers threads (t - 2 dd, t]
    sm[0][tid] = run;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t dd = 1; dd < kDyThreads; dd <<= 1) {
        long long m = sm[cur][tid];
        if (tid >= dd) {  // the right operand covers threads (tid - dd, tid]: its length follows from the indices
            const uint32_t right = dy_clip((tid + 1) * kDyReleasePer, n_here) - dy_clip((tid + 1 - dd) * kDyReleasePer, n_here);
            m = min(dy_ramp_in_tile(sm[cur][tid - dd], right, d), m);
        }
        sm[cur ^ 1][tid] = m;
        cur ^= 1;
        __syncthreads();
    }
    const long long before = tid != 0 ? sm[cur][tid - 1] : kDyCap;
    long long* out = a.r_local + (uint64_t)s * a.r_row + i0 + k0;
#pragma unroll
    for (uint32_t j = 0; j < kDyReleasePer; ++j) v[j] = min(v[j], dy_ramp_in_tile(before, j + 1, d));
    if (k0 + kDyReleasePer <= n_here) {  // (rows are a multiple of two values long and k0 is a multiple of eight: 16-byte aligned)
#pragma unroll
        for (uint32_t j = 0; j < kDyReleasePer; j += 2) *reinterpret_cast<v2ll*>(out + j) = v2ll{v[j], v[j + 1]};
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kDyReleasePer; ++j)
            if (k0 + j < n_here) out[j] = v[j];
    }
    if (tid == kDyThreads - 1) a.tile_agg[(uint64_t)s * a.t_row + tile] = sm[cur][tid];
}

// ---- chain: the carry in front of every tile of a stream
__global__ __launch_bounds__(kDyThreads) void dy_chain_kernel(DyArgs a) {
    __shared__ long long sm[2][kDyThreads];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const DyStreamCall call = a.calls[s];
    if (call.scan == 0) return;  // (uniform: the stream's carry stays)
    const uint64_t scan = call.scan;
    const uint32_t n_t = (uint32_t)((scan + kDyReleaseTile - 1) / kDyReleaseTile), per = (n_t + kDyThreads - 1) / kDyThreads;
    const uint32_t q0 = min(tid * per, n_t), q1 = min(q0 + per, n_t);
    const long long d = call.step, carry0 = a.carry[s];
    const long long* agg = a.tile_agg + (uint64_t)s * a.t_row;
    const auto tile_len = [&](uint32_t q) { return min((uint64_t)kDyReleaseTile, scan - (uint64_t)q * kDyReleaseTile); };
    const auto clip = [&](uint64_t tiles) { return min(tiles * kDyReleaseTile, scan); };  // values in front of tile `tiles`
    long long m = kDyCap;
    for (uint32_t q = q0; q < q1; ++q) m = min(dy_ramp(m, tile_len(q), d), agg[q]);
    sm[0][tid] = m;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t dd = 1; dd < kDyThreads; dd <<= 1) {
        long long x = sm[cur][tid];
        if (tid >= dd) {
            const uint64_t right = clip((uint64_t)(tid + 1) * per) - clip((uint64_t)(tid + 1 - dd) * per);
            x = min(dy_ramp(sm[cur][tid - dd], right, d), x);
        }
        sm[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    const long long before = tid != 0 ? sm[cur][tid - 1] : kDyCap;
    long long c = min(dy_ramp(carry0, clip((uint64_t)tid * per), d), before);
    long long* tc = a.tile_carry + (uint64_t)s * a.t_row;
    for (uint32_t q = q0; q < q1; ++q) {
        tc[q] = c;
        c = min(dy_ramp(c, tile_len(q), d), agg[q]);
    }
    if (q1 == n_t && q0 < q1) a.carry[s] = c;  // (every thread read carry0 in front of the scan's barriers)
}

// ---- apply
__device__ __forceinline__ double dy_factor(long long E, const unsigned long long* ex) {
    const long long I = E >> 32;
    const uint32_t F = (uint32_t)(E & 0xFFFFFFFFll), i = F >> 24, g = F & 0xFFFFFFu;
    const unsigned long long fx = ex[i] + (((ex[i + 1] - ex[i]) * (unsigned long long)g) >> 24);
    // 2^(I - 40), I within -40 .. 40, by its bits: the product is exact
    const double scale = __longlong_as_double((long long)(1023 + I - 40) << 52);
    return (double)fx * scale;
}

__global__ __launch_bounds__(kDyThreads) void dy_apply_kernel(DyArgs a, uint32_t n_tiles, uint32_t per) {
    // every array in the dynamic region, 8-byte entries first: [256 per] r and its prefix sums, [4] wavefront totals, [tile] factors,
    // [258] EXP, [4][kDyFoldSlots] the wavefronts' extrema and counts, then [tile] u32 "E == 0"
    extern __shared__ __attribute__((aligned(16))) long long dy_lds[];
    long long* P = dy_lds;
    long long* tot = P + kDyThreads * per;
    double* kf = reinterpret_cast<double*>(tot + kDyThreads / 64);
    unsigned long long* ex = reinterpret_cast<unsigned long long*>(kf + kDySmoothTile);
    long long* red = reinterpret_cast<long long*>(ex + OMX_DYNAMICS_TABLE_ENTRIES + 1);
    uint32_t* unity = reinterpret_cast<uint32_t*>(red + (kDyThreads / 64) * kDyFoldSlots);
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles, tid = threadIdx.x;
    const DyStreamCall call = a.calls[s];
    const uint64_t f0 = (uint64_t)tile * kDySmoothTile;
    if (f0 >= call.emit) return;  // (uniform)
    const uint32_t A = call.attack, C = a.channels;
    const uint32_t n_here = (uint32_t)min((uint64_t)kDySmoothTile, (uint64_t)call.emit - f0), M = n_here + A - 1;
    const int32_t first_gain = dy_first_gain(a, call);
    const int64_t rel0 = (int64_t)f0 - (int64_t)call.held;  // rel of the tile's first frame, and of P[0]
    for (uint32_t k = tid; k < OMX_DYNAMICS_TABLE_ENTRIES; k += kDyThreads) ex[k] = a.exp_table[k];
    for (uint32_t k = tid; k < M; k += kDyThreads) P[k] = dy_r_at(a, call, s, rel0 + (int64_t)k, first_gain);
    __syncthreads();
    long long sum = 0;
    const uint32_t k0 = tid * per;
    for (uint32_t j = 0; j < per; ++j)
        if (k0 + j < M) sum += P[k0 + j];
    // inclusive scan of the run totals: inside a wavefront by shuffles, the four wavefronts' totals around one barrier
    long long incl = sum;
#pragma unroll
    for (uint32_t dd = 1; dd < 64; dd <<= 1) {
        const long long up = __shfl_up(incl, dd);
        if ((tid & 63u) >= dd) incl += up;
    }
    if ((tid & 63u) == 63u) tot[tid >> 6] = incl;
    __syncthreads();
    long long run = incl - sum;  // what lies in front of this thread's run
    for (uint32_t w = 0; w < (tid >> 6); ++w) run += tot[w];
    for (uint32_t j = 0; j < per; ++j)
        if (k0 + j < M) {
            run += P[k0 + j];
            P[k0 + j] = run;
        }
    __syncthreads();
    uint32_t reduced = 0, boosted = 0;
    long long low = 0, high = 0;
    for (uint32_t t = tid; t < n_here; t += kDyThreads) {
        const long long S = P[t + A - 1] - (t != 0 ? P[t - 1] : 0ll);
        // floor(S / A) through one f64 division: |S| < 2^51 is exact in f64, and the quotient's rounding error (below 2^-14) is
        // smaller than its distance to the next integer (a multiple of 1 / A >= 2^-12, or 0); the remainder confirms it either way
        long long E = (long long)floor((double)S / (double)A);
        const long long rem = S - E * (long long)A;
        E += rem < 0 ? -1 : (rem >= (long long)A ? 1 : 0);
        kf[t] = dy_factor(E, ex);
        unity[t] = E == 0 ? 1u : 0u;
        if (a.gain_db) a.gain_db[(uint64_t)s * a.out_capacity + f0 + t] = (float)((double)E * (kDyOctave / 4294967296.0));
        reduced += E < 0 ? 1u : 0u;
        boosted += E > 0 ? 1u : 0u;
        low = min(low, E);
        high = max(high, E);
    }
    __syncthreads();
    // the floats of the tile's frames: floats [0, n) from `out`, the body from the first 16-byte boundary
    const uint32_t n = n_here * C;
    float* out = a.out + ((uint64_t)s * a.out_capacity + f0) * C;
    const uint32_t peel = min(ps_to_aligned(out), n), nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
    uint32_t over = 0, nonfinite = 0;
    float peak = 0.0f;
    const auto sample = [&](uint32_t fl, uint32_t c) {  // float c of the tile's frame fl
        const uint32_t bits = dy_x_bits(a, call, s, rel0 + (int64_t)fl, c);
        const float y = unity[fl] ? __uint_as_float(bits) : (float)((double)__uint_as_float(bits) * kf[fl]);
        const float m = fabsf(y);
        over += m > 1.0f ? 1u : 0u;  // false for NaN, true for infinity
        nonfinite += (__float_as_uint(y) & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
        peak = fmaxf(peak, m);  // a NaN operand is ignored
        return y;
    };
    {  // threads 0 .. 2 the head, threads 4 .. 6 the tail
        uint32_t i = n;
        if (tid < peel) i = tid;
        else if (tid >= 4 && tid < 4 + tail) i = peel + 4 * nvec + (tid - 4);
        if (i < n) out[i] = sample(i / C, i % C);
    }
    for (uint32_t v = tid; v < nvec; v += kDyThreads) {
        const uint32_t i = peel + 4 * v;
        uint32_t fl = i / C, c = i - fl * C;  // one division per vector; the four floats walk on from it
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j] = sample(fl, c);
            if (++c == C) {
                c = 0;
                ++fl;
            }
        }
        *reinterpret_cast<v4f*>(out + i) = v4f{y[0], y[1], y[2], y[3]};
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        ps_fold_step(over, PsSum{}, dd);
        ps_fold_step(nonfinite, PsSum{}, dd);
        ps_fold_step(reduced, PsSum{}, dd);
        ps_fold_step(boosted, PsSum{}, dd);
        ps_fold_step(peak, PsMax{}, dd);
        low = min(low, __shfl_xor(low, dd));
        high = max(high, __shfl_xor(high, dd));
    }
    if ((tid & 63u) == 0) {  // the wavefronts' values around one barrier
        long long* mine = red + (tid >> 6) * kDyFoldSlots;
        mine[0] = low;
        mine[1] = high;
        mine[2] = (long long)(((unsigned long long)over << 32) | nonfinite);    // (each at most 8192 per workgroup)
        mine[3] = (long long)(((unsigned long long)reduced << 32) | boosted);  // (each at most 1024)
        mine[4] = (long long)__float_as_uint(peak);
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < kDyThreads / 64; ++w) {
            const long long* theirs = red + w * kDyFoldSlots;
            low = min(low, theirs[0]);
            high = max(high, theirs[1]);
            over += (uint32_t)((unsigned long long)theirs[2] >> 32);
            nonfinite += (uint32_t)theirs[2];
            reduced += (uint32_t)((unsigned long long)theirs[3] >> 32);
            boosted += (uint32_t)theirs[3];
            peak = fmaxf(peak, __uint_as_float((uint32_t)theirs[4]));
        }
        omx_program_dynamics_record* r = a.records + s;
        if (over != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->samples_over), (unsigned long long)over);
        if (nonfinite != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->samples_nonfinite), (unsigned long long)nonfinite);
        if (reduced != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->frames_reduced), (unsigned long long)reduced);
        if (boosted != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->frames_boosted), (unsigned long long)boosted);
        // (the bit pattern of a non-negative float orders like the value; fmaxf never lets a NaN in)
        if (peak > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&r->out_sample_peak), __float_as_uint(peak));
        if (low < 0) __hip_atomic_fetch_min(reinterpret_cast<long long*>(&r->min_gain), low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (high > 0) __hip_atomic_fetch_max(reinterpret_cast<long long*>(&r->max_gain), high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- carry: frame n of the stream at slot n mod length of its ring
__global__ __launch_bounds__(kDyThreads) void dy_carry_kernel(DyArgs a, uint32_t n_tiles) {
    const uint32_t s = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const DyStreamCall call = a.calls[s];
    const uint32_t C = a.channels, e = tile * kDyThreads + threadIdx.x;
    const uint32_t LA = call.attack - 1, GH = call.window - 1;  // (the rows are as long as the bank's longest)
    ps_carry_row(a.ring_x + (uint64_t)s * a.max_latency * C, LA, C, call.ring_x, call.frames, e,
                 [&](uint64_t rel, uint32_t c) { return a.in[((uint64_t)s * a.frames_capacity + rel) * C + c]; });
    ps_carry_row(a.ring_r + (uint64_t)s * a.max_latency, LA, 1u, call.ring_x, call.frames, e,
                 [&](uint64_t rel, uint32_t) { return dy_r_here(a, call, s, rel); });
    ps_carry_row(a.ring_g + (uint64_t)s * a.max_history, GH, 1u, call.ring_g, call.frames, e,
                 [&](uint64_t rel, uint32_t) { return a.gt[(uint64_t)s * a.g_row + rel]; });
}

uint32_t dy_grid(const DyArgs& a, uint64_t tiles) {
    const uint64_t blocks = (uint64_t)a.n_streams * tiles;
    if (blocks > 0x7FFFFFFFull) unsupported("programme dynamics: call too long for one launch");
    return (uint32_t)blocks;
}

}  // namespace

void launch_dy_begin(const DyArgs& a, bool whole_call, hipStream_t stream) {
    ps_launch_per_stream(dy_begin_kernel, a.n_streams, stream, a, whole_call ? 1u : 0u);
}
void launch_dy_finish(const DyArgs& a, hipStream_t stream) {
    ps_launch_per_stream(dy_finish_kernel, a.n_streams, stream, a);
}
void launch_dy_level(const DyArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.max_frames + kDyLevelTile - 1) / kDyLevelTile;
    hipLaunchKernelGGL(dy_level_kernel, dim3(dy_grid(a, tiles)), dim3(kDyThreads), 0, stream, a, tiles);
}
void launch_dy_hold(const DyArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.m_row + kDyHoldTile - 1) / kDyHoldTile;
    hipLaunchKernelGGL(dy_hold_kernel, dim3(dy_grid(a, tiles)), dim3(kDyThreads), 0, stream, a, tiles);
}
void launch_dy_release(const DyArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(dy_release_kernel, dim3(dy_grid(a, a.t_row)), dim3(kDyThreads), 0, stream, a, a.t_row);
}
void launch_dy_chain(const DyArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(dy_chain_kernel, dim3(dy_grid(a, 1)), dim3(kDyThreads), 0, stream, a);
}
void launch_dy_apply(const DyArgs& a, hipStream_t stream) {
    const uint32_t tiles = (a.max_emit + kDySmoothTile - 1) / kDySmoothTile;
    // values per thread: odd, so that the runs of neighbouring threads start in different LDS banks
    const uint32_t per = ((kDySmoothTile + a.max_attack - 1 + kDyThreads - 1) / kDyThreads) | 1u;
    const size_t lds =
        ((size_t)kDyThreads * per + kDyThreads / 64 + kDySmoothTile + OMX_DYNAMICS_TABLE_ENTRIES + 1 + (kDyThreads / 64) * kDyFoldSlots) * 8 +
        kDySmoothTile * 4;
    hipLaunchKernelGGL(dy_apply_kernel, dim3(dy_grid(a, tiles)), dim3(kDyThreads), lds, stream, a, tiles, per);
}
void launch_dy_carry(const DyArgs& a, hipStream_t stream) {
    const uint32_t longest = std::max(a.max_latency * a.channels, a.max_history);
    const uint32_t tiles = (longest + kDyThreads - 1) / kDyThreads;
    hipLaunchKernelGGL(dy_carry_kernel, dim3(dy_grid(a, tiles)), dim3(kDyThreads), 0, stream, a, tiles);
}

}  // namespace omx

// Peaks of the programme loudness bank (include/omx/program_peaks.h): the true-peak interpolator of the reference
// (TruePeakMeter::process, loudness/processor.rs:123-151) has no recurrence — every output is a fixed-order f32 sum of 12 (4x, three
// phases) or 24 (2x) products of the newest samples — and a maximum does not care about order, so the whole programme call is cut
// into tiles that are measured independently and folded afterwards: bit-identical to the sample-by-sample meter however the programme
// is cut into calls.
//
// Peak pass, one workgroup per (stream, tile of kPkTile frames), one wavefront per channel up to four:
//   stage   : the tile and the DL - 1 frames before it, [frames][channels] interleaved in memory, are loaded as contiguous runs of
//             dwords (lane i takes dword i: coalesced for every channel count), sixteen loads in flight per thread, and written to
//             LDS per channel, frame f of the tile at f' + f' / 16 with f' = f + 32 (one pad dword per 16 frames).  The frames before the first tile of a call come from the
//             carried delay line (zeros after a reset); frames beyond frames[s] are staged as zeros and never counted.
//   measure : one wavefront per channel (the same map for 1 .. 8 channels: wave w takes channels w, w + 4), lane l takes the run of
//             kPkRun frames from 16 l: its window of 16 + DL - 1 samples sits at 17 l + constant in LDS, so every ds_read_b32 of the
//             wavefront hits 64 distinct banks.  The sums keep the reference's order, multiply THEN add, never fused (the library is
//             built with -ffp-contract=off); two samples half a run apart share one v_pk_mul_f32 / v_pk_add_f32 as lanes .x / .y, as
//             TruePeak<DL>::step of loudness_chunked.hip does.  The leading `0.0 + p` of every sum is dropped: it can only turn -0.0
//             into +0.0 and only |o| is used.
//   reduce  : (value, first frame) as one 64-bit key, value bits above the complemented frame: the larger value wins, the earlier
//             frame wins among equals (values are >= +0 and never NaN, so their bit patterns order like the values).  Six shuffle
//             steps per wavefront, then one 16-byte store per (stream, channel, tile).  No atomics.
//   timeline: the second instantiation, run only by a bank with the peak timeline on (include/omx/program_peak_timeline.h).  A lane
//             also keeps the sixteen v of its run; where a segment boundary cuts a run of the wavefront (a few lanes per tile), the
//             maxima of the two sides are formed from them without running the interpolator again.  The wavefront reduces one key
//             pair per segment the tile touches (at most five), the tile's partial is their maximum, and lanes 0 / 1 merge each into
//             the stream's keys with ONE global 64-bit atomic maximum per (segment, channel, kind): a maximum is order-free, so the
//             atomics cost no determinism, and a call boundary inside a segment merges by itself.
// Fold, one workgroup per stream, one wavefront per channel slot: the partials in tile order into the running record, the frame base
// added, the delay line of the next call written, the record's dB fields and maxima rebuilt.
#include "program_loudness.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v2f __attribute__((ext_vector_type(2)));  // two independent f32 lanes of a v_pk_*_f32 instruction

constexpr uint32_t T = kPkTile, R = kPkRun;
constexpr uint32_t kHalo = 32;                             // LDS frame index of the tile's frame 0 (>= the longest history, multiple of 16)
constexpr uint32_t kChanStride = (T + kHalo) / 16 * 17;    // dwords of one channel in LDS
constexpr uint32_t kThreads = 256;
static_assert(T == 64 * R && R == 16 && kHalo >= kPkMaxDelay - 1 && T % (4 * 64) == 0, "one wavefront per channel of a tile; pad per 16 frames");

__device__ __forceinline__ unsigned long long peak_key(float v, uint32_t frame) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - frame);
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long k) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), d), lo = (uint32_t)__shfl_xor((int)(uint32_t)k, d);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// |x| and v of the frames m (.._lo) and m + R / 2 (.._hi) of a run.  w[H + n] = sample n of the run, w[0 .. H) = the H samples before
// it; pair[j] = {w[j], w[j + R / 2]}: the same window position of the older and of the newer half of the run.
template <int DL>
__device__ __forceinline__ void run_values(const float (&w)[R + (DL > 1 ? DL - 1 : 0)], const v2f (&pair)[R / 2 + (DL > 1 ? DL - 1 : 0) + 1],
                                           const float (&fir)[DL == 12 ? 36 : 24], int m, float& x_lo, float& x_hi, float& v_lo, float& v_hi) {
    constexpr int H = DL > 1 ? DL - 1 : 0, HALF = R / 2;
    x_lo = fabsf(w[H + m]);
    x_hi = fabsf(w[H + m + HALF]);
    v_lo = x_lo;
    v_hi = x_hi;
    if constexpr (DL == 12) {
        // (three phases of one window position = three independent chains side by side)
        v2f o0 = pair[H + m] * v2f{fir[0], fir[0]};
        v2f o1 = pair[H + m] * v2f{fir[1], fir[1]};
        v2f o2 = pair[H + m] * v2f{fir[2], fir[2]};
#pragma unroll
        for (int i = 1; i < 12; ++i) {
            const v2f p0 = pair[H + m - i] * v2f{fir[3 * i], fir[3 * i]};
            const v2f p1 = pair[H + m - i] * v2f{fir[3 * i + 1], fir[3 * i + 1]};
            const v2f p2 = pair[H + m - i] * v2f{fir[3 * i + 2], fir[3 * i + 2]};
            o0 = o0 + p0;
            o1 = o1 + p1;
            o2 = o2 + p2;
        }
        v_lo = fmaxf(fmaxf(fmaxf(v_lo, fabsf(o0.x)), fabsf(o1.x)), fabsf(o2.x));
        v_hi = fmaxf(fmaxf(fmaxf(v_hi, fabsf(o0.y)), fabsf(o1.y)), fabsf(o2.y));
    } else if constexpr (DL == 24) {
        v2f o = pair[H + m] * v2f{fir[0], fir[0]};
#pragma unroll
        for (int i = 1; i < 24; ++i) o = o + pair[H + m - i] * v2f{fir[i], fir[i]};
        v_lo = fmaxf(v_lo, fabsf(o.x));
        v_hi = fmaxf(v_hi, fabsf(o.y));
    }
}

// a running maximum with the index of the first sample that reaches it (0 while the maximum is 0), and its merge with a LATER one
struct PkFirstMax {
    float v = 0.0f;
    uint32_t k = 0;
    // strictly greater, in time order: the first frame of the maximum.  A NaN (every operand of the max was one) compares false.
    __device__ __forceinline__ void take(bool in, float x, uint32_t at) {
        if (in && x > v) {
            v = x;
            k = at;
        }
    }
    __device__ __forceinline__ PkFirstMax then(const PkFirstMax& later) const { return later.v > v ? later : *this; }  // the older wins among equals
};

// the peaks of the first n_here (<= 16) samples of a run.
// k_* = index in the run of the first sample that reaches the maximum (0 when the maximum is 0).
// KEEP (the timeline form): v_all[n] = v of sample n of the run, for run_sides.
template <int DL, bool KEEP = false>
__device__ __forceinline__ void run_peaks(const float (&w)[R + (DL > 1 ? DL - 1 : 0)], uint32_t n_here, const float (&fir)[DL == 12 ? 36 : 24], float& tp,
                                          uint32_t& k_tp, float& sp, uint32_t& k_sp, float* v_all = nullptr) {
    constexpr int H = DL > 1 ? DL - 1 : 0, HALF = R / 2;
    v2f pair[HALF + H + 1];
#pragma unroll
    for (int j = 0; j < HALF + H; ++j) pair[j] = v2f{w[j], w[j + HALF]};
    PkFirstMax t_lo, t_hi, s_lo, s_hi;
#pragma unroll
    for (int m = 0; m < HALF; ++m) {
        const bool in_lo = (uint32_t)m < n_here, in_hi = (uint32_t)(m + HALF) < n_here;
        float x_lo, x_hi, v_lo, v_hi;
        run_values<DL>(w, pair, fir, m, x_lo, x_hi, v_lo, v_hi);
        if constexpr (KEEP) {
            v_all[m] = v_lo;
            v_all[m + HALF] = v_hi;
        }
        t_lo.take(in_lo, v_lo, (uint32_t)m);
        t_hi.take(in_hi, v_hi, (uint32_t)(m + HALF));
        s_lo.take(in_lo, x_lo, (uint32_t)m);
        s_hi.take(in_hi, x_hi, (uint32_t)(m + HALF));
    }
    const PkFirstMax t = t_lo.then(t_hi), s = s_lo.then(s_hi);
    tp = t.v;
    k_tp = t.k;
    sp = s.v;
    k_sp = s.k;
}

// A run that a segment boundary cuts (the timeline form): samples [0, n_a) lie before it, [n_a, n_here) behind it, and each side has
// maxima of its own.  From the v the interpolator has formed (it does not run again) and |x|, in time order.
__device__ __forceinline__ void run_sides(const float (&v_all)[R], const float* x, uint32_t n_a, uint32_t n_here, PkFirstMax (&t)[2], PkFirstMax (&s)[2]) {
#pragma unroll
    for (uint32_t n = 0; n < R; ++n) {
        const bool before = n < n_a, behind = !before && n < n_here;
        const float m = fabsf(x[n]);
        t[0].take(before, v_all[n], n);
        t[1].take(behind, v_all[n], n);
        s[0].take(before, m, n);
        s[1].take(behind, m, n);
    }
}

// TL: the timeline form (program_peak_timeline.hpp), launched only with the timeline on: besides the partial it merges the maxima of
// every segment the tile touches into the stream's keys.  Frame n of the call lies in segment seg_base + (phase + n) / L, and L >= 336
// (kPlMinRate), so a run of 16 frames touches at most 2 segments and a tile at most 5.
// Three wavefronts per SIMD are asked for: the timeline forms keep a run's sixteen v in registers beside the taps, and without the
// bound the 4x / 2x ones come out at 169 / 172 VGPRs, one and four above what three wavefronts leave each (168).  With it they take
// 167 / 168 and no scratch; the plain forms have the figures they had without it (152 / 143 / 55 VGPRs, 105 / 105 / 102 SGPRs).
// The attribute is a minimum only and carries no upper bound: the sample-peak-only forms still reach their 7 / 6 wavefronts.
template <int DL, bool TL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void pk_tile_kernel(PkArgs a) {
    extern __shared__ float lds[];  // [channels][kChanStride], then the taps
    constexpr int H = DL > 1 ? DL - 1 : 0;
    const uint32_t s = blockIdx.x / a.n_tiles, tile = blockIdx.x % a.n_tiles, tid = threadIdx.x;
    const PlStreamCall call = a.calls[s];
    const uint64_t start = (uint64_t)tile * T;
    if (start >= call.frames) return;  // (uniform) tiles beyond frames[s]
    const uint32_t nf = (uint32_t)min((uint64_t)T, (uint64_t)call.frames - start);
    const uint32_t C = a.channels, n_threads = blockDim.x;  // 64 x min(channels, 4): no wavefront without a channel

    // ---- stage.  The tile is T x channels contiguous dwords = a whole number of dwords per thread (16 ... 32); thread t takes dwords
    // t, t + n_threads, ...: (frame, channel) advance without a division.  Sixteen loads are issued before the first is used — a loop
    // of load-then-store turns waited for every load in turn (22 us per workgroup at 8 channels; this form: see DESIGN section 10).
    // The history in front of the tile (H x channels <= 184 dwords) is one more load of the first threads, issued ahead of them.
    {
        const float* row = a.pcm + ((uint64_t)s * a.frames_capacity + start) * C;  // frame 0 of the tile
        // (every load is unconditional — an address that does not count is replaced by the tile's first dword, which exists — so that
        // none waits for the one before it)
        const bool h_on = H > 0 && tid < (uint32_t)H * C;
        const uint32_t fh = h_on ? tid / C : 0u, ch = tid - fh * C;  // history frame fh - H of the tile
        const float* hp = row;
        if (h_on) hp = tile != 0 ? row - (uint32_t)H * C + tid                                        // inside the call
                                 : a.delay + ((uint64_t)s * kPlSlots + ch) * kPkMaxDelay + fh;  // before it: the carried history
        float hv = *hp;
        if (tile == 0 && call.reset) hv = 0.0f;
        constexpr uint32_t B = 16;
        const uint32_t per = T * C / n_threads, q = n_threads / C, r = n_threads - q * C;
        uint32_t f = tid / C, c = tid - f * C;
        for (uint32_t k0 = 0; k0 < per; k0 += B) {
            float v[B];
            uint32_t at[B];
            bool in[B];
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) {
                in[j] = k0 + j < per && f < nf;  // frames beyond frames[s] are staged as zeros
                v[j] = row[in[j] ? tid + (k0 + j) * n_threads : 0u];
                const uint32_t fp = kHalo + f;
                at[j] = c * kChanStride + fp + (fp >> 4);
                f += q;
                c += r;
                if (c >= C) {
                    c -= C;
                    ++f;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < B; ++j)
                if (k0 + j < per) lds[at[j]] = in[j] ? v[j] : 0.0f;  // (uniform)
        }
        if (h_on) {
            const uint32_t fp = kHalo - (uint32_t)H + fh;
            lds[ch * kChanStride + fp + (fp >> 4)] = hv;
        }
    }
    // The taps go through LDS into vector registers.  As kernel arguments they are scalars, and a packed operand needs the splat
    // {t, t} in a register pair: 72 scalar registers for the 4x interpolator, of which 18 spilled; as vector registers the pairs fit
    // (72 of the kernel's 152).
    constexpr uint32_t n_taps = DL == 12 ? 36 : 24;
    float* taps = lds + C * kChanStride;
    if (DL > 1 && tid < n_taps) taps[tid] = DL == 12 ? a.fir4[tid / 3][tid % 3] : a.fir2[tid];
    __syncthreads();
    float fir[n_taps];
    if constexpr (DL > 1) {
#pragma unroll
        for (uint32_t i = 0; i < n_taps; ++i) fir[i] = taps[i];
    }

    // ---- measure: wavefront w takes channels w, w + 4; lane l the frames [16 l, 16 l + 16) of the tile
    for (uint32_t u = tid; u < 64u * C; u += n_threads) {
        const uint32_t c = u >> 6, run = u & 63u;  // (c is uniform over the wavefront)
        const uint32_t first = run * R;
        const uint32_t n_here = nf > first ? min(nf - first, R) : 0u;
        const uint32_t at = (uint32_t)start + first;  // frames of the call fit 32 bits (frames_capacity <= 2^32 - 1)
        float w[R + H];
        if (n_here != 0) {
            const float* p = lds + c * kChanStride + 17u * run;
#pragma unroll
            for (int k = -H; k < (int)R; ++k) {
                // LDS frame kHalo + first + k at f' + f' / 16: 17 run + (kHalo + k) + floor((kHalo + k) / 16), a constant per k
                constexpr int base = (int)kHalo;
                w[k + H] = p[(base + k) + ((base + k) >> 4)];
            }
        }
        unsigned long long kt, ks;
        if constexpr (!TL) {
            float tp = 0.0f, sp = 0.0f;
            uint32_t k_tp = 0, k_sp = 0;
            if (n_here != 0) run_peaks<DL>(w, n_here, fir, tp, k_tp, sp, k_sp);
            kt = wave_max(peak_key(tp, at + k_tp));
            ks = wave_max(peak_key(sp, at + k_sp));
        } else {
            PkFirstMax t[2], m[2];
            float v_all[R];
            if (n_here != 0) run_peaks<DL, true>(w, n_here, fir, t[0].v, t[0].k, m[0].v, m[0].k, v_all);
            // frame 0 of the tile is frame off0 of segment seg0, and the tile touches n_segs segments.  (Uniform; formed behind the
            // interpolator, where the registers are free again; the 32-bit division is the common case and the cheap one.)
            const uint32_t L = a.seg;
            const uint64_t tile_pos = (uint64_t)call.phase + start;
            uint32_t off0;
            uint64_t seg0;
            if ((tile_pos >> 32) == 0) {
                seg0 = call.seg_base + (uint32_t)tile_pos / L;
                off0 = (uint32_t)tile_pos % L;
            } else {
                seg0 = call.seg_base + tile_pos / L;
                off0 = (uint32_t)(tile_pos % L);
            }
            const uint32_t n_segs = (off0 + nf - 1) / L + 1;
            // the run starts at frame `pos` of segment `r` of the tile; n_a of its frames lie before its one possible boundary
            uint32_t pos = off0 + first, r = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)  // (off0 + first < L + T <= 5 L)
                if (pos >= L) {
                    pos -= L;
                    ++r;
                }
            const uint32_t n_a = min(n_here, L - pos);
            // a boundary cuts the run of a few lanes per tile at most: only their wavefronts redo the bookkeeping, per side
            if (__any(n_a < n_here) != 0 && n_here != 0) {
                t[0] = m[0] = PkFirstMax{};
                run_sides(v_all, w + H, n_a, n_here, t, m);
            }
            kt = 0ull;
            ks = 0ull;
            for (uint32_t q = 0; q < n_segs; ++q) {  // (uniform) segment q of the tile: the wavefront's maximum, then one atomic per kind
                const bool mine_a = n_here != 0 && q == r, mine_b = n_a < n_here && q == r + 1;
                unsigned long long qt = 0ull, qs = 0ull;
                if (mine_a) {
                    qt = peak_key(t[0].v, at + t[0].k);
                    qs = peak_key(m[0].v, at + m[0].k);
                } else if (mine_b) {
                    qt = peak_key(t[1].v, at + t[1].k);
                    qs = peak_key(m[1].v, at + m[1].k);
                }
                qt = wave_max(qt);
                qs = wave_max(qs);
                kt = qt > kt ? qt : kt;  // the tile's partial is the maximum over its segments
                ks = qs > ks ? qs : ks;
                // lane 0 the true peak, lane 1 the sample peak.  A maximum of 0 leaves the key as it is: cleared, a peak of 0 at offset 0.
                const unsigned long long key = run == 0 ? qt : qs;
                const uint64_t row = seg0 + q;
                if (run < 2 && (key >> 32) != 0 && row < a.tl_rows) {
                    const uint32_t in_tile = (0xFFFFFFFFu - (uint32_t)key) - (uint32_t)start;
                    const unsigned long long merged = (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(0xFFFFFFFFu - (off0 + in_tile - q * L));
                    atomicMax(a.tl_keys + (((uint64_t)s * a.tl_rows + row) * C + c) * 2 + run, merged);
                }
            }
        }
        if (run == 0) {
            PkPartial out;
            out.true_peak = __uint_as_float((uint32_t)(kt >> 32));
            out.true_peak_frame = 0xFFFFFFFFu - (uint32_t)kt;
            out.sample_peak = __uint_as_float((uint32_t)(ks >> 32));
            out.sample_peak_frame = 0xFFFFFFFFu - (uint32_t)ks;
            a.partials[((uint64_t)s * C + c) * a.n_tiles + tile] = out;
        }
    }
}

// ---- fold: one workgroup per stream, wavefront c = channel slot c
__global__ __launch_bounds__(64 * kPlSlots) void pk_fold_kernel(PkArgs a) {
    __shared__ float s_tp[kPlSlots], s_sp[kPlSlots];
    __shared__ unsigned long long s_tpf[kPlSlots], s_spf[kPlSlots];
    const uint32_t s = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const PlStreamCall call = a.calls[s];
    if (call.frames == 0 && call.reset == 0) return;  // (uniform) a stream without frames keeps everything
    omx_program_peak_record* rec = a.records + s;
    const bool keep = call.reset == 0;
    const uint64_t base = keep ? rec->frames : 0;  // frames since the reset before this call
    float tp = keep ? rec->true_peak[c] : 0.0f, sp = keep ? rec->sample_peak[c] : 0.0f;
    unsigned long long tpf = keep ? rec->true_peak_frame[c] : 0ull, spf = keep ? rec->sample_peak_frame[c] : 0ull;
    const uint32_t H = a.delay_len > 1 ? a.delay_len - 1 : 0u;
    float* delay = a.delay + ((uint64_t)s * kPlSlots + c) * kPkMaxDelay;
    if (c < a.channels && call.frames != 0) {
        const uint32_t tiles = (call.frames + T - 1) / T;
        const PkPartial* part = a.partials + ((uint64_t)s * a.channels + c) * a.n_tiles;
        unsigned long long kt = 0ull, ks = 0ull;
        for (uint32_t j = lane; j < tiles; j += 64) {
            const PkPartial p = part[j];
            const unsigned long long t = peak_key(p.true_peak, p.true_peak_frame), m = peak_key(p.sample_peak, p.sample_peak_frame);
            kt = t > kt ? t : kt;
            ks = m > ks ? m : ks;
        }
        kt = wave_max(kt);
        ks = wave_max(ks);
        const float t = __uint_as_float((uint32_t)(kt >> 32)), m = __uint_as_float((uint32_t)(ks >> 32));
        if (t > tp) {  // the earlier frame (the running one) wins among equals
            tp = t;
            tpf = base + (0xFFFFFFFFu - (uint32_t)kt);
        }
        if (m > sp) {
            sp = m;
            spf = base + (0xFFFFFFFFu - (uint32_t)ks);
        }
        // the delay line of the next call: the newest H samples; a call of fewer than H frames shifts the old ones
        if (lane < H) {
            const int64_t n = (int64_t)call.frames - (int64_t)H + (int64_t)lane;  // frame of the call, < 0: before it
            float v = 0.0f;
            if (n >= 0) v = a.pcm[((uint64_t)s * a.frames_capacity + (uint64_t)n) * a.channels + c];
            else if (keep) v = delay[(int64_t)lane + (int64_t)call.frames];
            delay[lane] = v;  // (every lane of the wavefront has read before any writes)
        }
    } else if (!keep && lane < kPkMaxDelay) {
        delay[lane] = 0.0f;
    }
    if (lane == 0) {
        s_tp[c] = tp;
        s_sp[c] = sp;
        s_tpf[c] = tpf;
        s_spf[c] = spf;
    }
    __syncthreads();  // (also: every read of the running record lies before its rewrite)
    if (threadIdx.x != 0) return;
    omx_program_peak_record r{};
    const bool empty = base + call.frames == 0;  // reset and nothing taken: as a new bank
    r.frames = base + call.frames;
    r.channels = empty ? 0u : a.channels;
    r.oversampling = empty ? 0u : (a.delay_len == 12 ? 4u : (a.delay_len == 24 ? 2u : 1u));
    r.max_true_peak_db = a.floor_db;
    r.max_sample_peak_db = a.floor_db;
    float best = 0.0f;
    for (uint32_t k = 0; k < kPlSlots; ++k) {
        r.true_peak[k] = s_tp[k];
        r.sample_peak[k] = s_sp[k];
        r.true_peak_frame[k] = s_tpf[k];
        r.sample_peak_frame[k] = s_spf[k];
        r.true_peak_db[k] = power_to_db(s_tp[k] * s_tp[k], a.floor_db);
        r.sample_peak_db[k] = power_to_db(s_sp[k] * s_sp[k], a.floor_db);
        if (k < r.channels) {
            r.max_true_peak_db = fmaxf(r.max_true_peak_db, r.true_peak_db[k]);
            r.max_sample_peak_db = fmaxf(r.max_sample_peak_db, r.sample_peak_db[k]);
            if (s_tp[k] > best) {  // lowest channel on a tie
                best = s_tp[k];
                r.max_true_peak_channel = k;
            }
        }
    }
    *rec = r;
}

// a bank's records and delay lines as set_peaks(1) leaves them
__global__ __launch_bounds__(64) void pk_clear_kernel(omx_program_peak_record* records, float* delay, uint32_t n_streams, float floor_db) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_streams) return;
    for (uint32_t i = lane; i < kPlSlots * kPkMaxDelay; i += 64) delay[(uint64_t)s * kPlSlots * kPkMaxDelay + i] = 0.0f;
    if (lane != 0) return;
    omx_program_peak_record r{};
    for (uint32_t k = 0; k < kPlSlots; ++k) {
        r.true_peak_db[k] = floor_db;
        r.sample_peak_db[k] = floor_db;
    }
    r.max_true_peak_db = floor_db;
    r.max_sample_peak_db = floor_db;
    records[s] = r;
}

}  // namespace

void launch_pk_tiles(const PkArgs& a, hipStream_t stream) {
    const uint64_t blocks = (uint64_t)a.n_streams * a.n_tiles;
    if (blocks > 0x7FFFFFFFull) unsupported("programme peaks: call too long for one launch");
    const size_t lds = ((size_t)a.channels * kChanStride + 36) * sizeof(float);
    const dim3 grid((uint32_t)blocks), block(64u * std::min(a.channels, kThreads / 64u));
    if (a.tl_keys) {  // the timeline form: only a bank with the peak timeline on runs these
        if (a.delay_len == 12) hipLaunchKernelGGL((pk_tile_kernel<12, true>), grid, block, lds, stream, a);
        else if (a.delay_len == 24) hipLaunchKernelGGL((pk_tile_kernel<24, true>), grid, block, lds, stream, a);
        else hipLaunchKernelGGL((pk_tile_kernel<0, true>), grid, block, lds, stream, a);
        return;
    }
    if (a.delay_len == 12) hipLaunchKernelGGL((pk_tile_kernel<12, false>), grid, block, lds, stream, a);
    else if (a.delay_len == 24) hipLaunchKernelGGL((pk_tile_kernel<24, false>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((pk_tile_kernel<0, false>), grid, block, lds, stream, a);
}
void launch_pk_fold(const PkArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pk_fold_kernel, dim3(a.n_streams), dim3(64 * kPlSlots), 0, stream, a);
}
void launch_pk_clear(omx_program_peak_record* records, float* delay, uint32_t n_streams, float floor_db, hipStream_t stream) {
    hipLaunchKernelGGL(pk_clear_kernel, dim3(n_streams), dim3(64), 0, stream, records, delay, n_streams, floor_db);
}

}  // namespace omx

// Signal QC of the programme loudness bank (include/omx/program_inspect.h states the definition, program_inspect.hpp the passes).
//
// The pass is bound by reading 4 * channels bytes per frame once; it writes 32 bytes per predicate and tile.
//
//   main   : grid (tile of 256 * FPT frames, stream; in_frames_per_thread of the channel count).  A tile wholly beyond frames[s] leaves
//            after reading its stream's frame count.
//     in     the tile's input is one contiguous run of d_in, and a row's base is only 4-byte aligned at odd channel counts.  The
//            floats in front of the first 16-byte boundary and behind the last one go by dword, the body by aligned 16-byte loads
//            (all of a thread's loads issued before the first is used) and aligned 16-byte LDS stores: the staging keeps the
//            memory's interleaving, shifted by up to three floats.  Nothing is written to d_in.  (A staging with an odd frame
//            stride, as the remix has it, reads without bank conflicts but costs an index computation and a dword LDS store per
//            float: this pass is bound by instruction issue, not by LDS bandwidth, and the flat copy measured faster.)
//     terms  thread tid takes frames tid, tid + 256, .. of the tile, so the 64 lanes of a wavefront hold 64 consecutive frames and
//            one ballot gives the mask word of a predicate over them: C hot words and one quiet word per 64 frames
//            (at most 9 bits per frame against 32 * C bits read).  A ballot is uniform (a scalar register pair): lane 0 hands
//            the C + 1 words of 64 frames to LDS.  The frames a short tile lacks are staged as zeros and the quiet predicate asks for
//            the frame: bits beyond the tile's frames are clear.  The NaN count is the population count of a ballot.  The DC term and the pair terms are integers of at most 2^30 in magnitude,
//            summed per thread in 64 bits.
//     sums   the family's reduction: six shuffle steps, four wavefronts through LDS.  Then one plain 64-bit store per sum and
//            workgroup into the call's table of tile sums, NOT an atomic add on the stream's record: 64 long programmes mean
//            thousands of workgroups per record, and the remix measured what their atomics on one cache line cost.
//     runs   (C + 1) * W mask words, W = 4 * FPT words per predicate: one thread per word makes the word's run summary (InRuns) with
//            shift-and-and doubling (no loop over bits: an all-set word costs what an empty one costs), then log2 W butterfly steps
//            over the W lanes of a predicate compose them in frame order (in_compose is associative; the lower lane block is the left
//            operand).  The lane of word 0 stores the tile's summary: two 16-byte stores per predicate and tile.
//   fold   : one workgroup per stream, 1 to 16 wavefronts by the number of tiles (one wavefront per stream would leave 64 long
//            programmes to 64 wavefronts).  Every thread adds up its share of each tile sum, the workgroup reduces them and one
//            thread per sum adds the total to the record.  Per predicate every wavefront takes a contiguous range of the tiles, 64 at
//            a time: the lanes load 64 tile summaries, compose them with the same butterfly and append the result to what the
//            wavefront's earlier chunks gave.  One thread per predicate then composes the wavefronts' summaries in order, composes
//            the running record (as the summary of all earlier calls: its length N, its open run as the tail, its leading silence
//            as the head) with the call's summary and stores the fields.  Plain loads and stores, no atomics, a fixed order.
//   Templated on the channel count (eight instantiations; DESIGN.md lists their registers, LDS and scratch).
//   Only vector loads and vector stores are used, no atomics at all.
#include "program_inspect.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ InRuns in_identity() { return InRuns{0, 0, 0, 0, 0, 0, 0, 0}; }

// The summary of stretch a followed by stretch b under the minimum run m (>= 1).  The run across the seam has a.tail + b.head
// frames.  b counted its head run when b.head >= m, as if it began at b's start; in the whole it reaches m inside b only when
// a.tail < m.  Of equally long runs the earliest wins: a's best, the seam run, b's best start in that order.
__device__ __forceinline__ InRuns in_compose(const InRuns& a, const InRuns& b, uint32_t m) {
    InRuns r;
    r.len = a.len + b.len;
    r.head = a.head == a.len ? a.len + b.head : a.head;
    r.tail = b.tail == b.len ? b.len + a.tail : b.tail;
    const uint32_t cross = a.tail + b.head;
    uint32_t best = a.best, start = a.start;
    if (cross > best) {
        best = cross;
        start = a.len - a.tail;
    }
    if (b.best > best) {
        best = b.best;
        start = a.len + b.start;
    }
    r.best = best;
    r.start = start;
    r.reach = a.reach + b.reach - (b.head >= m ? 1u : 0u) + ((a.tail < m && cross >= m) ? 1u : 0u);
    r.set = a.set + b.set;
    r._pad = 0;
    return r;
}

// The summary of one mask word: bit n is frame n, `len` frames (0 .. 64), the bits at and above len clear.
// x<k> has bit n set when a run of at least k frames ends at frame n: x<2k> = x<k> & (x<k> << k), and in general
// x<j + k> = x<k> & (x<j> << k).
__device__ __forceinline__ InRuns in_word(uint64_t M, uint32_t len, uint32_t m) {
    InRuns r;
    r.len = len;
    r.set = (uint32_t)__popcll(M);
    r.head = ~M ? (uint32_t)__ffsll((long long)~M) - 1u : 64u;
    const uint64_t top = len ? M << (64u - len) : 0ull;  // the last frame at bit 63
    r.tail = ~top ? (uint32_t)__clzll((long long)~top) : 64u;
    const uint64_t x1 = M, x2 = x1 & (x1 << 1), x4 = x2 & (x2 << 2), x8 = x4 & (x4 << 4), x16 = x8 & (x8 << 8), x32 = x16 & (x16 << 16),
                   x64 = x32 & (x32 << 32);
    // the longest run: the largest k with x<k> != 0, found bit by bit from the top
    uint32_t k = x64 ? 64u : 0u;
    uint64_t cur = x64;
    const auto longer = [&](uint64_t xs, uint32_t s) {
        const uint64_t y = k ? xs & (cur << s) : xs;
        if (y) {
            cur = y;
            k += s;
        }
    };
    longer(x32, 32);
    longer(x16, 16);
    longer(x8, 8);
    longer(x4, 4);
    longer(x2, 2);
    longer(x1, 1);
    r.best = k;
    r.start = k ? (uint32_t)__ffsll((long long)cur) - k : 0u;  // (the lowest end, + 1 - k)
    // frames at which a run reaches m: x<m> set and x<m> of the frame before clear.  x<m> from the binary digits of m.
    uint32_t have = (m & 64u) ? 64u : 0u;
    uint64_t xm = x64;
    const auto digit = [&](uint64_t xs, uint32_t s) {
        if (m & s) {
            xm = have ? xs & (xm << s) : xs;
            have += s;
        }
    };
    digit(x32, 32);
    digit(x16, 16);
    digit(x8, 8);
    digit(x4, 4);
    digit(x2, 2);
    digit(x1, 1);
    r.reach = m <= 64u ? (uint32_t)__popcll(xm & ~(xm << 1)) : 0u;
    r._pad = 0;
    return r;
}

__device__ __forceinline__ InRuns in_shuffle_xor(const InRuns& r, int d) {
    InRuns o;
    o.len = (uint32_t)__shfl_xor((int)r.len, d);
    o.head = (uint32_t)__shfl_xor((int)r.head, d);
    o.tail = (uint32_t)__shfl_xor((int)r.tail, d);
    o.best = (uint32_t)__shfl_xor((int)r.best, d);
    o.start = (uint32_t)__shfl_xor((int)r.start, d);
    o.reach = (uint32_t)__shfl_xor((int)r.reach, d);
    o.set = (uint32_t)__shfl_xor((int)r.set, d);
    o._pad = 0;
    return o;
}

// One butterfly step over lane blocks of d lanes: afterwards every lane of a block of 2 d lanes holds the block's summary.
__device__ __forceinline__ InRuns in_butterfly(const InRuns& r, uint32_t lane, int d, uint32_t m) {
    const InRuns other = in_shuffle_xor(r, d);
    const bool upper = (lane & (uint32_t)d) != 0;
    return in_compose(upper ? other : r, upper ? r : other, m);
}

__device__ __forceinline__ long long in_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// a.frames[s] != 0: stream s starts over
__global__ __launch_bounds__(64) void in_reset_kernel(InArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams || a.frames[s] == 0) return;
    omx_program_inspect_record* rec = a.records + s;
    uint64_t* w = reinterpret_cast<uint64_t*>(rec);
    for (uint32_t i = 0; i < sizeof(omx_program_inspect_record) / 8; ++i) w[i] = 0;
    rec->channels = a.channels;
    rec->n_pairs = a.n_pairs;
    for (uint32_t p = 0; p < a.n_pairs; ++p) {
        rec->pair[p].a = a.pair_a[p];
        rec->pair[p].b = a.pair_b[p];
    }
}

template <int C>
__global__ __launch_bounds__(kInThreads) void in_main_kernel(InArgs a, uint32_t s_base) {
    constexpr uint32_t FPT = in_frames_per_thread(C), kTile = kInThreads * FPT, kWaves = kInThreads / 64, W = kTile / 64;
    constexpr uint32_t kSums = 2 * C + 3 * OMX_INSPECT_MAX_PAIRS;
    __shared__ __attribute__((aligned(16))) float s_x[kTile * C + 4];  // (+ 4: the shift)
    __shared__ uint64_t s_mask[(C + 1) * W];  // predicate p, word k * kWaves + wave: frames 64 * word ..
    __shared__ long long s_sum[kWaves][kSums];
    const uint32_t s = s_base + blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t frames = a.frames[s];
    const uint64_t first = (uint64_t)blockIdx.x * kTile;
    if (first >= frames) return;  // (uniform over the workgroup: no thread is left at a barrier below)
    const uint32_t nf = (uint32_t)min((uint64_t)kTile, (uint64_t)frames - first);

    // ---- in: the tile's run of d_in, float j at s_x[shift + j]: shifted by up to three floats so that the run's first aligned
    // 16-byte vector is an aligned 16 bytes of LDS as well.  The floats of a short tile's missing frames are zero: such a frame is
    // not hot, has no NaN and adds nothing to any sum; only the quiet predicate has to ask whether the frame exists.
    const float* src = a.in + ((uint64_t)s * a.frames_capacity + first) * C;
    const uint32_t n = nf * C;
    const uint32_t peel = min(n, ps_to_aligned(src));
    const uint32_t shift = (4u - peel) & 3u;
    {
        const uint32_t nvec = (n - peel) >> 2, tail = (n - peel) & 3u;
        if (tid < peel) s_x[shift + tid] = src[tid];  // threads 0 .. 2 the head, threads 4 .. 6 the tail
        else if (tid >= 4 && tid < 4 + tail) s_x[shift + peel + 4 * nvec + (tid - 4)] = src[peel + 4 * nvec + (tid - 4)];
        constexpr uint32_t kInFlight = (kTile * C / 4 + kInThreads - 1) / kInThreads;  // every vector of a full tile in one round
        if (nvec) {  // (uniform)
            // no load under a branch: a thread without a vector loads the last one again and keeps nothing, so that every load of
            // the thread is in flight before the first is waited for
            v4f v[kInFlight];
#pragma unroll
            for (uint32_t u = 0; u < kInFlight; ++u) v[u] = *reinterpret_cast<const v4f*>(src + peel + 4 * min(u * kInThreads + tid, nvec - 1));
#pragma unroll
            for (uint32_t u = 0; u < kInFlight; ++u) {
                const uint32_t i = u * kInThreads + tid;
                if (i < nvec) *reinterpret_cast<v4f*>(s_x + shift + peel + 4 * i) = v[u];
            }
        }
        if (nf < kTile)  // (uniform; the last tile of a stream only)
            for (uint32_t j = shift + n + tid; j < shift + kTile * C; j += kInThreads) s_x[j] = 0.0f;
    }
    __syncthreads();

    // ---- terms: frames tid, tid + 256, .. of the tile.  The ballot of a predicate over the 64 consecutive frames of a wavefront is
    // uniform: lane 0 hands the C + 1 words of a frame row to LDS; the NaN count is a ballot's population count.
    long long dc[C];
    uint32_t nan[C];  // (uniform)
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)C; ++c) {
        dc[c] = 0;
        nan[c] = 0;
    }
    // (many channels: one frame at a time, or the scheduler hoists every LDS read of the tile and takes 200 registers)
#pragma unroll C <= 4 ? FPT : 1
    for (uint32_t k = 0; k < FPT; ++k) {
        const uint32_t f = k * kInThreads + tid;
        const float* x = s_x + shift + f * C;
        bool quiet = f < nf;
        uint64_t words[C + 1];  // (uniform)
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)C; ++c) {
            const float v = x[c];
            const float av = fabsf(v);
            const bool is_nan = v != v;
            quiet = quiet && av <= a.silence_level;                              // false for NaN
            // clamp(v, -4, 4) with NaN -> 0 in one go: fmaxf(NaN, 0) is 0, and the sign goes back on afterwards (a zero of either sign
            // rounds to the integer 0)
            const float vc = copysignf(fminf(fmaxf(av, 0.0f), 4.0f), v);
            dc[c] += (long long)(int)rintf(vc * 268435456.0f);                   // |q| <= 2^30
            nan[c] += (uint32_t)__popcll(__ballot(is_nan));
            words[c] = __ballot(av >= a.clip_level);                             // false for NaN, true for infinity
        }
        words[C] = __ballot(quiet);
        if (lane == 0) {
#pragma unroll
            for (uint32_t p = 0; p <= (uint32_t)C; ++p) s_mask[p * W + k * kWaves + wave] = words[p];
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)C; ++c) {
        const long long total = in_wave_sum(dc[c]);
        if (lane == 0) {
            s_sum[wave][2 * c] = total;
            s_sum[wave][2 * c + 1] = (long long)nan[c];
        }
    }
#pragma unroll
    for (uint32_t p = 0; p < OMX_INSPECT_MAX_PAIRS; ++p) {
        if (p < a.n_pairs) {  // (uniform)
            const uint32_t ia = a.pair_a[p], ib = a.pair_b[p];
            long long ab = 0;
            unsigned long long aa = 0, bb = 0;
#pragma unroll
            for (uint32_t k = 0; k < FPT; ++k) {
                const float* x = s_x + shift + (k * kInThreads + tid) * C;
                const float xa = x[ia], xb = x[ib];
                const float pab = xa * xb, paa = xa * xa, pbb = xb * xb;  // each rounded to f32 (-ffp-contract=off)
                // NaN gives 0, else rint(clamp(p, -1, 1) * 2^30).  fmaxf(NaN, 0) is 0, so clamping the magnitude to [0, 1] sends a
                // NaN to 0 without a compare; the product's sign goes back on afterwards; a square is not negative.
                const float cab = copysignf(fminf(fmaxf(fabsf(pab), 0.0f), 1.0f), pab);
                ab += (long long)(int)rintf(cab * 1073741824.0f);
                aa += (uint32_t)(int)rintf(fminf(fmaxf(paa, 0.0f), 1.0f) * 1073741824.0f);
                bb += (uint32_t)(int)rintf(fminf(fmaxf(pbb, 0.0f), 1.0f) * 1073741824.0f);
            }
            ab = in_wave_sum(ab);
            aa = (unsigned long long)in_wave_sum((long long)aa);
            bb = (unsigned long long)in_wave_sum((long long)bb);
            if (lane == 0) {
                s_sum[wave][2 * C + 3 * p] = ab;
                s_sum[wave][2 * C + 3 * p + 1] = (long long)aa;
                s_sum[wave][2 * C + 3 * p + 2] = (long long)bb;
            }
        }
    }
    __syncthreads();

    // ---- sums: one store per sum and workgroup into the call's table [stream][sum][tile]
    const uint32_t n_sums = 2 * C + 3 * a.n_pairs;
    if (tid < n_sums) {
        long long v = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) v += s_sum[w][tid];
        a.sums[((uint64_t)s * n_sums + tid) * a.tiles + blockIdx.x] = v;
    }

    // ---- runs: thread p * W + word makes the summary of its word; the W lanes of a predicate compose theirs in frame order
    constexpr uint32_t kWords = (C + 1) * W;
    if ((tid & ~63u) < kWords) {  // (uniform over the wavefront: the shuffles below see all 64 lanes)
        const bool valid = tid < kWords;
        const uint32_t p = tid / W, word = tid % W;
        const uint32_t m = p < (uint32_t)C ? a.clip_min_run : a.silence_min_run;
        const uint32_t lo = word * 64u;
        const uint32_t len = (valid && nf > lo) ? min(64u, nf - lo) : 0u;
        const uint64_t mask = valid ? s_mask[valid ? tid : 0u] : 0ull;
        InRuns r = in_word(mask, len, m);
#pragma unroll
        for (int d = 1; d < (int)W; d <<= 1) r = in_butterfly(r, lane, d, m);
        if (valid && word == 0) {
            v4u* dst = reinterpret_cast<v4u*>(a.runs + ((uint64_t)s * a.tiles + blockIdx.x) * (C + 1) + p);
            dst[0] = v4u{r.len, r.head, r.tail, r.best};
            dst[1] = v4u{r.start, r.reach, r.set, 0u};
        }
    }
}

__global__ __launch_bounds__(kInFoldMaxThreads) void in_fold_kernel(InArgs a, uint32_t s_base) {
    constexpr uint32_t kMaxWaves = kInFoldMaxThreads / 64, kMaxSums = 2 * OMX_MAX_CHANNELS + 3 * OMX_INSPECT_MAX_PAIRS;
    __shared__ InRuns s_part[OMX_MAX_CHANNELS + 1][kMaxWaves];
    __shared__ long long s_tot[kMaxWaves][kMaxSums];
    const uint32_t s = s_base + blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = blockDim.x >> 6;
    const uint32_t frames = a.frames[s];
    if (frames == 0) return;  // (uniform over the workgroup: one stream per workgroup)
    const uint32_t tile = in_tile_frames(a.channels);
    const uint32_t tiles = (uint32_t)(((uint64_t)frames + tile - 1) / tile);
    const uint32_t P = a.channels + 1, n_sums = 2 * a.channels + 3 * a.n_pairs;
    omx_program_inspect_record* rec = a.records + s;
    const uint32_t n0 = (uint32_t)rec->frames;  // (at most 2^32 - 1 - frames: the host refuses more)

    // Every load of a step is issued before the first is used: one wavefront's chain of dependent loads is what this kernel costs.
    {
        long long v[kMaxSums];
#pragma unroll
        for (uint32_t j = 0; j < kMaxSums; ++j) {
            const long long* src = a.sums + ((uint64_t)s * n_sums + min(j, n_sums - 1)) * a.tiles;
            v[j] = (j < n_sums && tid < tiles) ? src[tid] : 0ll;
        }
        for (uint32_t t = tid + blockDim.x; t < tiles; t += blockDim.x) {
#pragma unroll
            for (uint32_t j = 0; j < kMaxSums; ++j)
                if (j < n_sums) v[j] += a.sums[((uint64_t)s * n_sums + j) * a.tiles + t];
        }
#pragma unroll
        for (uint32_t j = 0; j < kMaxSums; ++j) {
            if (j < n_sums) {  // (uniform)
                const long long total = in_wave_sum(v[j]);
                if (lane == 0) s_tot[wave][j] = total;
            }
        }
    }
    const uint32_t chunks = (tiles + 63) / 64, per_wave = (chunks + waves - 1) / waves;
    const uint32_t c0 = min(chunks, wave * per_wave), c1 = min(chunks, c0 + per_wave);
    if (lane <= OMX_MAX_CHANNELS) s_part[lane][wave] = in_identity();
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t t = c * 64 + lane;
        const uint32_t span = min(64u, tiles - c * 64);  // tiles of this chunk: a short call takes fewer butterfly steps
        InRuns r[OMX_MAX_CHANNELS + 1];
#pragma unroll
        for (uint32_t p = 0; p <= OMX_MAX_CHANNELS; ++p) {
            r[p] = in_identity();
            if (p < P && t < tiles) {
                const v4u* src = reinterpret_cast<const v4u*>(a.runs + ((uint64_t)s * a.tiles + t) * P + p);
                const v4u lo = src[0], hi = src[1];
                r[p] = InRuns{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, 0u};
            }
        }
#pragma unroll
        for (uint32_t p = 0; p <= OMX_MAX_CHANNELS; ++p) {
            if (p < P) {  // (uniform)
                const uint32_t m = p < a.channels ? a.clip_min_run : a.silence_min_run;
                InRuns q = r[p];
                for (int d = 1; d < (int)span; d <<= 1) q = in_butterfly(q, lane, d, m);  // (lane 0 wants lanes 0 .. span - 1 only)
                if (lane == 0) s_part[p][wave] = in_compose(s_part[p][wave], q, m);  // (the wavefront's own entry: in order)
            }
        }
    }
    __syncthreads();

    if (tid < n_sums) {  // the record's integer sums: one thread per sum (two's complement: the signed sums add as unsigned ones)
        long long v = 0;
        for (uint32_t w = 0; w < waves; ++w) v += s_tot[w][tid];
        unsigned long long* dst;
        if (tid < 2 * a.channels) {
            omx_program_inspect_channel* ch = rec->channel + (tid >> 1);
            dst = (tid & 1u) ? reinterpret_cast<unsigned long long*>(&ch->nan_samples) : reinterpret_cast<unsigned long long*>(&ch->dc_sum);
        } else {
            const uint32_t j = tid - 2 * a.channels;
            dst = reinterpret_cast<unsigned long long*>(&rec->pair[j / 3].sum_ab) + j % 3;  // sum_ab, sum_aa, sum_bb lie in a row
        }
        *dst += (unsigned long long)v;
    }
    if (tid < P) {  // the record's runs: one thread per predicate
        const uint32_t p = tid;
        const uint32_t m = p < a.channels ? a.clip_min_run : a.silence_min_run;
        InRuns call = in_identity();
        for (uint32_t w = 0; w < waves; ++w) call = in_compose(call, s_part[p][w], m);
        // the running record as the summary of the frames before this call
        InRuns before;
        before.len = n0;
        before._pad = 0;
        if (p < a.channels) {
            omx_program_inspect_channel* ch = rec->channel + p;
            before.tail = (uint32_t)ch->open_clip_run;
            before.head = before.tail == n0 ? n0 : 0u;  // (only "all set or not" is read from it)
            before.best = (uint32_t)ch->longest_clip_run;
            before.start = (uint32_t)ch->longest_clip_start;
            before.reach = (uint32_t)ch->clip_runs;
            before.set = (uint32_t)ch->clipped_samples;
            const InRuns now = in_compose(before, call, m);
            ch->clipped_samples = now.set;
            ch->clip_runs = now.reach;
            ch->longest_clip_run = now.best;
            ch->longest_clip_start = now.start;
            ch->open_clip_run = now.tail;
        } else {
            before.tail = (uint32_t)rec->trailing_silence;
            before.head = (uint32_t)rec->leading_silence;
            before.best = (uint32_t)rec->longest_silent_run;
            before.start = (uint32_t)rec->longest_silent_start;
            before.reach = (uint32_t)rec->silent_runs;
            before.set = (uint32_t)rec->silent_frames;
            const InRuns now = in_compose(before, call, m);
            rec->silent_frames = now.set;
            rec->silent_runs = now.reach;
            rec->longest_silent_run = now.best;
            rec->longest_silent_start = now.start;
            rec->leading_silence = now.head;
            rec->trailing_silence = now.tail;
            rec->frames = (uint64_t)n0 + frames;  // (every thread read n0 in front of the barrier)
        }
    }
}

template <int C>
void in_launch_tiles(const InArgs& a, hipStream_t stream) {
    const uint32_t tiles = std::max<uint32_t>(a.tiles, 1);
    for_stream_slabs(a.n_streams, tiles, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL((in_main_kernel<C>), dim3(tiles, count), dim3(kInThreads), 0, stream, a, base);
    });
}

}  // namespace

void launch_in_reset(const InArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(in_reset_kernel, dim3((a.n_streams + 63) / 64), dim3(64), 0, stream, a);
}
void launch_in_main(const InArgs& a, hipStream_t stream) {
    switch (a.channels) {
        case 1: in_launch_tiles<1>(a, stream); break;
        case 2: in_launch_tiles<2>(a, stream); break;
        case 3: in_launch_tiles<3>(a, stream); break;
        case 4: in_launch_tiles<4>(a, stream); break;
        case 5: in_launch_tiles<5>(a, stream); break;
        case 6: in_launch_tiles<6>(a, stream); break;
        case 7: in_launch_tiles<7>(a, stream); break;
        default: in_launch_tiles<8>(a, stream); break;
    }
}
void launch_in_fold(const InArgs& a, hipStream_t stream) {
    // one workgroup per stream: a wavefront per 64 tiles of the longest stream, 16 at the most
    const uint32_t threads = a.tiles <= 64 ? 64u : (a.tiles <= 256 ? 256u : kInFoldMaxThreads);
    const uint64_t slab = (1ull << 31) / threads;  // fewer than 2^32 threads a launch
    for (uint64_t base = 0; base < a.n_streams; base += slab)
        hipLaunchKernelGGL(in_fold_kernel, dim3((uint32_t)std::min<uint64_t>(slab, a.n_streams - base)), dim3(threads), 0, stream, a, (uint32_t)base);
}

}  // namespace omx

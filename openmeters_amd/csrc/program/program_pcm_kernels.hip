// Integer PCM in and out of the programme loudness bank (include/omx/program_pcm.h): siblings of pn_tile_kernel.
//
// Both passes are bandwidth bound and the NARROW side sets the tile: accesses to the integer buffer are aligned 16-byte vectors (loads
// for import, stores for export), the f32 side takes dwords at 4-byte alignment (the dword form of apply_gains).
//   grid    : x = tiles of a row (kPcTileSamples samples), y = streams in slabs of at most 65535.  Calls are ragged: a tile wholly
//             beyond frames[s] * channels exits at once, before it reads anything but its stream's call entry.
//   rows    : a row is frames_capacity * channels * bytes bytes, so its base A sits at any even (S16), any (S24) or any 4-byte (S32)
//             address.  A0 = A rounded up to 16; the body is the whole runs behind A0: 16 bytes = 8 samples (S16) or 4 samples (S32),
//             48 bytes = 16 samples (S24).  A thread takes 16 samples: two runs, one run, four runs.  Every load is issued before
//             the first store.
//   S24     : h = ceil((A0 - A) / 3) samples start in front of A0, and the body's first sample starts sh = 3 h - (A0 - A) bytes into
//             it (0, 1 or 2: the same for every run of the row, because a run is 48 bytes).  Import: the run's three aligned vectors
//             and, for sh > 0, the dword behind them go through v_alignbyte_b32 by sh, then four samples come out of three dwords by
//             byte-align and sign extension.  Export: sixteen samples are packed into twelve dwords by byte-align, shifted up by sh
//             with the LAST sample of the run before (computed again, not counted again) supplying the first sh bytes; the last sh
//             bytes of the run's sixteenth sample belong to the next run and are written there.  On the f32 side a thread's sixteen
//             floats lie 64 bytes from its neighbour's; the import and the undithered export move them as lane-contiguous vectors and
//             turn the wavefront's 1024 floats through LDS (20 KB per workgroup), which took the import from 1.19 to 0.89 of the
//             yardstick's time.  The TPDF export, bound by its hash, was slower with the turn and reads its floats where they lie.
//   ragged  : the samples in front of A0 and behind the last whole run (at most 7 + 17) are taken by one thread each of tile 0 with
//             byte (S24), short (S16) or dword (S32) accesses.  Two rows may share a dword, a row and its neighbour's unwritten
//             frames too: every store writes bytes of its own row's frames only, none is a read-modify-write.
//   dither  : key_s comes with the call's table; 0x9E37.. * (n * 8 + c) is multiplied out once per run and stepped by additions.
//   reduce  : export counts clipped and NaN samples and takes the maximum |y| per thread, six shuffle steps per wavefront, four
//             wavefronts through LDS, then at most ONE atomicAdd (u64) per count and ONE atomicMax (u32) per workgroup into the
//             stream's record.  Sums of counts and a maximum of integers do not depend on arrival order.
//   Only vector loads, vector stores and vector atomics are used.
#include "program_pcm.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

template <int BYTES>
struct PcFormat;
template <>
struct PcFormat<2> {
    static constexpr uint32_t kBits = 16, kRun = 8, kRuns = 2;
};
template <>
struct PcFormat<3> {
    static constexpr uint32_t kBits = 24, kRun = 16, kRuns = 1;
};
template <>
struct PcFormat<4> {
    static constexpr uint32_t kBits = 32, kRun = 4, kRuns = 4;
};

// Where the aligned body of a row lies.  Uniform over the workgroup.
struct PcRow {
    uint64_t n;        // samples of the row in this call
    uint64_t nrun;     // whole runs of the body
    uint32_t hb;       // bytes in front of the body
    uint32_t head;     // samples that start in front of the body
    uint32_t sh;       // S24: bytes from the body's start to its first sample's start
};
template <int BYTES>
__device__ __forceinline__ PcRow pc_row(uintptr_t base, uint64_t n) {
    constexpr uint32_t RB = PcFormat<BYTES>::kRun * BYTES;
    PcRow r;
    const uint64_t nb = n * BYTES;
    const uint32_t to_aligned = (16u - (uint32_t)(base & 15u)) & 15u;
    r.n = n;
    r.hb = (uint32_t)(to_aligned < nb ? to_aligned : nb);
    r.head = (r.hb + BYTES - 1) / BYTES;
    r.sh = r.head * BYTES - r.hb;
    r.nrun = (nb - r.hb) / RB;
    return r;
}

__device__ __forceinline__ int32_t sext24(uint32_t w) { return (int32_t)(w << 8) >> 8; }

// ---------------------------------------------------------------- import
template <int BYTES>
__device__ __forceinline__ float pc_to_float(int32_t v) {
    return (float)v * (BYTES == 2 ? 0x1p-15f : BYTES == 3 ? 0x1p-23f : 0x1p-31f);
}

template <int BYTES>
__device__ __forceinline__ int32_t pc_read_sample(const uint8_t* p) {  // the ragged ends: p = the sample's first byte
    if (BYTES == 2) return *reinterpret_cast<const int16_t*>(p);
    if (BYTES == 4) return *reinterpret_cast<const int32_t*>(p);
    return sext24((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
}

template <int BYTES>
__global__ __launch_bounds__(kPcThreads) void pc_import_kernel(PcArgs a, uint32_t stream_base) {
    using F = PcFormat<BYTES>;
    const uint32_t s = stream_base + blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const uint64_t n = a.calls[s].n;
    if (n == 0) return;
    const uint8_t* in = static_cast<const uint8_t*>(a.in) + (uint64_t)s * a.row * BYTES;
    float* out = static_cast<float*>(a.out) + (uint64_t)s * a.row;
    const PcRow row = pc_row<BYTES>(reinterpret_cast<uintptr_t>(in), n);
    const uint64_t r0 = (uint64_t)t * (kPcThreads * F::kRuns);
    if (t != 0 && r0 >= row.nrun) return;
    if (t == 0 && tid < 64) {  // the ragged ends: threads 0 .. 31 the head, 32 .. 63 the tail
        const uint64_t tail_first = row.head + row.nrun * F::kRun;
        uint64_t k = n;
        if (tid < 32) {
            if (tid < row.head) k = tid;
        } else {
            k = tail_first + (tid - 32);
        }
        if (k < n) out[k] = pc_to_float<BYTES>(pc_read_sample<BYTES>(in + k * BYTES));
    }
    if (r0 >= row.nrun) return;
    const uint8_t* body = in + row.hb;  // 16-byte aligned
    float* bo = out + row.head;
    const bool full = r0 + kPcThreads * F::kRuns <= row.nrun;
    if constexpr (BYTES != 3) {
        v4u w[F::kRuns];
#pragma unroll
        for (uint32_t k = 0; k < F::kRuns; ++k) {
            const uint64_t r = r0 + k * kPcThreads + tid;
            if (full || r < row.nrun) w[k] = *reinterpret_cast<const v4u*>(body + r * 16);
        }
#pragma unroll
        for (uint32_t k = 0; k < F::kRuns; ++k) {
            const uint64_t r = r0 + k * kPcThreads + tid;
            if (full || r < row.nrun) {
                float* q = bo + r * F::kRun;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (BYTES == 2) {
                        q[2 * j] = pc_to_float<2>((int32_t)(w[k][j] << 16) >> 16);
                        q[2 * j + 1] = pc_to_float<2>((int32_t)w[k][j] >> 16);
                    } else {
                        q[j] = pc_to_float<4>((int32_t)w[k][j]);
                    }
                }
            }
        }
    } else {
        // A thread's sixteen floats lie 64 bytes from its neighbour's, and stores of that shape ran at 0.84 of the rate of
        // lane-contiguous ones ("PCM formats"): the wavefront turns its 1024 floats through LDS (rows of 80 bytes,
        // so that the 16-byte writes of sixteen lanes fall on distinct banks) and stores them as lane-contiguous vectors.
        constexpr uint32_t kRowVecs = 5;
        __shared__ v4f s_turn[kPcThreads / 64][64 * kRowVecs];
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        const uint64_t r = r0 + tid;
        v4f f[4] = {};
        if (full || r < row.nrun) {
            const uint8_t* p = body + r * 48;
            uint32_t w[13];
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                const v4u v = *reinterpret_cast<const v4u*>(p + 16 * k);
                w[4 * k] = v.x;
                w[4 * k + 1] = v.y;
                w[4 * k + 2] = v.z;
                w[4 * k + 3] = v.w;
            }
            // sh > 0: the run's last sample ends sh bytes into the next dword, which therefore holds bytes of this row
            w[12] = row.sh != 0 ? *reinterpret_cast<const uint32_t*>(p + 48) : 0u;
#pragma unroll
            for (uint32_t k = 0; k < 12; ++k) w[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], row.sh);
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) {  // four samples in three dwords
                const uint32_t d0 = w[3 * g], d1 = w[3 * g + 1], d2 = w[3 * g + 2];
                f[g] = v4f{pc_to_float<3>(sext24(d0)), pc_to_float<3>(sext24(__builtin_amdgcn_alignbyte(d1, d0, 3))),
                           pc_to_float<3>(sext24(__builtin_amdgcn_alignbyte(d2, d1, 2))), pc_to_float<3>((int32_t)d2 >> 8)};
            }
        }
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) s_turn[wave][lane * kRowVecs + g] = f[g];
        __syncthreads();  // (every thread of the workgroup arrives: the returns above are uniform)
        const uint64_t wave_run = r0 + wave * 64;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t m = k * 64 + lane;  // vector m of the wavefront's 256: floats 4 m .. 4 m + 3 of run m / 4
            if (full || wave_run + (m >> 2) < row.nrun) {
                const v4f v = s_turn[wave][(m >> 2) * kRowVecs + (m & 3u)];
                float* q = bo + wave_run * 16 + 4 * m;
                q[0] = v.x;
                q[1] = v.y;
                q[2] = v.z;
                q[3] = v.w;
            }
        }
    }
}

// ---------------------------------------------------------------- export
__global__ __launch_bounds__(64) void pc_export_begin_kernel(PcArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const PcStreamCall c = a.calls[s];
    omx_program_export_record* r = a.records + s;
    if (c.flags & kPcFlagKeep) return;
    if (c.flags & kPcFlagClear) {
        r->samples_clipped = 0;
        r->samples_nan = 0;
        r->out_peak = 0;
        r->out_peak_db = a.floor_db;
    }
    const uint64_t frames = c.n / a.channels;
    r->frames_out = c.pos + frames;
    r->frames_written = frames;
    r->format = a.format;
    r->dither = a.dither;
}

__global__ __launch_bounds__(64) void pc_export_finish_kernel(PcArgs a) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_streams) return;
    const uint32_t bits = a.format == OMX_PCM_S16 ? 16u : a.format == OMX_PCM_S24 ? 24u : 32u;
    const float p = (float)((double)a.records[s].out_peak / (double)(1ull << (bits - 1)));
    a.records[s].out_peak_db = ps_peak_db(p, a.floor_db);
}

struct PcTally {
    uint32_t clipped, nans, peak;
};

// The dither position of sample i of the row: frame pos + i / channels, channel i % channels, as the counter kPcGolden * (n * 8 + c).
struct PcCursor {
    uint64_t counter;
    uint32_t c;
};
__device__ __forceinline__ PcCursor pc_cursor(uint64_t pos, uint64_t frame, uint32_t c) {
    return PcCursor{kPcGolden * ((pos + frame) * 8 + c), c};
}
__device__ __forceinline__ void pc_step(PcCursor& k, uint32_t channels, uint64_t wrap) {
    k.counter += kPcGolden;
    if (++k.c == channels) {
        k.c = 0;
        k.counter += wrap;  // kPcGolden * (8 - channels): from channel channels - 1 of one frame to channel 0 of the next
    }
}

template <int BYTES, bool TPDF>
__device__ __forceinline__ int32_t pc_sample(float x, uint64_t key, const PcCursor& k, PcTally& tally) {
    const double d = TPDF ? pc_dither(key, k.counter) : 0.0;
    return pc_quantise<PcFormat<BYTES>::kBits>(x, d, tally.clipped, tally.nans, tally.peak);
}

template <int BYTES, bool TPDF>
__global__ __launch_bounds__(kPcThreads) void pc_export_kernel(PcArgs a, uint32_t stream_base) {
    using F = PcFormat<BYTES>;
    const uint32_t s = stream_base + blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const PcStreamCall call = a.calls[s];
    const uint64_t n = call.n;
    if (n == 0) return;
    const float* in = static_cast<const float*>(a.in) + (uint64_t)s * a.row;
    uint8_t* out = static_cast<uint8_t*>(a.out) + (uint64_t)s * a.row * BYTES;
    const PcRow row = pc_row<BYTES>(reinterpret_cast<uintptr_t>(out), n);
    const uint64_t r0 = (uint64_t)t * (kPcThreads * F::kRuns);
    if (t != 0 && r0 >= row.nrun) return;  // (uniform over the workgroup, as the return above: no thread is left at the barrier below)
    const uint32_t ch = a.channels;
    const uint64_t wrap = kPcGolden * (uint64_t)(8u - ch);
    uint8_t* body = out + row.hb;  // 16-byte aligned
    PcTally tally{0, 0, 0}, unused{0, 0, 0};

    if (t == 0 && tid < 64) {  // the ragged ends: threads 0 .. 31 the head, 32 .. 63 the tail
        // S24: with sh > 0 the body's last sample ends in the tail; its thread here writes those bytes and counts nothing
        const bool straddle = BYTES == 3 && row.sh != 0 && row.nrun != 0;
        const uint64_t tail_first = row.head + row.nrun * F::kRun - (straddle ? 1u : 0u);
        uint64_t k = n;
        if (tid < 32) {
            if (tid < row.head) k = tid;
        } else {
            k = tail_first + (tid - 32);
        }
        if (k < n) {
            const PcCursor cur = pc_cursor(call.pos, k / ch, (uint32_t)(k % ch));
            uint8_t* p = out + k * BYTES;
            const uint8_t *lo = body, *hi = body + row.nrun * (F::kRun * BYTES);  // the body's bytes are not written from here
            const bool counted = !(p >= lo && p < hi);
            const int32_t y = pc_sample<BYTES, TPDF>(in[k], call.key, cur, counted ? tally : unused);
            if (BYTES == 2) {
                *reinterpret_cast<int16_t*>(p) = (int16_t)y;
            } else if (BYTES == 4) {
                *reinterpret_cast<int32_t*>(p) = y;
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 3; ++b)
                    if (!(p + b >= lo && p + b < hi)) p[b] = (uint8_t)((uint32_t)y >> (8 * b));
            }
        }
    }

    if (r0 < row.nrun) {
        const float* bi = in + row.head;
        const bool full = r0 + kPcThreads * F::kRuns <= row.nrun;
        // frame and channel of the tile's first body sample, once; a run's own follow from 32-bit arithmetic
        const uint64_t i0 = row.head + r0 * F::kRun;
        const uint64_t f0 = TPDF ? i0 / ch : 0;
        const uint32_t c0 = TPDF ? (uint32_t)(i0 % ch) : 0;
        float x[F::kRuns][F::kRun];
        float x_prev = 0.0f;
        if constexpr (BYTES == 3 && !TPDF) {
            // the mirror image of the import: the wavefront loads its 1024 floats as lane-contiguous vectors and turns them through
            // LDS, so that every thread gets the sixteen samples of its run.  Not with TPDF: that form is bound by the hash, and the
            // turn's barrier cost it 6 % (0.246 -> 0.262 ms on 1024 x 8 ch x 16 384 frames) where it gained the plain form 8 %.
            constexpr uint32_t kRowVecs = 5;
            __shared__ v4f s_turn[kPcThreads / 64][64 * kRowVecs];
            const uint32_t wave = tid >> 6, lane = tid & 63u;
            const uint64_t wave_run = r0 + wave * 64, r = r0 + tid;
            v4f v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t m = k * 64 + lane;  // vector m of the wavefront's 256: floats 4 m .. 4 m + 3 of run m / 4
                v[k] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
                if (full || wave_run + (m >> 2) < row.nrun) {
                    const float* p = bi + wave_run * 16 + 4 * m;
                    v[k] = v4f{p[0], p[1], p[2], p[3]};
                }
            }
            if ((full || r < row.nrun) && row.sh != 0) x_prev = bi[r * 16 - 1];  // (sh > 0 means head >= 1: the sample exists)
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t m = k * 64 + lane;
                s_turn[wave][(m >> 2) * kRowVecs + (m & 3u)] = v[k];
            }
            __syncthreads();  // (r0 < nrun holds for the whole workgroup or for none of it)
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) {
                const v4f u = s_turn[wave][lane * kRowVecs + g];
                x[0][4 * g] = u.x;
                x[0][4 * g + 1] = u.y;
                x[0][4 * g + 2] = u.z;
                x[0][4 * g + 3] = u.w;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < F::kRuns; ++k) {
                const uint64_t r = r0 + k * kPcThreads + tid;
                if (full || r < row.nrun) {
                    const float* p = bi + r * F::kRun;
#pragma unroll
                    for (uint32_t j = 0; j < F::kRun; ++j) x[k][j] = p[j];
                    if (BYTES == 3 && row.sh != 0) x_prev = p[-1];  // (sh > 0 means head >= 1: the sample exists)
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < F::kRuns; ++k) {
            const uint64_t r = r0 + k * kPcThreads + tid;
            if (full || r < row.nrun) {
                const uint32_t local = c0 + (k * kPcThreads + tid) * F::kRun;  // below 2^13
                PcCursor cur = pc_cursor(call.pos, f0 + local / ch, local % ch);
                int32_t y[F::kRun];
                int32_t y_prev = 0;
                if (BYTES == 3 && row.sh != 0) {
                    PcCursor before;
                    before.c = (cur.c == 0 ? ch : cur.c) - 1;
                    before.counter = cur.counter - kPcGolden - (cur.c == 0 ? wrap : 0);
                    y_prev = pc_sample<BYTES, TPDF>(x_prev, call.key, before, unused);
                }
#pragma unroll
                for (uint32_t j = 0; j < F::kRun; ++j) {
                    y[j] = pc_sample<BYTES, TPDF>(x[k][j], call.key, cur, tally);
                    pc_step(cur, ch, wrap);
                }
                if (BYTES == 2) {
                    v4u w;
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) w[j] = ((uint32_t)y[2 * j] & 0xFFFFu) | ((uint32_t)y[2 * j + 1] << 16);
                    *reinterpret_cast<v4u*>(body + r * 16) = w;
                } else if (BYTES == 4) {
                    *reinterpret_cast<v4u*>(body + r * 16) = v4u{(uint32_t)y[0], (uint32_t)y[1], (uint32_t)y[2], (uint32_t)y[3]};
                } else {
                    uint32_t w[13];  // w[0]: the sample before the run in its top three bytes; w[1 .. 12]: the run, packed
                    w[0] = (uint32_t)y_prev << 8;
#pragma unroll
                    for (uint32_t g = 0; g < 4; ++g) {  // four samples into three dwords
                        const uint32_t y0 = (uint32_t)y[4 * g], y1 = (uint32_t)y[4 * g + 1], y2 = (uint32_t)y[4 * g + 2], y3 = (uint32_t)y[4 * g + 3];
                        w[1 + 3 * g] = __builtin_amdgcn_alignbyte(y1, y0 << 8, 1);
                        w[2 + 3 * g] = __builtin_amdgcn_alignbyte(y2, y1 << 8, 2);
                        w[3 + 3 * g] = __builtin_amdgcn_alignbyte(y3, y2 << 8, 3);
                    }
                    uint32_t o[12];
                    if (row.sh == 0) {
#pragma unroll
                        for (uint32_t i = 0; i < 12; ++i) o[i] = w[i + 1];
                    } else {  // the top sh bytes of the dword before, then the low 4 - sh bytes of this one
#pragma unroll
                        for (uint32_t i = 0; i < 12; ++i) o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], 4u - row.sh);
                    }
                    uint8_t* p = body + r * 48;
#pragma unroll
                    for (uint32_t i = 0; i < 3; ++i) *reinterpret_cast<v4u*>(p + 16 * i) = v4u{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
                }
            }
        }
    }

#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ps_fold_step(tally.clipped, PsSum{}, d);
        ps_fold_step(tally.nans, PsSum{}, d);
        ps_fold_step(tally.peak, PsMax{}, d);
    }
    __shared__ uint32_t s_clipped[kPcThreads / 64], s_nans[kPcThreads / 64], s_peak[kPcThreads / 64];
    ps_fold_post(tally.clipped, s_clipped);
    ps_fold_post(tally.nans, s_nans);
    ps_fold_post(tally.peak, s_peak);
    __syncthreads();
    if (tid == 0) {
        ps_fold_gather<kPcThreads>(tally.clipped, PsSum{}, s_clipped);
        ps_fold_gather<kPcThreads>(tally.nans, PsSum{}, s_nans);
        ps_fold_gather<kPcThreads>(tally.peak, PsMax{}, s_peak);
        omx_program_export_record* r = a.records + s;
        if (tally.clipped != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->samples_clipped), (unsigned long long)tally.clipped);
        if (tally.nans != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&r->samples_nan), (unsigned long long)tally.nans);
        if (tally.peak != 0) atomicMax(&r->out_peak, tally.peak);
    }
}

// tiles of the longest row (its body is at most max_n / 16 threads' worth; tile 0 exists for every row that brings a sample)
template <class Launch>
void pc_slabs(uint64_t max_n, uint32_t n_streams, Launch&& launch) {
    const uint64_t tiles = std::max<uint64_t>((max_n + kPcTileSamples - 1) / kPcTileSamples, 1);
    for_stream_slabs(n_streams, tiles, [&](uint32_t base, uint32_t count) { launch(dim3((uint32_t)tiles, count), base); });
}

}  // namespace

void launch_pc_import(const PcArgs& a, uint64_t max_n, hipStream_t stream) {
    pc_slabs(max_n, a.n_streams, [&](dim3 grid, uint32_t base) {
        if (a.format == OMX_PCM_S16) hipLaunchKernelGGL(pc_import_kernel<2>, grid, dim3(kPcThreads), 0, stream, a, base);
        else if (a.format == OMX_PCM_S24) hipLaunchKernelGGL(pc_import_kernel<3>, grid, dim3(kPcThreads), 0, stream, a, base);
        else hipLaunchKernelGGL(pc_import_kernel<4>, grid, dim3(kPcThreads), 0, stream, a, base);
    });
}
void launch_pc_export_begin(const PcArgs& a, hipStream_t stream) {
    ps_launch_per_stream(pc_export_begin_kernel, a.n_streams, stream, a);
}
void launch_pc_export_finish(const PcArgs& a, hipStream_t stream) {
    ps_launch_per_stream(pc_export_finish_kernel, a.n_streams, stream, a);
}
void launch_pc_export(const PcArgs& a, uint64_t max_n, hipStream_t stream) {
    const bool tpdf = a.dither == OMX_DITHER_TPDF;
    pc_slabs(max_n, a.n_streams, [&](dim3 grid, uint32_t base) {
#define OMX_PC_EXPORT(BYTES)                                                                                                  \
    do {                                                                                                                      \
        if (tpdf) hipLaunchKernelGGL((pc_export_kernel<BYTES, true>), grid, dim3(kPcThreads), 0, stream, a, base);            \
        else hipLaunchKernelGGL((pc_export_kernel<BYTES, false>), grid, dim3(kPcThreads), 0, stream, a, base);                \
    } while (0)
        if (a.format == OMX_PCM_S16) OMX_PC_EXPORT(2);
        else if (a.format == OMX_PCM_S24) OMX_PC_EXPORT(3);
        else OMX_PC_EXPORT(4);
#undef OMX_PC_EXPORT
    });
}

}  // namespace omx

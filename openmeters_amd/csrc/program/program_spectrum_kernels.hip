// Long-term spectrum of the programme loudness bank (include/omx/program_spectrum.h states the definition, program_spectrum.hpp the
// passes and the call table).
//
//   begin     : a thread per stream adds the call's frames to the record and sets its finish flag.
//   transform : grid (units / FR, stream), 256 threads.  A unit is one channel's part of one run of R transforms; a workgroup runs FR
//               = 4, 2 or 1 units side by side at N = 2048, 4096, 8192 (N/32 threads carry one transform, fft_pow2_device.hpp at N/2
//               complex points).  Units are numbered run-major, channel-minor, so neighbouring slots and workgroups read the same
//               frames.  Per transform a thread loads its 32 samples (m = j + T u: frames 2m and 2m + 1) from the carried frames
//               or from d_in, whichever holds the frame, and zero behind a finished stream's last frame; it multiplies by the
//               window, takes part in the complex transform of (y[2m], y[2m+1]) in LDS, writes Z back in natural order and reads
//               the partner Z[N/2 - b] of each of its bins b = j + T u: X[b] = E[b] + w^b O[b] with E, O the even and odd halves,
//               p = |X|^2; thread 0 also makes the Nyquist bin from Z[0].  A transform is ONE channel's ONE frame: nothing else
//               rides in the imaginary half.  The run's chain lives in 17 f64 registers per thread, which owns its bins for the
//               whole run: it starts from the stream's open run when the call continues one, else from zero, and ends in the
//               run's scratch row, complete or not.  A non-finite sample raises a flag in LDS and the whole
//               transform is left out.  The counts go to the record as two integer atomic adds per unit.
//               Every slot of a workgroup makes the same number of trips (the longest of its units): the barriers of the transform
//               are the workgroup's at N = 4096 and 8192.
//   chain     : grid (bins / 256, channel, stream): closed += the call's complete runs in ascending run order; the row of a run the call
//               leaves open becomes the stream's open run; S = closed + open.
//   carry     : grid (floats / 1024, stream): the frames from the next transform's start on go to the other carry buffer, or,
//               when the call took no transform, the new frames are appended in place.  It runs behind the transform pass, which
//               reads the current buffer.
//   No kernel walks a stream's frames: a unit is at most R transforms, the chain pass walks one value per R * N / 2 frames.
//   Only vector loads and vector stores are used; the only atomics are the integer counts.
#define OMX_FRAME_SYNC_LDS_ONLY 1  // the transforms of this file exchange data through LDS only (fft_pow2_device.hpp: frame_sync)
#include "../fft_pow2_device.hpp"
#include "program_spectrum.hpp"
#include "program_stage_device.hpp"

namespace omx {
namespace {

__global__ void sp_reset_kernel(SpArgs a, uint32_t base) {
    const uint32_t s = base + blockIdx.y;
    if (a.calls[s].frames == 0) return;
    const uint32_t bins = a.fft_size / 2 + 1, per = a.channels * bins;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < per) {
        const uint64_t at = (uint64_t)s * per + i;
        a.sums[at] = 0.0;
        a.closed[at] = 0.0;
        a.open[at] = 0.0;
    }
    if (i == 0) {
        omx_program_spectrum_record r{};
        r.fft_size = a.fft_size;
        r.channels = a.channels;
        a.records[s] = r;
    }
}

__global__ void sp_begin_kernel(SpArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_streams) return;
    const SpCall call = a.calls[s];
    if (call.frames) a.records[s].frames += call.frames;
    if (call.finish) a.records[s].finished = 1;
}

template <int LOGM>
__global__ __launch_bounds__(256) void sp_transform_kernel(SpArgs a, uint32_t base) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::N, T = G::T, FR = 256 / T;  // M = N / 2 complex points, the hop
    constexpr uint32_t R = kSpRun;
    __shared__ v2f buf[FR][G::LDS];
    __shared__ v2f tw2_lds[256];
    __shared__ uint32_t bad[FR][4];

    const uint32_t s = base + blockIdx.y;
    const SpCall call = a.calls[s];
    if (call.nk == 0) return;
    const uint32_t ch = a.channels;
    const uint32_t k0 = call.k0, k1 = k0 + call.nk;
    const uint32_t j0 = k0 / R, units = ((k1 - 1) / R - j0 + 1) * ch;
    const uint32_t unit0 = blockIdx.x * (uint32_t)FR;
    if (unit0 >= units) return;  // (the whole workgroup)
    tw2_lds[threadIdx.x] = reinterpret_cast<const v2f*>(a.tw256)[threadIdx.x];
    __syncthreads();

    const int slot = (int)threadIdx.x / T, jf = (int)threadIdx.x % T;
    const uint32_t unit = unit0 + (uint32_t)slot;
    const bool live = unit < units;
    const uint32_t c = live ? unit % ch : 0, j = j0 + (live ? unit / ch : 0);
    const uint32_t ka = max(j * R, k0), kb = live ? min(j * R + R, k1) : ka;  // the unit's transforms [ka, kb)
    uint32_t trips = 0;
#pragma unroll
    for (int q = 0; q < FR; ++q) {
        const uint32_t u = unit0 + (uint32_t)q;
        if (u < units) {
            const uint32_t jq = j0 + u / ch;
            trips = max(trips, min(jq * R + R, k1) - max(jq * R, k0));
        }
    }

    const uint32_t bins = (uint32_t)M + 1;
    const uint64_t state_at = ((uint64_t)s * ch + c) * bins;
    double acc[16], acc_ny = 0.0;
    const bool resumes = live && ka > j * R;  // the call continues the stream's open run
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = resumes ? a.open[state_at + (uint32_t)(jf + T * u)] : 0.0;
    if (resumes && jf == 0) acc_ny = a.open[state_at + (uint32_t)M];

    TwiddlesPow2<LOGM> tw;
    tw.tw2 = tw2_lds;
    tw.load(reinterpret_cast<const v2f*>(a.tw_half), (unsigned)jf);
    const v2f* win = reinterpret_cast<const v2f*>(a.window);
    const v2f* wn = reinterpret_cast<const v2f*>(a.tw_full);
    const float* cur = a.carry + ((uint64_t)call.parity * a.n_streams + s) * ((uint64_t)2 * M) * ch;
    const float* in = a.in + (uint64_t)s * a.frames_capacity * ch;
    const uint64_t carried = call.carried, brought = call.frames;
    v2f* lds = buf[slot];
    uint32_t taken = 0, left_out = 0;

    for (uint32_t i = 0; i < trips; ++i) {
        const uint32_t k = ka + i;
        const bool act = k < kb;
        if (jf == 0) bad[slot][0] = 0;
        v2f v[16];
        bool nonfinite = false;
        if (act) {
            const uint64_t first = (uint64_t)(k - k0) * (uint64_t)M;  // the logical frame the transform starts at
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const uint32_t m = (uint32_t)(jf + T * u);
                float x[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint64_t at = first + 2u * m + (uint32_t)h;
                    float value = 0.0f;
                    if (at < carried) value = cur[at * ch + c];
                    else if (at - carried < brought) value = in[(at - carried) * ch + c];
                    x[h] = value;
                    nonfinite |= !(fabsf(value) <= 3.402823466e38f);
                }
                const v2f w = win[m];
                v[u] = v2f{x[0] * w.x, x[1] * w.y};
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = v2f{0.0f, 0.0f};
        }
        frame_sync<LOGM>();
        if (nonfinite) bad[slot][0] = 1;
        fftp_inplace<false, LOGM>(v, lds, jf, tw);
        frame_sync<LOGM>();
        const int own = pad16(jf);  // pad16(jf + T t) = pad16(jf) + (T + T / 16) t
#pragma unroll
        for (int t = 0; t < 16; ++t) lds[own + (T + T / 16) * t] = v[t];
        frame_sync<LOGM>();
        const bool keep = act && bad[slot][0] == 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int b = jf + T * u;
            const v2f z = v[u], zr = lds[pad16((M - b) & (M - 1))], w = wn[b];
            const v2f e{0.5f * (z.x + zr.x), 0.5f * (z.y - zr.y)};
            const v2f o{0.5f * (z.y + zr.y), -0.5f * (z.x - zr.x)};
            const float re = e.x + (w.x * o.x - w.y * o.y), im = e.y + (w.x * o.y + w.y * o.x);
            const float p = re * re + im * im;
            if (keep) acc[u] += (double)p;
        }
        if (jf == 0) {
            const float ny = v[0].x - v[0].y;
            if (keep) acc_ny += (double)(ny * ny);
            if (act) {
                taken += keep ? 1u : 0u;
                left_out += keep ? 0u : 1u;
            }
        }
        frame_sync<LOGM>();  // (the next trip rewrites the buffer and the flag)
    }

    if (!live || kb == ka) return;
    // (an open run goes to its row as well: another workgroup of this launch may still be reading the stream's open run)
    double* out = a.rows + (((uint64_t)s * ch + c) * a.max_rows + (j - j0)) * bins;
#pragma unroll
    for (int u = 0; u < 16; ++u) out[jf + T * u] = acc[u];
    if (jf == 0) {
        out[M] = acc_ny;
        if (taken) atomicAdd(reinterpret_cast<unsigned long long*>(&a.records[s].transforms[c]), (unsigned long long)taken);
        if (left_out) atomicAdd(reinterpret_cast<unsigned long long*>(&a.records[s].skipped[c]), (unsigned long long)left_out);
    }
}

__global__ void sp_chain_kernel(SpArgs a, uint32_t base) {
    const uint32_t s = base + blockIdx.z;
    const SpCall call = a.calls[s];
    if (call.nk == 0) return;
    const uint32_t bins = a.fft_size / 2 + 1, b = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (b >= bins) return;
    const uint32_t k1 = call.k0 + call.nk, rows = k1 / kSpRun - call.k0 / kSpRun;
    const uint64_t at = ((uint64_t)s * a.channels + c) * bins + b;
    const double* row = a.rows + ((uint64_t)s * a.channels + c) * a.max_rows * bins + b;
    double sum = a.closed[at];
    for (uint32_t r = 0; r < rows; ++r) sum += row[(uint64_t)r * bins];
    if (rows) a.closed[at] = sum;
    const double open = k1 % kSpRun ? row[(uint64_t)rows * bins] : 0.0;  // the row behind the complete ones
    a.open[at] = open;
    a.sums[at] = sum + open;
}

__global__ void sp_carry_kernel(SpArgs a, uint32_t base) {
    const uint32_t s = base + blockIdx.y;
    const SpCall call = a.calls[s];
    if (call.finish) return;
    const uint32_t ch = a.channels, n = a.fft_size;
    const uint64_t had = (uint64_t)call.carried * ch, brought = (uint64_t)call.frames * ch, skip = (uint64_t)call.shift * ch;
    const uint64_t from = call.shift ? 0 : had, to = (uint64_t)call.keep * ch;
    const float* cur = a.carry + ((uint64_t)call.parity * a.n_streams + s) * (uint64_t)n * ch;
    float* dst = a.carry + ((uint64_t)(call.shift ? call.parity ^ 1u : call.parity) * a.n_streams + s) * (uint64_t)n * ch;
    const float* in = a.in + (uint64_t)s * a.frames_capacity * ch;
    for (uint64_t e = from + (uint64_t)blockIdx.x * 1024 + threadIdx.x, q = 0; q < 4 && e < to; ++q, e += 256) {
        const uint64_t at = e + skip;
        float value = 0.0f;
        if (at < had) value = cur[at];
        else if (at - had < brought) value = in[at - had];
        dst[e] = value;
    }
}

template <int LOGM>
void sp_launch_transform(const SpArgs& a, hipStream_t stream) {
    constexpr uint32_t FR = 256 / FftGeom<LOGM>::T;
    const uint32_t groups = (a.max_units + FR - 1) / FR;
    for_stream_slabs(a.n_streams, groups, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL((sp_transform_kernel<LOGM>), dim3(groups, count), dim3(256), 0, stream, a, base);
    });
}

}  // namespace

void launch_sp_reset(const SpArgs& a, hipStream_t stream) {
    const uint32_t blocks = (a.channels * (a.fft_size / 2 + 1) + 255) / 256;
    for_stream_slabs(a.n_streams, blocks, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(sp_reset_kernel, dim3(blocks, count), dim3(256), 0, stream, a, base);
    });
}
void launch_sp_begin(const SpArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(sp_begin_kernel, dim3((a.n_streams + 63) / 64), dim3(64), 0, stream, a);
}
void launch_sp_transform(const SpArgs& a, hipStream_t stream) {
    if (a.max_units == 0) return;
    switch (a.fft_size) {
        case 2048: sp_launch_transform<10>(a, stream); break;
        case 4096: sp_launch_transform<11>(a, stream); break;
        default: sp_launch_transform<12>(a, stream); break;
    }
}
void launch_sp_chain(const SpArgs& a, hipStream_t stream) {
    if (a.max_units == 0) return;
    const uint32_t blocks = (a.fft_size / 2 + 1 + 255) / 256;
    for_stream_slabs(a.n_streams, (uint64_t)blocks * a.channels, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(sp_chain_kernel, dim3(blocks, a.channels, count), dim3(256), 0, stream, a, base);
    });
}
void launch_sp_carry(const SpArgs& a, hipStream_t stream) {
    if (a.max_move == 0) return;
    const uint32_t blocks = (a.max_move + 1023) / 1024;
    for_stream_slabs(a.n_streams, blocks, [&](uint32_t base, uint32_t count) {
        hipLaunchKernelGGL(sp_carry_kernel, dim3(blocks, count), dim3(256), 0, stream, a, base);
    });
}

}  // namespace omx

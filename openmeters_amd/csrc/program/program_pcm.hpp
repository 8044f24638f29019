// Integer PCM in and out of the programme loudness bank (include/omx/program_pcm.h): the dither and the quantiser as ONE set of inline
// functions for the host (omx_program_dither_evaluate) and the device (the export kernel of program_pcm_kernels.hip), so they cannot
// drift apart, and the two passes' launchers.  program_pcm.cpp validates on the host and uploads one small table per call.
#pragma once
#include "../common.hpp"
#include "../../../include/omx/program_pcm.h"

namespace omx {

constexpr uint64_t kPcGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t pc_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline uint64_t pc_stream_key(uint64_t seed, uint64_t stream) { return pc_mix(seed + kPcGolden * (stream + 1)); }
// counter = kPcGolden * (frame * 8 + channel): it steps by a constant from one sample to the next, so the kernel carries it
__host__ __device__ inline double pc_dither(uint64_t key, uint64_t counter) {
    const uint64_t h = pc_mix(key + counter);
    const int32_t a = (int32_t)(h & 0xFFFFFFu), b = (int32_t)((h >> 24) & 0xFFFFFFu);
    return (double)(a - b) * 0x1p-24;  // |a - b| < 2^24: the difference and the product are exact
}

// One sample of the export: scale, dither, round, clamp in f64, every step its own operation (the library is built with
// -ffp-contract=off).  A NaN gives 0 and counts only as a NaN.
template <int BITS>
__host__ __device__ inline int32_t pc_quantise(float x, double d, uint32_t& clipped, uint32_t& nans, uint32_t& peak) {
    constexpr double full = (double)(1ull << (BITS - 1));
    const bool nan = x != x;
    const double sv = (double)(nan ? 0.0f : x) * full;
    const double t = sv + d;
    const double r = floor(t + 0.5);
    const bool out = r < -full || r > full - 1.0;
    const double y = r < -full ? -full : (r > full - 1.0 ? full - 1.0 : r);
    const int32_t yi = nan ? 0 : (int32_t)y;
    clipped += (out && !nan) ? 1u : 0u;
    nans += nan ? 1u : 0u;
    const uint32_t m = yi < 0 ? 0u - (uint32_t)yi : (uint32_t)yi;
    peak = m > peak ? m : peak;
    return yi;
}

inline uint32_t pc_format_bytes(uint32_t format) {  // 0: unknown
    return format == OMX_PCM_S16 ? 2u : format == OMX_PCM_S24 ? 3u : format == OMX_PCM_S32 ? 4u : 0u;
}

// What one import or export call does to one stream: made on the host, uploaded per call.
constexpr uint32_t kPcFlagClear = 1u;  // the stream's export record starts over
constexpr uint32_t kPcFlagKeep = 2u;   // a reset that does not name the stream: its record stays as it is
struct PcStreamCall {
    uint64_t n;      // samples: frames * channels
    uint64_t pos;    // export: frames exported before this call (the host's mirror)
    uint64_t key;    // export: key_s of the dither
    uint32_t flags;
    uint32_t _pad;
};

// Both passes move a row in tiles of kPcTileSamples samples: 256 threads, 16 samples each, in runs that are whole aligned 16-byte
// vectors of the integer buffer (S16: 2 runs of 8 samples; S24: 1 run of 16 samples = 48 bytes; S32: 4 runs of 4 samples).
constexpr uint32_t kPcThreads = 256, kPcSamplesPerThread = 16;
constexpr uint32_t kPcTileSamples = kPcThreads * kPcSamplesPerThread;

struct PcArgs {
    const void* in;   // import: integer PCM; export: f32
    void* out;        // import: f32; export: integer PCM
    uint64_t row;     // samples per row: frames_capacity * channels
    const PcStreamCall* calls;           // [n_streams]
    omx_program_export_record* records;  // [n_streams], export only
    uint32_t n_streams, channels, format, dither;
    float floor_db;
};
// import: the pass alone (not launched without frames).  export: begin (positions, this call's frame counts, cleared records), the
// pass, finish (the peak's dB field).  max_n = the longest row of the call in samples.
void launch_pc_import(const PcArgs& a, uint64_t max_n, hipStream_t stream);
void launch_pc_export_begin(const PcArgs& a, hipStream_t stream);
void launch_pc_export(const PcArgs& a, uint64_t max_n, hipStream_t stream);
void launch_pc_export_finish(const PcArgs& a, hipStream_t stream);

struct ProgramExporter {
    omx_program_export_rule rule{};
    uint32_t channels = 0;
    std::vector<uint64_t> h_pos;  // frames exported since the reset, per stream
    std::vector<PcStreamCall> h_calls;
    DeviceBuffer<PcStreamCall> calls;
    DeviceBuffer<omx_program_export_record> records;
    BlobStaging staging;
};

}  // namespace omx

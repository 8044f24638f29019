// What the stages of the programme loudness bank share on the host: the refusal of a bad call, the checks a call makes on its
// channel count, its frame counts and its device ranges before it touches anything, the taps of the true-peak interpolators and the
// upload of a call's per-stream table.  All inline: nothing here is compiled on its own.  program_carried.hpp holds what the stages
// that carry state between calls share beyond that.
#pragma once
#include "../common.hpp"
#include "program_carried.hpp"

namespace omx {

// The refusal of a call whose arguments are wrong: OMX_ERR_INVALID, with "program loudness <who>: <why>" as the last error
inline int pl_refuse(const char* who, const char* why) {
    set_last_error(std::string("program loudness ") + who + ": " + why);
    return OMX_ERR_INVALID;
}

inline bool pl_channels_ok(uint32_t c) { return c >= 1 && c <= OMX_MAX_CHANNELS; }

// a row's frames are counted in 32 bits on the device
inline bool pl_capacity_ok(uint64_t frames_capacity) { return frames_capacity <= 0xFFFFFFFFull; }

// The frames stream s brings to a call: frames[s], or the whole row where the call gives no counts.  False, with the refusal set,
// when frames[s] exceeds the row.
inline bool pl_stream_frames(const char* who, const uint32_t* frames, uint64_t frames_capacity, uint32_t s, uint64_t& f) {
    const char* why = carry_frames_of(frames, frames_capacity, s, f);
    if (why) pl_refuse(who, why);
    return !why;
}

// [a, a + bytes_a) and [b, b + bytes_b) share a byte
inline bool pl_ranges_overlap(const void* a, unsigned __int128 bytes_a, const void* b, unsigned __int128 bytes_b) {
    const unsigned __int128 lo_a = reinterpret_cast<uintptr_t>(a), lo_b = reinterpret_cast<uintptr_t>(b);
    return bytes_a != 0 && bytes_b != 0 && lo_a < lo_b + bytes_b && lo_b < lo_a + bytes_a;
}
// The out-of-place test of the carried stages (a tile would read what another has already written): the PCM of d_in,
// [n_streams][frames_capacity][channels], and the rows of d_out, out_capacity frames of frame_floats f32 per stream, share a byte
inline bool pl_in_out_overlap(const float* d_in, uint64_t frames_capacity, const float* d_out, uint64_t out_capacity, uint32_t n_streams,
                              uint32_t channels, uint32_t frame_floats) {
    const unsigned __int128 row = (unsigned __int128)n_streams * sizeof(float);
    return d_in && d_out && pl_ranges_overlap(d_in, row * channels * frames_capacity, d_out, row * frame_floats * out_capacity);
}

constexpr size_t kTruePeakTaps = 48;  // loudness/processor.rs:75

inline float true_peak_coefficient(size_t j, size_t factor) {  // :79-84
    const double offset = (double)j - (double)kTruePeakTaps * 0.5;
    const double window = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)j / (double)kTruePeakTaps));
    const double x = offset * M_PI / (double)factor;
    return (float)(window * std::sin(x) / x);
}
// TRUE_PEAK_FIRS (:90-97): the three interpolated phases of the 4x filter, the one of the 2x filter
inline void pl_true_peak_fir(float (&fir4)[12][3], float (&fir2)[24]) {
    for (size_t tap = 0; tap < 12; ++tap)
        for (size_t phase = 0; phase < 3; ++phase) fir4[tap][phase] = true_peak_coefficient(tap * 4 + phase + 1, 4);
    for (size_t tap = 0; tap < 24; ++tap) fir2[tap] = true_peak_coefficient(tap * 2 + 1, 2);
}

// A call's per-stream table, made on the host, to the device in one upload on the call's stream
template <class T>
inline void pl_upload_table(BlobStaging& staging, const std::vector<T>& calls, T* d_calls, hipStream_t stream) {
    staging.upload(calls.data(), calls.size() * sizeof(T), d_calls, stream);
}

}  // namespace omx
